"""CPU: qgcm_deliver_pack_cpu writes exactly what tests/deliver_pack_model.py writes -- the packed area, the
table and the counts, over sentinels -- and qgcm_tun_write_packed writes Raw[4 : 4 + L] of every record in
order (over a datagram socket pair, where every write is one datagram; and over a real TUN queue where the
kernel allows one)."""
import socket

import numpy as np
import pytest

import deliver_pack_model as M
from quantum_amd import _lib, route


def cpu_pack(case, stride, packed_cap, room=None):
    arena, lens, peer, status = case
    n = len(lens)
    packed, recs, _ = M.fresh(n, packed_cap if room is None else room)
    got_recs, got_bytes = route.deliver_pack_cpu(arena, stride, n, lens, peer, status, packed[:packed_cap], recs)
    return packed, got_recs, got_bytes, recs


def check(case, stride, packed_cap=None):
    arena, lens, peer, status = case
    n = len(lens)
    full = M.need(lens, status, stride)
    cap = full if packed_cap is None else packed_cap
    want_packed = np.full(cap + 64, M.SENTINEL, np.uint8)
    want_recs, (m, total) = M.pack(arena, stride, n, lens, peer, status, want_packed, cap)
    assert total == full
    fast_packed = np.full(cap + 64, M.SENTINEL, np.uint8)  # the vectorised model the GPU tests use for large batches
    fast_recs, fast_counts = M.pack_fast(arena, stride, n, lens, peer, status, fast_packed, cap)
    assert np.array_equal(fast_recs, want_recs) and fast_counts == (m, total) and np.array_equal(fast_packed, want_packed)
    packed, got_recs, got_bytes, recs = cpu_pack(case, stride, cap, cap + 64)
    assert got_bytes == full and len(got_recs) == m
    assert np.array_equal(got_recs, want_recs)
    assert np.array_equal(packed, want_packed)  # whole: padding zeroed, the bytes behind untouched
    assert np.all(recs[m:] == M.REC_SENTINEL)
    return want_recs, want_packed


@pytest.mark.parametrize("stride", (1536, 1388))
def test_edges(stride):
    recs, _ = check(M.edge_case(stride), stride)
    assert {0, 1, 11, 12, 13, 1382, stride - 4} <= set(recs[:, 1].tolist())
    assert np.all(recs[:, 0] % 16 == 0) and np.all(np.diff(recs[:, 2].astype(np.int64)) > 0)


def test_random_batch():
    check(M.random_batch(0xB47C, 3000, 1536), 1536)
    check(M.random_batch(0xB47D, 1000, 64, max_len=70, drop=0.3), 64)  # lengths past the slot are left out


def test_status_null_delivers_every_packet_that_fits():
    case = M.random_batch(0x5747, 500, 1388, max_len=1400, with_status=False)
    recs, _ = check(case, 1388)
    assert len(recs) == int(np.sum(case[1] <= 1384)) < 500


def test_packed_cap_cuts_mid_batch():
    case = M.edge_case(1536)
    full, _ = check(case, 1536)
    k = len(full) // 2
    start, size = int(full[k, 0]), M.rec_bytes(int(full[k, 1]))
    for cap in (start, start + size - 1, start + size, 0):
        recs, _ = check(case, 1536, cap)
        fitted = int(np.sum(recs[:, 0] != M.NO_ROOM))
        assert fitted == (0 if cap == 0 else k + (cap == start + size))
        assert np.all(recs[fitted:, 0] == M.NO_ROOM) and np.array_equal(recs[:, 1:], full[:, 1:])


def test_bad_arguments():
    L = _lib.lib()
    arena, lens, peer, status = M.edge_case(1536)
    packed, recs, counts = M.fresh(len(lens), 1 << 16)
    args = [arena.ctypes.data, 1536, len(lens), lens.ctypes.data, peer.ctypes.data, status.ctypes.data, packed.ctypes.data,
            packed.size, recs.ctypes.data, counts.ctypes.data]

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_deliver_pack_cpu(*a)

    assert call(a1=1538) == _lib.QGCM_E_ARG and call(a1=0) == _lib.QGCM_E_ARG
    assert call(a7=(1 << 32) - 15) == _lib.QGCM_E_ARG
    for k in (0, 3, 4, 6, 8, 9):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert np.all(packed == M.SENTINEL) and np.all(recs == M.REC_SENTINEL) and np.all(counts == M.COUNT_SENTINEL)
    assert call(a2=0) == 0 and counts.tolist() == [0, 0]


# ---- qgcm_tun_write_packed ----

def packed_case():
    arena, lens, peer, status = M.edge_case(1536)
    packed = np.full(1 << 16, M.SENTINEL, np.uint8)
    recs, (m, total) = M.pack(arena, 1536, len(lens), lens, peer, status, packed, packed.size)
    want = [bytes(arena[i * 1536 + 4:i * 1536 + 4 + L]) for _, L, i, _ in recs.tolist()]
    assert any(len(w) == 0 for w in want)
    return packed, total, recs, want


def test_tun_write_packed_over_a_datagram_socket_pair():
    packed, total, recs, want = packed_case()
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
        b.settimeout(2.0)
        got = []
        for k in range(0, len(recs), 8):  # a datagram socket queues about ten: eight records a call
            part = np.ascontiguousarray(recs[k:k + 8])
            assert route.tun_write_packed(a.fileno(), packed, total, part) == len(part)
            got += [b.recv(4096) for _ in part]
        assert got == want  # the order, the bytes Raw[4 : 4 + L], the zero-length packet as an empty datagram
        b.setblocking(False)
        with pytest.raises(BlockingIOError):
            b.recv(16)
        # a table that reaches past packed_len: -1, nothing written
        bad = recs.copy()
        bad[len(bad) // 2, 0] = total
        assert route.tun_write_packed(a.fileno(), packed, total, bad) == -1
        cut = recs.copy()
        cut[-1, 0] = M.NO_ROOM  # a record that did not fit
        assert route.tun_write_packed(a.fileno(), packed, total, cut) == -1
        assert route.tun_write_packed(a.fileno(), packed, int(recs[-1, 0]) + 4 + int(recs[-1, 1]) - 1, recs) == -1
        with pytest.raises(BlockingIOError):
            b.recv(16)
        assert route.tun_write_packed(-1, packed, total, recs) == -1
        assert route.tun_write_packed(a.fileno(), packed, total, recs[:0]) == 0
    finally:
        a.close()
        b.close()


def test_tun_write_packed_ends_at_a_failed_write():
    """A write the kernel refuses ends the batch there, as in qgcm_tun_write_slots: a non-blocking socket whose
    peer does not read takes the datagrams its queue holds and refuses the next; the call returns how many went
    out, and they are the first ones.  With the peer closed every write is refused: -1."""
    packed, total, recs, want = packed_case()
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        a.setblocking(False)
        done = route.tun_write_packed(a.fileno(), packed, total, recs)
        assert 0 < done <= len(recs)
        b.setblocking(False)
        assert [b.recv(4096) for _ in range(done)] == want[:done]
        with pytest.raises(BlockingIOError):
            b.recv(16)
        b.close()
        assert route.tun_write_packed(a.fileno(), packed, total, recs) == -1
    finally:
        a.close()
        b.close()


def test_tun_write_packed_reaches_a_socket():
    """Shaped like tests/test_tun_batch.py: IPv4 packets written to a TUN queue from a packed area reach a local
    UDP socket; skipped where the kernel refuses the device."""
    import ctypes as C

    from test_tun_batch import HOST_IP, PEER_IP, STRIDE, _ipv4_udp

    L = _lib.lib()
    fds = (C.c_int * 2)()
    name = C.create_string_buffer(16)
    rc = L.qgcm_tun_open(b"qgcmp%d", 2, fds, name, 16)
    if rc < 0:
        pytest.skip(f"TUN device refused (errno {-rc})")
    try:
        rc = L.qgcm_tun_up(name.value, HOST_IP.encode(), 24, 1433)
        if rc < 0:
            pytest.skip(f"TUN link set-up refused (errno {-rc})")
        rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        rx.bind((HOST_IP, 0))
        rx.settimeout(2.0)
        port = rx.getsockname()[1]
        n = 24
        arena = np.zeros(n * STRIDE, np.uint8)
        lens, status = np.zeros(n, np.uint32), np.ones(n, np.uint8)
        want = []
        for i in range(n):
            payload = bytes([i]) * (10 + 40 * i)
            pkt = _ipv4_udp(PEER_IP, HOST_IP, 7000, port, payload)
            arena[i * STRIDE + 4:i * STRIDE + 4 + len(pkt)] = np.frombuffer(pkt, np.uint8)
            lens[i] = len(pkt)
            if i % 5 == 2:
                status[i] = 0  # dropped: never written
            else:
                want.append(payload)
        packed = np.zeros(n * STRIDE, np.uint8)
        recs, total = route.deliver_pack_cpu(arena, STRIDE, n, lens, np.zeros(n, np.uint32), status, packed)
        assert route.tun_write_packed(fds[1], packed, total, recs) == len(want)
        got = [rx.recv(4096) for _ in want]
        rx.close()
        assert got == want
    finally:
        for fd in fds:
            L.qgcm_tun_close(fd)
