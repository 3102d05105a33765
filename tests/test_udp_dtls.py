"""CPU: qgcm_udp_send_dtls / qgcm_udp_recv_dtls (quantum_amd/csrc/udp_batch.cpp) over loopback: split records go
out as one datagram each (the 21 header bytes, then the slot's bytes) and come back split, byte for byte; the
slots the send skips; datagrams that cannot be a record in a slot are dropped and counted.  No GPU."""
import ctypes as C
import socket

import numpy as np

from quantum_amd import _lib, dtls, route

STRIDE = 256


def open_pair():
    L = _lib.lib()
    rx = L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 20)
    tx = L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 20)
    assert rx >= 0 and tx >= 0
    return rx, tx, L.qgcm_udp_port(rx), L.qgcm_udp_port(tx)


def recv_all(fd, arena, lens, hdr, addrs, want, max_n=None):
    got = dropped = 0
    for _ in range(50):
        k, d = dtls.udp_recv_dtls(fd, arena.ctypes.data + got * STRIDE, STRIDE, (max_n or len(lens)) - got,
                                  lens[got:], hdr[got:], None if addrs is None else
                                  (_lib.PeerAddr * (len(lens) - got)).from_address(C.addressof(addrs) + 8 * got), 200)
        assert k >= 0
        got, dropped = got + k, dropped + d
        if got + dropped >= want:
            break
    return got, dropped


def test_round_trip_split_records():
    L = _lib.lib()
    rx, tx, rx_port, tx_port = open_pair()
    try:
        rng = np.random.default_rng(0xD7151000)
        n = 40
        arena = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
        hdr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        lens = (1 + (np.arange(n) * 37) % STRIDE).astype(np.uint32)
        lens[5] = STRIDE                      # a full slot
        lens[6] = 0                           # nothing to send
        status = np.ones(n, np.uint8)
        status[7] = 0                         # rejected by the seal
        peer = np.zeros(n, np.uint32)
        peer[8] = _lib.NO_PEER
        addrs = route.peer_addrs([("127.0.0.1", rx_port)])
        sent = dtls.udp_send_dtls(tx, arena.ctypes.data, STRIDE, n, lens, hdr, status, peer, addrs, 1)
        keep = [i for i in range(n) if i not in (6, 7, 8)]
        assert sent == len(keep)
        r_arena = np.full((n, STRIDE), 0xEE, np.uint8)
        r_hdr = np.full((n, 32), 0xEE, np.uint8)
        r_lens = np.zeros(n, np.uint32)
        r_addrs = (_lib.PeerAddr * n)()
        got, dropped = recv_all(rx, r_arena, r_lens, r_hdr, r_addrs, sent)
        assert (got, dropped) == (sent, 0)
        for k, i in enumerate(keep):  # loopback keeps the order
            assert r_lens[k] == lens[i]
            assert np.array_equal(r_hdr[k, :21], hdr[i, :21]) and not r_hdr[k, 21:].any()
            assert np.array_equal(r_arena[k, :lens[i]], arena[i, :lens[i]])
            assert (r_arena[k, lens[i]:] == 0xEE).all()
            assert r_addrs[k].ip == addrs[0].ip and socket.ntohs(r_addrs[k].port) == tx_port
        assert (r_arena[got:] == 0xEE).all() and (r_hdr[got:] == 0xEE).all()
        # a peer past the address table fails the call before anything is sent
        peer[3] = 1
        assert dtls.udp_send_dtls(tx, arena.ctypes.data, STRIDE, n, lens, hdr, status, peer, addrs, 1) == -1
        assert dtls.udp_recv_dtls(rx, r_arena.ctypes.data, STRIDE, n, r_lens, r_hdr, None, 50) == (0, 0)
    finally:
        L.qgcm_udp_close(rx)
        L.qgcm_udp_close(tx)


def test_short_and_long_datagrams_are_dropped_and_counted():
    L = _lib.lib()
    rx, tx, rx_port, _ = open_pair()
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        good = [bytes([i]) * (21 + k) for i, k in ((1, 1), (2, 100), (3, STRIDE))]
        # 21 bytes: a header with no record behind it; 1: a stray byte; STRIDE + 22: one byte too long for a slot
        seq = [good[0], b"\x09" * 21, good[1], b"\x08", b"\x07" * (21 + STRIDE + 1), good[2]]
        for d in seq:
            s.sendto(d, ("127.0.0.1", rx_port))
        n = 8
        arena = np.full((n, STRIDE), 0xEE, np.uint8)
        hdr = np.full((n, 32), 0xEE, np.uint8)
        lens = np.zeros(n, np.uint32)
        got, dropped = recv_all(rx, arena, lens, hdr, None, len(seq))
        assert (got, dropped) == (3, 3)
        for k, d in enumerate(good):  # the slots filled stay dense
            assert lens[k] == len(d) - 21
            assert hdr[k, :21].tobytes() == d[:21] and arena[k, :lens[k]].tobytes() == d[21:]
        # max_n bounds a call: two of three, then the third
        for d in good:
            s.sendto(d, ("127.0.0.1", rx_port))
        got, dropped = recv_all(rx, arena, lens, hdr, None, 2, max_n=2)
        assert (got, dropped) == (2, 0)
        assert dtls.udp_recv_dtls(rx, arena.ctypes.data, STRIDE, n, lens, hdr, None, 200) == (1, 0)
        assert lens[0] == STRIDE
    finally:
        s.close()
        L.qgcm_udp_close(rx)
        L.qgcm_udp_close(tx)


def test_argument_errors():
    L = _lib.lib()
    buf = np.zeros(64, np.uint8)
    lens = np.zeros(1, np.uint32)
    assert L.qgcm_udp_send_dtls(-1, buf.ctypes.data, 64, 1, lens.ctypes.data, buf.ctypes.data, None,
                                lens.ctypes.data, None, 0) == -1
    assert L.qgcm_udp_send_dtls(0, None, 64, 1, lens.ctypes.data, buf.ctypes.data, None, lens.ctypes.data, None, 0) == -1
    assert L.qgcm_udp_recv_dtls(-1, buf.ctypes.data, 64, 1, lens.ctypes.data, buf.ctypes.data, None, 0, None) == -1
    assert L.qgcm_udp_recv_dtls(0, None, 64, 1, lens.ctypes.data, buf.ctypes.data, None, 0, None) == -1
    assert L.qgcm_udp_recv_dtls(0, buf.ctypes.data, 0, 1, lens.ctypes.data, buf.ctypes.data, None, 0, None) == -1
