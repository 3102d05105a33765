"""CPU, loopback: qgcm_udp_recv_gro takes what qgcm_udp_send_plan put on the wire -- coalesced by the kernel
where it does that -- into a packed area, and qgcm_gro_unpack_cpu makes the sent datagrams of it again."""
import socket

import numpy as np
import pytest

import gro_model as M
from quantum_amd import _lib, route
from send_plan_wire import STRIDE, Wire

PLAIN = (0, 1, 77)  # lengths no train below has


@pytest.fixture
def wire():
    w = Wire(1)
    yield w
    w.close()


def trains_batch(counts_and_lens, seed=1):
    """Slots, lengths and the plan of trains of (count, seg_len) to peer 0, in slot order; every datagram differs."""
    n = sum(c for c, _ in counts_and_lens)
    slots = np.random.default_rng(seed).integers(0, 256, (n, STRIDE), dtype=np.uint8)
    lens, trains, at = np.zeros(n, np.uint32), [], 0
    for c, L in counts_and_lens:
        lens[at:at + c] = L
        trains.append((at, c, 0, L))
        at += c
    return slots, lens, np.arange(n, dtype=np.uint32), np.array(trains, np.uint32)


def send(wire, batch):
    slots, lens, order, trains = batch
    assert wire.send(slots, lens, order, trains) == len(lens)
    return [slots[i, :lens[i]].tobytes() for i in range(len(lens))]


def recv_call(fd, packed_cap=1 << 20, max_bufs=256, max_n=1024, timeout_ms=1000):
    """One qgcm_udp_recv_gro call -> (n, bufs[:n_bufs], out, datagrams), the datagrams by qgcm_gro_unpack_cpu."""
    packed = np.zeros(packed_cap, np.uint8)
    bufs = np.zeros((max_bufs, 4), np.uint32)
    out = np.zeros(3, np.uint64)
    n = route.udp_recv_gro(fd, packed, bufs, max_n, timeout_ms, out)
    assert n >= 0
    bufs = bufs[:int(out[0])]
    if n == 0:
        assert out.tolist() == [0, 0, 0]
        return 0, bufs, out, []
    assert M.table_ok(bufs, n) and int(out[2]) == 0
    assert all(int(b[0]) % 16 == 0 for b in bufs)
    assert int(out[1]) == int(bufs[-1][0]) + int(bufs[-1][1]) and int(out[1]) <= packed_cap
    arena, lens = M.fresh(n, STRIDE)
    route.gro_unpack_cpu(packed, int(out[1]), bufs, n, arena, STRIDE, lens)
    assert lens.max() <= STRIDE
    return n, bufs, out, [arena[i * STRIDE:i * STRIDE + lens[i]].tobytes() for i in range(n)]


def recv_all(fd, want, **kw):
    got, tables = [], []
    while len(got) < want:
        n, bufs, _, dgrams = recv_call(fd, **kw)
        if n == 0:
            break
        got += dgrams
        tables.append(bufs)
    assert recv_call(fd, timeout_ms=10, **{k: v for k, v in kw.items() if k != "timeout_ms"})[0] == 0
    return got, tables


def mixed_traffic(wire):
    """Trains of 1, 2, 45 and 64 segments from the wire's sender and plain datagrams of 0, 1 and 77 bytes from a
    socket of its own -> what each sender sent, in its order."""
    plain = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        port = wire.L.qgcm_udp_port(wire.rx[0])
        sent_plain = []
        trains = send(wire, trains_batch(((45, 1382), (1, 300)), 2))
        for L in PLAIN:
            sent_plain.append(bytes(range(L)))
            plain.sendto(sent_plain[-1], ("127.0.0.1", port))
        trains += send(wire, trains_batch(((64, 100), (2, 200)), 3))
    finally:
        plain.close()
    return trains, sent_plain


def check_mixed(got, trains, sent_plain):
    assert len(got) == len(trains) + len(sent_plain)
    assert [d for d in got if len(d) in PLAIN] == sent_plain
    assert [d for d in got if len(d) not in PLAIN] == trains


def test_every_datagram_arrives_with_gro_on(wire):
    route.udp_gro(wire.rx[0], True)
    trains, sent_plain = mixed_traffic(wire)
    got, _ = recv_all(wire.rx[0], len(trains) + len(sent_plain))
    check_mixed(got, trains, sent_plain)


def test_with_gro_off_the_same_bytes_arrive_as_lone_buffers(wire):
    route.udp_gro(wire.rx[0], True)
    route.udp_gro(wire.rx[0], False)
    trains, sent_plain = mixed_traffic(wire)
    got, tables = recv_all(wire.rx[0], len(trains) + len(sent_plain))
    check_mixed(got, trains, sent_plain)
    bufs = np.concatenate(tables)
    assert len(bufs) == len(got) and np.all(bufs[:, 2] == 0)


def test_without_the_option_ever_set(wire):
    trains, sent_plain = mixed_traffic(wire)
    got, tables = recv_all(wire.rx[0], len(trains) + len(sent_plain))
    check_mixed(got, trains, sent_plain)
    assert np.all(np.concatenate(tables)[:, 2] == 0)


@pytest.mark.parametrize("gro", (True, False))
def test_stops_with_fewer_than_64_slots_left(wire, gro):
    route.udp_gro(wire.rx[0], gro)
    sent = send(wire, trains_batch(((45, 1382), (45, 1382), (45, 700)), 4))
    got = []
    for _ in range(len(sent)):
        n, bufs, _, dgrams = recv_call(wire.rx[0], max_n=100)
        if n == 0:
            break
        # it stopped because the slots ran short, or it took all there was
        assert n <= 100 and (100 - n < _lib.GRO_SEGS or len(got) + n == len(sent))
        got += dgrams
    assert got == sent
    assert recv_call(wire.rx[0], timeout_ms=10)[0] == 0


@pytest.mark.parametrize("gro", (True, False))
def test_stops_with_less_than_64k_of_room_left(wire, gro):
    route.udp_gro(wire.rx[0], gro)
    sent = send(wire, trains_batch(((45, 1382), (3, 64)), 5))
    got, calls = [], 0
    while len(got) < len(sent):
        # room for one receive: after the first buffer fewer than 65536 bytes are left
        n, bufs, out, dgrams = recv_call(wire.rx[0], packed_cap=65536 + 15)
        assert n > 0 and len(bufs) == 1
        got += dgrams
        calls += 1
    assert got == sent and calls >= 2
    n, bufs, out, dgrams = recv_call(wire.rx[0], max_bufs=2, timeout_ms=10)
    assert n == 0


def test_stops_at_max_bufs(wire):
    sent = send(wire, trains_batch(((5, 64),), 6))  # the option is off: five lone buffers
    n, bufs, _, first = recv_call(wire.rx[0], max_bufs=2)
    assert n == 2 and len(bufs) == 2
    rest, _ = recv_all(wire.rx[0], 3)
    assert first + rest == sent


def test_arguments(wire):
    L = _lib.lib()
    packed, bufs, out = np.zeros(1 << 17, np.uint8), np.zeros((4, 4), np.uint32), np.full(3, 9, np.uint64)
    assert route.udp_recv_gro(wire.rx[0], packed, bufs, 64, 10, out) == 0 and out.tolist() == [0, 0, 0]  # timeout
    assert route.udp_recv_gro(wire.rx[0], packed, bufs, 64, 10) == 0                                       # no out
    assert route.udp_recv_gro(wire.rx[0], packed, bufs, 63, 10, out) == -1     # never 64 slots left
    assert route.udp_recv_gro(wire.rx[0], packed[:65535], bufs, 64, 10, out) == -1  # never 64 KiB of room
    assert route.udp_recv_gro(wire.rx[0], packed, bufs[:0], 64, 10, out) == -1
    assert route.udp_recv_gro(-1, packed, bufs, 64, 10, out) == -1
    assert L.qgcm_udp_recv_gro(wire.rx[0], None, 1 << 17, bufs.ctypes.data, 4, 64, 10, None) == -1
    assert L.qgcm_udp_gro(-1, 1) < 0
    with pytest.raises(OSError):
        route.udp_gro(-1)


def test_at_least_one_buffer_was_coalesced(wire):
    if not M.host_coalesces():
        pytest.skip("this host's loopback does not coalesce: a UDP_SEGMENT train of three came back from a plain "
                    "UDP_GRO socket as something other than one buffer with a control message of 10")
    route.udp_gro(wire.rx[0], True)
    sent = send(wire, trains_batch(((45, 1382), (3, 100)), 7))
    got, tables = recv_all(wire.rx[0], len(sent))
    assert got == sent
    bufs = np.concatenate(tables)
    assert len(bufs) < len(sent) and np.any(bufs[:, 2] != 0)
