"""CPU, loopback: qgcm_udp_send_packed sends a packed batch as one message per train with one iovec (UDP_SEGMENT
for trains of more than one datagram) and every receiver gets what qgcm_udp_send_plan delivers for the same batch:
its peer's datagrams byte for byte, in arena order; a train the kernel refuses goes out as single datagrams cut
from the packed bytes; a table that does not fit the packed area sends nothing."""
import numpy as np
import pytest

import send_plan_model as P
import train_pack_model as M
from quantum_amd import route
from send_plan_wire import STRIDE, Wire, expected, gso_probe
from test_udp_send_plan import PEERS, hand_batch


@pytest.fixture()
def wire():
    w = Wire(PEERS)
    yield w
    w.close()


@pytest.fixture(scope="module")
def gso():
    return gso_probe()


def packed_of(slots, order, trains):
    """The model's pack of a plan over `slots` (n, stride) -> (packed, ptrains)."""
    n, stride = slots.shape
    order, trains = np.array(order, np.uint32), np.array(trains, np.uint32).reshape(-1, 4)
    packed = np.zeros(M.need(trains), np.uint8)
    ptrains, (t, total) = M.pack(slots.reshape(-1), stride, n, order, trains, len(order), len(trains), packed, packed.size)
    assert total == packed.size and t == len(trains)
    return packed, ptrains


def send(wire, packed, ptrains, stats=None, packed_len=None, n_addrs=None):
    return route.udp_send_packed(wire.tx, packed, packed.size if packed_len is None else packed_len,
                                 np.ascontiguousarray(ptrains, np.uint32).reshape(-1, 4), wire.addrs,
                                 wire.n_addrs if n_addrs is None else n_addrs, stats)


def arrivals(wire, slots, lens, peer):
    return [wire.drain(p, len(expected(slots, lens, peer, p))) for p in range(PEERS)]


def test_the_same_datagrams_as_the_planned_sender(wire, gso):
    slots, lens, peer = hand_batch()
    order, trains = P.plan(lens, peer, PEERS)
    assert any(t[1] > 1 for t in trains) and any(t[1] == 1 for t in trains)
    assert wire.send(slots, lens, order, trains) == len(order)
    planned = arrivals(wire, slots, lens, peer)
    assert planned == [expected(slots, lens, peer, p) for p in range(PEERS)]
    packed, ptrains = packed_of(slots, order, trains)
    stats = np.zeros(3, np.uint64)
    assert send(wire, packed, ptrains, stats) == len(order)
    assert arrivals(wire, slots, lens, peer) == planned
    if gso:  # without UDP_SEGMENT every train falls back, and the datagrams above arrived all the same
        assert stats.tolist() == [len(trains), sum(t[1] > 1 for t in trains), 0]


def test_gso_off_sends_the_same_datagrams(wire, monkeypatch):
    monkeypatch.setenv("QGCM_UDP_GSO", "0")
    slots, lens, peer = hand_batch()
    order, trains = P.plan(lens, peer, PEERS)
    assert wire.send(slots, lens, order, trains) == len(order)
    planned = arrivals(wire, slots, lens, peer)
    packed, ptrains = packed_of(slots, order, trains)
    stats = np.zeros(3, np.uint64)
    assert send(wire, packed, ptrains, stats) == len(order)
    assert arrivals(wire, slots, lens, peer) == planned == [expected(slots, lens, peer, p) for p in range(PEERS)]
    assert stats.tolist() == [len(order), 0, 0]


def test_a_refused_train_goes_out_as_singles_and_the_trains_behind_it_still_go(wire, gso):
    """200 segments are more than any kernel takes in one message (64 or 128): EINVAL, or no UDP_SEGMENT at all.
    The refused train sits between two good ones: all three arrive, in table order per peer."""
    n = 220
    slots = np.random.default_rng(6).integers(0, 256, (n, STRIDE), dtype=np.uint8)
    lens, peer = np.full(n, 20, np.uint32), np.array([0] * 10 + [1] * 200 + [2] * 10, np.uint32)
    trains = [(0, 10, 0, 20), (10, 200, 1, 20), (210, 10, 2, 20)]
    packed, ptrains = packed_of(slots, np.arange(n), trains)
    assert ptrains[:, 0].tolist() == [0, 208, 4208]
    stats = np.zeros(3, np.uint64)
    assert send(wire, packed, ptrains, stats) == n
    assert arrivals(wire, slots, lens, peer) == [expected(slots, lens, peer, p) for p in range(PEERS)]
    if gso:
        assert stats.tolist() == [202, 2, 1]
    else:
        assert stats[0] == n and stats[1] == 0


def test_a_table_that_does_not_fit_sends_nothing(wire):
    slots, lens, peer = hand_batch()
    order, trains = P.plan(lens, peer, PEERS)
    packed, ptrains = packed_of(slots, order, trains)
    big = next(k for k, t in enumerate(ptrains.tolist()) if t[1] > 2)

    def broken(k, field, value, **kw):
        bad = ptrains.copy()
        bad[k, field] = value
        return send(wire, packed, bad, **kw)

    assert broken(big, 0, M.NO_ROOM) == -1                           # a train that did not fit
    assert broken(len(ptrains) - 1, 0, int(ptrains[-1, 0]) + 16) == -1  # an entry past packed_len
    last_end = int(ptrains[-1, 0]) + int(ptrains[-1, 1]) * int(ptrains[-1, 3])
    assert send(wire, packed, ptrains, packed_len=last_end - 1) == -1
    assert broken(big, 2, PEERS) == -1                               # a peer at n_addrs
    assert send(wire, packed, ptrains, n_addrs=PEERS - 1) == -1
    assert broken(big, 1, 0) == -1 and broken(big, 1, 1025) == -1    # counts of 0 and 1025
    assert broken(big, 3, 0) == -1                                   # an empty datagram is never sendable
    assert broken(big, 3, 0xFFFFFFFF) == -1                          # count * seg_len in 64 bits
    # a segment size travels as 16 bits: no train of several 65536-byte members
    wide = np.zeros(2 * 65536, np.uint8)
    assert send(wire, wide, [(0, 2, 0, 65536)]) == -1
    assert route.udp_send_packed(-1, packed, packed.size, ptrains, wire.addrs, PEERS) == -1
    assert wire.nothing_arrived()
    assert send(wire, packed, ptrains, packed_len=last_end) == len(order)  # and the table as made goes through
    assert arrivals(wire, slots, lens, peer) == [expected(slots, lens, peer, p) for p in range(PEERS)]
