"""CPU, loopback: qgcm_udp_send_plan sends a planned batch as one message per train (UDP_SEGMENT for trains of
more than one datagram) and every receiver gets its peer's datagrams byte for byte, in arena order; a train
the kernel refuses goes out as single datagrams; a plan that does not fit the batch sends nothing."""
import numpy as np
import pytest

import send_plan_model as M
from send_plan_wire import STRIDE, Wire, expected, gso_probe

PEERS = 3


@pytest.fixture()
def wire():
    w = Wire(PEERS)
    yield w
    w.close()


@pytest.fixture(scope="module")
def gso():
    return gso_probe()


def hand_batch(n=90, seed=11):
    """n interleaved packets of three peers, lengths from {36, 700, 1382} in short same-length stretches, a few
    unsendable ones between them."""
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
    lens = np.array([(36, 700, 1382)[(i // 12) % 3] for i in range(n)], np.uint32)
    peer = np.array([i % PEERS for i in range(n)], np.uint32)
    lens[20] = 64  # a train of one in the middle of a stretch
    lens[[7, 40]] = 0
    peer[[13, 61]] = M.NO_PEER
    return slots, lens, peer


def check_arrivals(wire, slots, lens, peer):
    for p in range(PEERS):
        want = expected(slots, lens, peer, p)
        assert wire.drain(p, len(want)) == want, p


def test_hand_made_plan_three_receivers(wire, gso):
    slots, lens, peer = hand_batch()
    order, trains = M.plan(lens, peer, PEERS)
    assert any(t[1] > 1 for t in trains) and any(t[1] == 1 for t in trains)
    stats = np.zeros(3, np.uint64)
    assert wire.send(slots, lens, order, trains, stats) == len(order)
    check_arrivals(wire, slots, lens, peer)
    if gso:  # without UDP_SEGMENT every train falls back, and the datagrams above arrived all the same
        assert stats.tolist() == [len(trains), sum(t[1] > 1 for t in trains), 0]


def test_gso_off_sends_the_same_datagrams(wire, monkeypatch):
    monkeypatch.setenv("QGCM_UDP_GSO", "0")
    slots, lens, peer = hand_batch()
    order, trains = M.plan(lens, peer, PEERS)
    stats = np.zeros(3, np.uint64)
    assert wire.send(slots, lens, order, trains, stats) == len(order)
    check_arrivals(wire, slots, lens, peer)
    assert stats.tolist() == [len(order), 0, 0]


def test_a_refused_train_goes_out_as_singles(wire):
    """200 segments are more than any kernel takes in one message (64 or 128): EINVAL, or no UDP_SEGMENT at all."""
    n = 200
    slots = np.random.default_rng(5).integers(0, 256, (n, STRIDE), dtype=np.uint8)
    lens, peer = np.full(n, 20, np.uint32), np.full(n, 1, np.uint32)
    stats = np.zeros(3, np.uint64)
    assert wire.send(slots, lens, np.arange(n), [(0, n, 1, 20)], stats) == n
    assert wire.drain(1, n) == expected(slots, lens, peer, 1)
    assert stats.tolist() == [n, 0, 1]


def test_fallback_keeps_the_trains_behind_it(wire, gso):
    """A refused train between two good ones: all three arrive, in plan order per peer."""
    n = 220
    slots = np.random.default_rng(6).integers(0, 256, (n, STRIDE), dtype=np.uint8)
    lens, peer = np.full(n, 20, np.uint32), np.array([0] * 10 + [1] * 200 + [2] * 10, np.uint32)
    trains = [(0, 10, 0, 20), (10, 200, 1, 20), (210, 10, 2, 20)]
    stats = np.zeros(3, np.uint64)
    assert wire.send(slots, lens, np.arange(n), trains, stats) == n
    check_arrivals(wire, slots, lens, peer)
    if gso:
        assert stats.tolist() == [202, 2, 1]


def test_a_plan_that_does_not_fit_sends_nothing(wire):
    slots, lens, peer = hand_batch()
    order, trains = M.plan(lens, peer, PEERS)
    n, m = len(lens), len(order)
    big = next(k for k, t in enumerate(trains) if t[1] > 2)

    def broken(**kw):
        o, t, ln = list(order), [list(x) for x in trains], lens.copy()
        if "order" in kw:
            o[kw["order"][0]] = kw["order"][1]
        if "train" in kw:
            k, field, value = kw["train"]
            t[k][field] = value
        if "len" in kw:
            ln[kw["len"][0]] = kw["len"][1]
        return wire.send(slots, ln, o, t, None, kw.get("n_addrs"))

    member = order[trains[big][0] + 1]
    assert broken(len=(member, int(lens[member]) - 1)) == -1  # a member whose length is not seg_len
    assert broken(train=(big, 3, trains[big][3] + 1)) == -1   # ... seen from the train
    assert broken(order=(0, n)) == -1                         # an index past the batch
    assert broken(order=(m - 1, 0xFFFFFFFF)) == -1
    assert broken(train=(len(trains) - 1, 1, trains[-1][1] + 1)) == -1  # a train running past m
    assert broken(train=(big, 0, 0xFFFFFFFF)) == -1                     # ... by wrapping
    assert broken(n_addrs=PEERS - 1) == -1                    # a peer at n_addrs
    assert broken(train=(big, 2, PEERS)) == -1                # ... and past it
    assert broken(train=(big, 1, 0)) == -1                    # counts of 0 and 1025
    assert broken(train=(big, 1, 1025)) == -1
    # an empty datagram is never sendable, whatever the lengths say
    empty = order[trains[big][0]:trains[big][0] + trains[big][1]]
    zeroed = lens.copy()
    zeroed[empty] = 0
    t0 = [list(x) for x in trains]
    t0[big][3] = 0
    assert wire.send(slots, zeroed, order, t0) == -1
    # a segment size travels as 16 bits: no train of several 65536-byte members (one alone may be that long)
    wide = np.zeros((2, 65536), np.uint8)
    assert wire.send(wide, np.full(2, 65536, np.uint32), [0, 1], [(0, 2, 0, 65536)]) == -1
    # a slot cannot hold more than stride bytes
    assert wire.send(slots[:, :64].copy(), lens, order, trains) == -1
    assert wire.nothing_arrived()
    assert wire.send(slots, lens, order, trains) == m  # and the plan as made goes through
    check_arrivals(wire, slots, lens, peer)
