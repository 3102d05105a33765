"""The yardstick of the route accounting tests against itself: route_model.route_sums (numpy, uint64) equals a
per-packet loop over Python ints written from the header's counter table (include/qgcm.h, qgcm_route_account),
on seeded batches holding every class of packet and on a 6-packet batch whose rows are written out by hand.
The table model the GPU tests pick their inputs with is checked against the cluster those tests rely on."""
import random

import numpy as np
import pytest

from route_model import (NO_PEER, RX, SWEEP_TABLES, TX, build_table, capacity, crosses_seam, probe_path, py_route_hash,
                         route_sums, sweep_case, sweep_wraps)


def loop_sums(direction, peer, lens, status, max_keys):
    """The counter table, one packet at a time, in Python ints."""
    totals = [0, 0, 0, 0]
    links = [[0, 0, 0, 0] for _ in range(max_keys)]
    for i in range(len(peer)):
        p, length = int(peer[i]), int(lens[i])
        if p == NO_PEER or p >= max_keys:
            totals[2] += 1
            continue
        delivered = True if status is None else int(status[i]) == 1
        if direction == RX and length < 28:
            delivered = False
        for row in (totals, links[p]):
            if delivered:
                row[0] += 1
                row[1] += 4 + length + 28 if direction == TX else 4 + length - 28
            else:
                row[2] += 1
                row[3] += 4 + length
    return totals, links


def mixed_batch(seed, n, max_keys):
    """Every class: a hot link, links sharing `peer & 255`, unresolved (QGCM_NO_PEER and values at or above
    max_keys), lengths around 28, lengths near 2^32, statuses 0, 1 and neither."""
    rng = random.Random(seed)
    links = [7, 7 + 256, 7 + 512, 0, max_keys - 1, 300, 301]
    peer, lens, status = [], [], []
    for _ in range(n):
        r = rng.random()
        peer.append(7 if r < 0.5 else NO_PEER if r < 0.55 else rng.choice([max_keys, 0x7FFFFFFF, 0xFFFFFFFE])
                    if r < 0.6 else rng.choice(links))
        r = rng.random()
        lens.append(rng.choice([0, 1, 27, 28, 29]) if r < 0.2 else rng.choice([0xFFFFFFFF, 0xFFFFFFF0, 0xFFFFFFE0])
                    if r < 0.25 else rng.randint(0, 1400))
        r = rng.random()
        status.append(0 if r < 0.15 else 7 if r < 0.17 else 1)
    return np.array(peer, np.uint32), np.array(lens, np.uint32), np.array(status, np.uint8)


@pytest.mark.parametrize("direction", [TX, RX], ids=["tx", "rx"])
@pytest.mark.parametrize("with_status", [True, False], ids=["status", "null"])
@pytest.mark.parametrize("seed, n, max_keys", [(1, 2000, 2048), (2, 2001, 2048), (3, 1937, 1024), (4, 1, 2048)])
def test_route_sums_equals_the_loop(direction, with_status, seed, n, max_keys):
    peer, lens, status = mixed_batch(seed, n, max_keys)
    if not with_status:
        status = None
    totals, links = route_sums(direction, peer, lens, status, max_keys)
    want_totals, want_links = loop_sums(direction, peer, lens, status, max_keys)
    assert totals.dtype == np.uint64 and links.dtype == np.uint64 and links.shape == (max_keys, 4)
    assert [int(v) for v in totals] == want_totals
    assert [[int(v) for v in row] for row in links] == want_links
    if n >= 1000:  # the batch holds what it says: every class moved a counter, a sum passed 2^32
        assert want_totals[0] and want_totals[2] and want_totals[1] > 1 << 32
        assert want_links[7][0] and want_links[7 + 256][0] and want_links[7 + 512][0] and want_links[max_keys - 1][0]
        if with_status:
            assert want_totals[3] > 1 << 32


def test_six_packets_by_hand():
    peer = np.array([1, 1, NO_PEER, 4, 3, 3], np.uint32)   # max_keys 4: peer 4 is unresolved
    lens = np.array([100, 0, 500, 77, 0xFFFFFFFF, 27], np.uint32)
    status = np.array([1, 0, 1, 1, 1, 1], np.uint8)
    cases = {
        # Tx: 4 + len + 28 delivered, 4 + len dropped
        (TX, True): ([3, 4294967518, 3, 4], {1: [1, 132, 1, 4], 3: [2, 4294967386, 0, 0]}),
        (TX, False): ([4, 4294967550, 2, 0], {1: [2, 164, 0, 0], 3: [2, 4294967386, 0, 0]}),
        # Rx: 4 + len - 28 delivered; len 0 and len 27 are dropped whatever their status
        (RX, True): ([2, 4294967347, 4, 35], {1: [1, 76, 1, 4], 3: [1, 4294967271, 1, 31]}),
        (RX, False): ([2, 4294967347, 4, 35], {1: [1, 76, 1, 4], 3: [1, 4294967271, 1, 31]}),
    }
    for (direction, with_status), (want_totals, want_links) in cases.items():
        for sums in (route_sums, loop_sums):
            totals, links = sums(direction, peer, lens, status if with_status else None, 4)
            assert [int(v) for v in totals] == want_totals, (direction, with_status, sums.__name__)
            for k in range(4):
                assert [int(v) for v in links[k]] == want_links.get(k, [0, 0, 0, 0]), (direction, with_status, k)


def test_empty_batch():
    totals, links = route_sums(TX, np.zeros(0, np.uint32), np.zeros(0, np.uint32), None, 8)
    assert not totals.any() and not links.any()


def ip4(a, b, c, d):
    return a | b << 8 | c << 16 | d << 24


def test_table_model_on_the_wrapping_cluster():
    """10.99.0.2 ... 10.99.0.9 share home slot 14 of a 16-entry table and fill slots 14, 15, 0 ... 5: the cluster
    the GPU wrap test depends on (that test asserts the same of whatever set it picks)."""
    ips = [ip4(10, 99, 0, k) for k in range(2, 10)]
    assert capacity(8) == 16 and [py_route_hash(ip) & 15 for ip in ips] == [14] * 8
    slots, wrapped = build_table([(ip, k) for k, ip in enumerate(ips)])
    assert wrapped
    assert [i for i, s in enumerate(slots) if s is not None] == [0, 1, 2, 3, 4, 5, 14, 15]
    assert [slots[i][0] for i in (14, 15, 0, 1, 2, 3, 4, 5)] == ips
    assert probe_path(slots, ips[0]) == [14] and probe_path(slots, ips[7]) == [14, 15, 0, 1, 2, 3, 4, 5]
    assert crosses_seam(probe_path(slots, ips[2])) and not crosses_seam(probe_path(slots, ips[1]))
    # a repeated ip overwrites in place
    slots2, _ = build_table([(ip, k) for k, ip in enumerate(ips)] + [(ips[3], 99)])
    assert capacity(9) == 32 and sum(s is not None for s in slots2) == 8
    assert [s[1] for s in slots2 if s is not None and s[0] == ips[3]] == [99]


def test_sweep_tables_wrap():
    """The random-address sweep of the GPU tests is not blind to the seam: 33 of its 64 tables step from the
    last slot to slot 0, 7 of them already while they are built."""
    assert sum(sweep_wraps(k) for k in range(SWEEP_TABLES)) == 33
    assert sum(build_table(list(sweep_case(k)[0].items()))[1] for k in range(SWEEP_TABLES)) == 7
    t, addrs, gateway = sweep_case(5)
    assert len(t) == 6 and len(addrs) == 256 and gateway not in t
    assert all((a in t) == (i % 2 == 0) for i, a in enumerate(addrs))


def test_hash_low_bit_is_constant_within_a_slash16():
    """An observation the GPU tests work around (they add tables of random 32-bit addresses): inside one /16 the
    low 16 bits of the address are fixed, so bit 0 of route_hash (h ^ h >> 15: bits 0 and 15 of the product) is
    too -- only every other slot is a home slot there."""
    assert len({py_route_hash(ip4(10, 99, c, d)) & 1 for c in range(0, 256, 5) for d in range(256)}) == 1
    assert len({py_route_hash(ip4(a, b, 0, 1)) & 1 for a in range(1, 60) for b in range(0, 256, 7)}) == 2
