"""The route kernels at their edges (include/qgcm.h "routes resolved on the GPU"): probes that wrap past the
table's last slot, net / mask / gateway shapes, lengths that break 32-bit arithmetic, waves built lane by lane
for the accounting kernel (links sharing an LDS entry, sums past 2^32, workgroups that walk several tiles), and
the second chunk of the host pipelines.

Every expected peer comes from a dict and the rule of router/router.go:21-31, every expected counter from
route_model.route_sums (the header's counter table in numpy, checked on the CPU by test_route_model.py), sealed
bytes from the oracle.  route_model's copy of the table layout only picks inputs and asserts that they still
collide and wrap as intended.  All comparisons are exact.
"""
import random

import numpy as np
import pytest

from oracle import oracle as O
from route_model import (RX, SWEEP_TABLES, TX, build_table, capacity, crosses_seam, probe_path, py_route_hash, route_sums,
                         sweep_case, sweep_wraps)
from test_gpu_route import (DESC, GATEWAY, MASK, NET, NO_PEER, OUTSIDE, OWN, PEERS, STRIDE, UNIVERSE, UNMAPPED_GW, le,
                            nodes, oracle_seal, torch, wire_batch)  # noqa: F401  (nodes, torch: fixtures)

pytestmark = pytest.mark.gpu


# ---- resolve ----

def rule_net(t, net, mask, gateway, addr):
    """router.go:21-31 over the dict; None = no mapping."""
    return t.get(addr if (addr & mask) == (net & mask) else gateway)


def u32_tensor(torch, a):
    """A device int32 tensor holding the bits of uint32 values (lengths up to 2^32 - 1, QGCM_NO_PEER)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


def slots_with(rng, n, stride, addrs, outgoing):
    """n random slots (an (n, stride) array) carrying addrs[i] where the resolve reads it: Packet[16:20] of an
    outgoing slot (Raw[20:24]), Raw[0:4] of an incoming one."""
    arena = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    col = 20 if outgoing else 0
    arena[:, col:col + 4] = np.array(addrs, "<u4").view(np.uint8).reshape(n, 4)
    return arena


def resolve_dev(torch, ctx, outgoing, arena_h, lens_h, stride):
    """One resolve launch over poisoned outputs -> (arena tensor, peer tensor, descs tensor)."""
    from quantum_amd import route

    n = len(lens_h)
    arena = torch.from_numpy(arena_h.reshape(-1).copy()).cuda()
    peer = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    descs = torch.full((16 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    (route.resolve_outgoing if outgoing else route.resolve_incoming)(ctx, arena, stride, n, u32_tensor(torch, lens_h),
                                                                     peer, descs)
    return arena, peer, descs


def expect_resolve(outgoing, t, net, mask, gateway, own, arena_h, lens_h, addrs, stride):
    """(arena, peers, descriptor lengths) by the header: outgoing reads Packet[16:20] of a packet of at least
    20 bytes whose datagram fits the slot, incoming Raw[0:4] of a datagram of 4 ... stride bytes."""
    want, peers = arena_h.copy(), []
    for i, (length, a) in enumerate(zip((int(x) for x in lens_h), addrs)):
        readable = length >= 20 and 4 + length + 28 <= stride if outgoing else 4 <= length <= stride
        p = rule_net(t, net, mask, gateway, a) if readable else None
        peers.append(NO_PEER if p is None else p)
        if outgoing and p is not None:
            want[i, 0:4] = np.frombuffer(own.to_bytes(4, "little"), np.uint8)
    dlen = [int(x) if outgoing else max(int(x) - 4, 0) for x in lens_h]
    return want, np.array(peers, np.uint32), np.array(dlen, np.uint32)


def resolve_and_check(torch, ctx, outgoing, t, net, mask, gateway, own, arena_h, lens_h, addrs, stride=STRIDE):
    arena, peer, descs = resolve_dev(torch, ctx, outgoing, arena_h, lens_h, stride)
    want, want_peer, want_len = expect_resolve(outgoing, t, net, mask, gateway, own, arena_h, lens_h, addrs, stride)
    got_peer = peer.cpu().numpy().view(np.uint32)
    d = np.frombuffer(descs.cpu().numpy().tobytes(), DESC)
    bad = np.flatnonzero(got_peer != want_peer)
    assert not len(bad), [(int(i), hex(addrs[i]), int(lens_h[i]), int(got_peer[i]), int(want_peer[i])) for i in bad[:8]]
    assert np.array_equal(d["off"], np.arange(len(lens_h), dtype=np.uint64) * stride)
    assert np.array_equal(d["len"], want_len)
    assert np.array_equal(d["key"], want_peer)
    # own_ip in the resolved outgoing slots' Raw[0:4]; every other byte, and every unresolved slot, unchanged
    assert np.array_equal(arena.cpu().numpy().reshape(arena_h.shape), want)
    return want_peer


def homes_in_net(cap):
    """home slot -> the in-net addresses 10.99.x.y of UNIVERSE's range that hash to it, for a table of `cap`."""
    homes = {}
    for j in range(2, 8194):
        ip = le(10, 99, j >> 8, j & 255)
        homes.setdefault(py_route_hash(ip) & (cap - 1), []).append(ip)
    return homes


def test_probe_wraps_past_the_last_slot(torch, ctx):
    """Eight routes sharing the highest reachable home slot of a 16-entry table: the cluster runs over the last
    slot into slots 0 ..., so hits, misses behind the cluster and misses that start after the seam all depend on
    `(h + 1) & cap_mask` and on builder and kernel agreeing there."""
    from quantum_amd import route

    count = 8
    cap = capacity(count)
    homes = homes_in_net(cap)
    home = max(h for h, v in homes.items() if len(v) >= count + 12)
    mapped, same_home = homes[home][:count], homes[home][count:count + 12]
    rng = random.Random(0x5EA4)
    t = {a: rng.randrange(ctx.max_keys) for a in mapped}
    slots, wrapped = build_table(list(t.items()))
    taken = [i for i, s in enumerate(slots) if s is not None]
    # the inputs do what they were picked for (a changed hash fails here, not silently)
    assert wrapped and cap == 16 and 0 in taken and cap - 1 in taken, (home, taken)
    assert sum(crosses_seam(probe_path(slots, a)) for a in mapped) >= 4
    assert len(same_home) >= 8 and all(crosses_seam(probe_path(slots, a)) for a in same_home)
    after_seam = [a for h in taken if h < home and h in homes for a in homes[h][:4] if a not in t]
    assert len(after_seam) >= 4
    for a in after_seam:  # starts on an occupied slot behind the seam, ends on the first empty one
        path = probe_path(slots, a)
        assert path[0] < home and slots[path[0]] is not None and slots[path[-1]] is None and len(path) >= 2
    probes = mapped + same_home + after_seam + [OUTSIDE[0]]
    n = 257
    addrs = [probes[i % len(probes)] for i in range(n)]
    lens = np.full(n, 64, np.uint32)
    route.routes_set(ctx, t, NET, MASK, GATEWAY, OWN)
    nrng = np.random.default_rng(0x5EA5)
    for outgoing in (True, False):
        peers = resolve_and_check(torch, ctx, outgoing, t, NET, MASK, GATEWAY, OWN,
                                  slots_with(nrng, n, STRIDE, addrs, outgoing), lens, addrs)
        assert (peers != NO_PEER).sum() == sum(a in t for a in addrs) >= 8 * (n // len(probes))


def test_small_tables_of_random_addresses(torch, ctx):
    """Mask 0 puts every address in the net, so all 32 bits reach the hash: no residue pattern of one subnet
    decides which slots are used.  64 tables of 1 ... 8 routes (route_model.sweep_case), each probed by one
    256-packet batch, half mapped addresses and half random misses, outgoing and incoming."""
    from quantum_amd import route

    # 33 of the 64 tables step from the last slot to slot 0 in an insertion or in a lookup of their batch (7
    # already in an insertion), counted with route_model's copy of the layout: test_route_model.py pins the number
    assert sum(sweep_wraps(k) for k in range(SWEEP_TABLES)) >= 8
    nrng = np.random.default_rng(0x5EEA)
    for k in range(SWEEP_TABLES):
        t, addrs, gateway = sweep_case(k)
        route.routes_set(ctx, t, 0, 0, gateway, OWN)
        for outgoing in (True, False):
            lens = np.full(256, 32 if outgoing else 64, np.uint32)  # both fill a 64-byte slot
            peers = resolve_and_check(torch, ctx, outgoing, t, 0, 0, gateway, OWN,
                                      slots_with(nrng, 256, 64, addrs, outgoing), lens, addrs, stride=64)
            assert (peers != NO_PEER).sum() == 128, k


A5, A6, A7 = le(10, 99, 0, 5), le(10, 99, 0, 6), le(10, 99, 0, 7)
FAR = le(8, 8, 8, 8)
ALL1 = 0xFFFFFFFF
SHAPES = {
    # id: (table, net, mask, gateway, addresses every batch must hold)
    "mask0": ({FAR: 1, A5: 2, le(192, 168, 1, 1): 3, ALL1: 4, le(1, 1, 1, 1): 5}, NET, 0, le(1, 1, 1, 1),
              [FAR, A5, le(192, 168, 1, 1), ALL1, le(1, 1, 1, 1), le(9, 9, 9, 9), A6, 0]),
    "mask32": ({A5: 1, A6: 2, GATEWAY: 3}, A5, ALL1, GATEWAY, [A5, A6, A7, GATEWAY, FAR, 0, A5 ^ 1, A5 ^ (1 << 31)]),
    "mask32_gateway_unmapped": ({A5: 1, A6: 2}, A5, ALL1, GATEWAY, [A5, A6, A7, GATEWAY, FAR, 0]),
    "net_with_host_bits": ({A5: 1, le(10, 99, 3, 7): 2, le(10, 99, 200, 1): 3, GATEWAY: 4, le(10, 98, 3, 7): 5},
                           le(10, 99, 3, 7), MASK, GATEWAY,
                           [A5, le(10, 99, 3, 7), le(10, 99, 200, 1), A6, le(10, 98, 3, 7), le(11, 99, 3, 7), FAR, 0]),
    "gateway_outside_mapped": ({A5: 1, A6: 2, FAR: 6}, NET, MASK, FAR, [A5, A6, A7, FAR, le(10, 98, 0, 5), 0, ALL1]),
    "gateway_is_a_mapped_peer": ({A5: 1, A6: 2}, NET, MASK, A5, [A5, A6, A7, FAR, le(10, 98, 0, 5), 0]),
    "zero_mapped_mask0": ({0: 7, A5: 1}, NET, 0, GATEWAY, [0, A5, A6, 1, 1 << 24, FAR]),
    "zero_in_empty_table": ({}, NET, 0, GATEWAY, [0, A5, FAR]),
    "zero_unmapped_mask0": ({A5: 1, A6: 2}, NET, 0, GATEWAY, [0, A5, A6, A7]),
    "zero_unmapped_slash16": ({A5: 1, A6: 2, GATEWAY: 9}, NET, MASK, GATEWAY, [0, A5, A6, A7]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_net_mask_gateway_shapes(torch, ctx, shape):
    from quantum_amd import route

    t, net, mask, gateway, must = SHAPES[shape]
    rng = random.Random(0x54A9 + len(shape))
    n = 130
    addrs = [must[i % len(must)] if i < 100 else rng.getrandbits(32) if i % 2 else le(10, 99, 0, rng.randrange(256))
             for i in range(n)]
    route.routes_set(ctx, t, net, mask, gateway, OWN)
    nrng = np.random.default_rng(0x54AA)
    lens = np.array([(40, 64, 1350)[i % 3] for i in range(n)], np.uint32)
    for outgoing in (True, False):
        resolve_and_check(torch, ctx, outgoing, t, net, mask, gateway, OWN, slots_with(nrng, n, STRIDE, addrs, outgoing),
                          lens, addrs)


def test_duplicate_ip_takes_its_last_entry(torch, ctx):
    """qgcm_routes_set of pairs in which three addresses come twice: the later peer wins (a map assignment), also
    when entries with the same home slot were inserted between the two, and no other lookup changes."""
    from quantum_amd import route

    cap = capacity(11)  # the eleven pairs below
    homes = homes_in_net(cap)
    cluster = max(homes.values(), key=len)
    s0, s1, s2, s3 = cluster[:4]
    others = [a for h, v in sorted(homes.items()) if v is not cluster for a in v[:1]][:5]
    y, z, u1, u2, u3 = others
    pairs = [(z, 7), (s0, 1), (s1, 2), (s2, 3), (s0, 4), (y, 5), (y, 6), (u1, 10), (u2, 11), (u3, 12), (z, 8)]
    assert capacity(len(pairs)) == cap and len({py_route_hash(a) & (cap - 1) for a in (s0, s1, s2, s3)}) == 1
    t = dict(pairs)
    assert len(t) == 8 and (t[s0], t[y], t[z]) == (4, 6, 8)
    slots, _ = build_table(pairs)
    assert len(probe_path(slots, s2)) >= 3  # s0's entry stayed first of its cluster: s1 and s2 probe past it
    probes = [s0, s1, s2, s3, y, z, u1, u2, u3] + cluster[4:8] + [OUTSIDE[1]]
    n = 130
    addrs = [probes[i % len(probes)] for i in range(n)]
    lens = np.full(n, 64, np.uint32)
    nrng = np.random.default_rng(0xD0B1)
    route.routes_set(ctx, pairs, NET, MASK, GATEWAY, OWN)
    for outgoing in (True, False):
        resolve_and_check(torch, ctx, outgoing, t, NET, MASK, GATEWAY, OWN, slots_with(nrng, n, STRIDE, addrs, outgoing),
                          lens, addrs)


@pytest.mark.parametrize("stride", [1472, 64])
def test_length_edges(torch, ctx, stride):
    """Every packet carries a mapped address: the length alone decides.  Outgoing 0xFFFFFFE0 makes 4 + len + 28
    zero in 32 bits; at stride 64 the accepted outgoing lengths are exactly 20 ... 32."""
    from quantum_amd import route

    t = {A5: 1, A6: 2, A7: 2047, le(10, 99, 77, 1): 0}
    route.routes_set(ctx, t, NET, MASK, GATEWAY, OWN)
    edges = {True: [0, 19, 20, 32, 33, stride - 32, stride - 31, 0xFFFFFFE0, 0xFFFFFFE3, 0xFFFFFFFF],
             False: [0, 3, 4, stride - 1, stride, stride + 1, 0xFFFFFFFF]}
    nrng = np.random.default_rng(0x1E9 + stride)
    keys = list(t)
    for outgoing in (True, False):
        n = 13 * len(edges[outgoing])
        lens = np.array([edges[outgoing][i % len(edges[outgoing])] for i in range(n)], np.uint32)
        addrs = [keys[(i // 3) % 4] for i in range(n)]
        peers = resolve_and_check(torch, ctx, outgoing, t, NET, MASK, GATEWAY, OWN,
                                  slots_with(nrng, n, stride, addrs, outgoing), lens, addrs, stride=stride)
        accepted = sorted({int(x) for x in lens[peers != NO_PEER]})
        assert accepted == {(1472, True): [20, 32, 33, 1440], (64, True): [20, 32],
                            (1472, False): [4, 1471, 1472], (64, False): [4, 63, 64]}[stride, outgoing]


# ---- accounting ----

def read_block(ctx, direction, links=None):
    """The counter block of one direction: (totals (4,), links (max_keys, 4)), uint64 -- every link, or the
    given ones with the other rows left zero."""
    from quantum_amd import route

    block = np.zeros((ctx.max_keys, 4), np.uint64)
    for k in range(ctx.max_keys) if links is None else links:
        block[k] = list(route.route_stats(ctx, direction, int(k)).values())
    return np.array(list(route.route_stats(ctx, direction).values()), np.uint64), block


def watched(peer, max_keys, seed):
    """The links a quick check reads: those the batch names, their +-256 neighbours (the LDS entry's other
    tenants), and 16 random others."""
    named = {int(p) for p in np.unique(peer) if p < max_keys}
    near = {p + d for p in named for d in (-256, 256) if 0 <= p + d < max_keys}
    return sorted(named | near | {int(k) for k in np.random.default_rng(seed).integers(0, max_keys, 16)})


def account(torch, ctx, direction, peer, lens, status):
    from quantum_amd import route

    n = len(peer)
    d = np.zeros(n, DESC)
    d["off"], d["len"], d["key"] = np.arange(n, dtype=np.uint64) * STRIDE, lens, peer
    route.route_account(ctx, direction, n, u32_tensor(torch, peer), torch.from_numpy(d.view(np.uint8).copy()).cuda(),
                        None if status is None else torch.from_numpy(np.ascontiguousarray(status, np.uint8)).cuda())
    torch.cuda.synchronize()


def account_and_check(torch, ctx, direction, peer, lens, status, before=None, links=None):
    """One accounting launch; the deltas of the totals and of all links (or of `links`, which must hold every
    link the batch names) equal route_sums -- a sum that lands on a wrong link shows on both.  Returns (the
    block read after, the expected sums)."""
    if before is None:
        before = read_block(ctx, direction, links)
    account(torch, ctx, direction, peer, lens, status)
    after = read_block(ctx, direction, links)
    want_tot, want_links = route_sums(direction, peer, lens, status, ctx.max_keys)
    if links is not None:
        assert not np.delete(want_links, links, axis=0).any()
    got_tot, got_links = after[0] - before[0], after[1] - before[1]
    assert got_tot.tolist() == want_tot.tolist(), ("totals", got_tot.tolist(), want_tot.tolist())
    bad = np.flatnonzero((got_links != want_links).any(axis=1))
    assert not len(bad), [(int(k), got_links[k].tolist(), want_links[k].tolist()) for k in bad[:8]]
    return after, (want_tot, want_links)


def all_four_ways(torch, ctx, peer, lens, status):
    """Tx and Rx, with the status array and with NULL; the other direction's block never moves."""
    out = {}
    for direction in (TX, RX):
        other = read_block(ctx, 1 - direction)
        after, out[direction, True] = account_and_check(torch, ctx, direction, peer, lens, status)
        _, out[direction, False] = account_and_check(torch, ctx, direction, peer, lens, None, before=after)
        now = read_block(ctx, 1 - direction)
        assert np.array_equal(now[0], other[0]) and np.array_equal(now[1], other[1])
    return out


def lds_mates(p):
    """Eight links of one LDS entry of the accounting kernel (entry = peer & 255)."""
    return [p + 256 * j for j in range(8)]


BIG_DROPPED, BIG_DROPPED_FEW, BIG_SENT, BIG_SENT_FEW = 1234, 1235, 900, 901


def named_waves(direction, seed):
    """[(name, peer[64], lens[64], status[64])]: each wave holds what its name says; the first four are one
    256-packet tile."""
    rng = np.random.default_rng(seed)
    waves = []

    def wave(name, peer, lens=None, status=None, shuffle=False):
        peer = np.array(peer, np.uint32)
        assert len(peer) == 64, name
        lens = rng.integers(0, 1401, 64).astype(np.uint32) if lens is None else np.array(lens, np.uint32)
        status = (rng.random(64) >= 0.1).astype(np.uint8) if status is None else np.array(status, np.uint8)
        if shuffle:
            order = rng.permutation(64)
            peer, lens, status = peer[order], lens[order], status[order]
        waves.append((name, peer, lens, status))

    m1, m2 = lds_mates(37), lds_mates(200)
    for j in range(4):  # eight links per LDS entry, two entries, spread over the four waves of one tile
        wave(f"lds mates over a tile {j}", np.repeat([m1[2 * j], m1[2 * j + 1], m2[2 * j], m2[2 * j + 1]], 16), shuffle=True)
    wave("lds mates in one wave", np.repeat(m1[::-1] + m2, 4), shuffle=True)
    wave("64 distinct links", 300 + rng.permutation(64))
    wave("singletons and LDS mates interleaved", [lds_mates(5)[i % 8] if i % 2 else 1000 + i for i in range(64)])
    wave("one link", [777] * 64)
    wave("two links alternating", [5, 6] * 32)
    wave("two LDS mates alternating", [9, 9 + 1024] * 32)
    wave("two singletons then three groups", [1500, 1501] + list(rng.permutation(np.repeat([40, 41, 42], [21, 21, 20]))))
    wave("leader dropped, group delivered", [1600] * 64, status=[0] + [1] * 63)
    wave("leader delivered, group dropped", [1601] * 64, status=[1] + [0] * 63)
    wave("both of those in one wave", [1602] * 30 + [1603] * 34, status=[0] + [1] * 29 + [1] + [0] * 33)
    wave("unresolved lanes lead", [NO_PEER] * 10 + [50, 51] * 27)
    wave("peers at or above max_keys", [2048, 0x7FFFFFFF, 0xFFFFFFFE, 60, 2047, NO_PEER, 61, 2048] * 8)
    big = [0xFFFFFFFF, 0xFFFFFFF0] if direction == TX else [0xFFFFFFFF]
    for name, many, few, st in (("lengths near 2^32, dropped", BIG_DROPPED, BIG_DROPPED_FEW, 0),
                                ("lengths near 2^32, delivered", BIG_SENT, BIG_SENT_FEW, 1)):
        wave(name, [many] * 40 + [few] * 3 + [70] * 21,
             lens=[big[i % len(big)] for i in range(43)] + list(rng.integers(0, 1401, 21)),
             status=[st] * 40 + [1 - st] * 3 + [1] * 21, shuffle=True)
    six = [(0, 1), (27, 1), (28, 1), (0, 0), (27, 0), (28, 0)]
    wave("lengths around 28", [80 + (i // 6) % 2 for i in range(64)], lens=[six[i % 6][0] for i in range(64)],
         status=[six[i % 6][1] for i in range(64)])
    return waves


def test_named_waves(torch, ctx):
    from quantum_amd import route

    route.routes_set(ctx, {}, NET, MASK, GATEWAY, OWN)
    for direction in (TX, RX):
        waves = named_waves(direction, 0xACE5 + direction)
        assert [w[0] for w in waves[:4]] == [f"lds mates over a tile {j}" for j in range(4)]
        rng = np.random.default_rng(0xACE7)
        tail = 37  # the ragged end: n = 64 k + 37
        peer = np.concatenate([w[1] for w in waves] + [np.where(rng.random(tail) < 0.7, 64, 3).astype(np.uint32)])
        lens = np.concatenate([w[2] for w in waves] + [rng.integers(0, 1401, tail).astype(np.uint32)])
        status = np.concatenate([w[3] for w in waves] + [(rng.random(tail) >= 0.1).astype(np.uint8)])
        assert len(peer) == 64 * len(waves) + 37
        # the waves one at a time first, over the links near them: a failure names its wave
        for k, (name, p, ln, st) in enumerate(waves):
            try:
                account_and_check(torch, ctx, direction, p, ln, st, links=watched(p, ctx.max_keys, k))
            except AssertionError as e:
                raise AssertionError(f"wave '{name}', direction {direction}: {e}") from None
        # the whole batch, with the status array and with NULL, over every link
        after, (_, links) = account_and_check(torch, ctx, direction, peer, lens, status)
        _, (_, links_null) = account_and_check(torch, ctx, direction, peer, lens, None, before=after)
        # the sums the batch was built to reach: past 2^37 on one link, exact above
        assert int(links[BIG_DROPPED][3]) > 1 << 37 and int(links[BIG_SENT][1]) > 1 << 37
        assert int(links_null[BIG_DROPPED][1]) > 1 << 37 and int(links_null[BIG_DROPPED][3]) == 0
        assert int(links[BIG_DROPPED_FEW][1]) > 1 << 32 and int(links[BIG_SENT_FEW][3]) > 1 << 32


def test_named_waves_leave_the_other_direction_alone(torch, ctx):
    from quantum_amd import route

    route.routes_set(ctx, {}, NET, MASK, GATEWAY, OWN)
    waves = named_waves(TX, 0xACE9)
    all_four_ways(torch, ctx, *(np.concatenate([w[k] for w in waves]) for k in (1, 2, 3)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_small_batches_on_two_links(torch, ctx, n):
    from quantum_amd import route

    route.routes_set(ctx, {}, NET, MASK, GATEWAY, OWN)
    rng = np.random.default_rng(0x2117 + n)
    peer = np.where(rng.random(n) < 0.6, 11, 1500).astype(np.uint32)
    peer[rng.random(n) < 0.05] = NO_PEER
    lens = rng.integers(0, 1401, n).astype(np.uint32)
    all_four_ways(torch, ctx, peer, lens, (rng.random(n) >= 0.2).astype(np.uint8))


def test_workgroups_walk_several_tiles(torch, ctx):
    """More tiles than the grid's cap of 8 workgroups per CU: half the workgroups walk two tiles, carry their
    LDS table from the first into the second and flush once; the last tile is partial."""
    from quantum_amd import route

    route.routes_set(ctx, {}, NET, MASK, GATEWAY, OWN)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = 8 * cus
    n = 256 * (cap + cap // 2) + 77
    hot = 64
    mates = [hot + 256, hot + 512, hot + 768, 10, 10 + 256, 10 + 1024, 99, 99 + 512]  # of the hot link, of each other
    rng = np.random.default_rng(0x711E5)
    rest = [int(k) for k in rng.permutation(2048) if int(k) not in mates and int(k) != hot][:32]
    links = np.array(mates + rest, np.uint32)
    assert len(set(links.tolist())) == 40
    for direction in (TX, RX):
        peer = np.where(rng.random(n) < 0.85, hot, links[rng.integers(0, 40, n)]).astype(np.uint32)
        unresolved = rng.random(n) < 0.03
        peer[unresolved] = np.where(rng.random(int(unresolved.sum())) < 0.8, NO_PEER, 2048)
        lens = rng.integers(0, 1401, n).astype(np.uint32)
        status = (rng.random(n) >= 0.1).astype(np.uint8)
        _, (tot, want_links) = account_and_check(torch, ctx, direction, peer, lens, status)
        assert int(tot[0]) > n // 2 and int(want_links[hot][0]) > n // 2 and all(int(want_links[k][0]) for k in links)


# ---- host pipelines ----

SEAM = 65536        # packets per chunk of the routed host pipelines
SMALL = 64          # the smallest stride a 20-byte packet fits: 4 + 20 + 28 = 52


def small_batch(seed, n, unroutable_every=None):
    """n slots of stride 64 with packets of 20 ... 32 bytes for the five PEERS; with `unroutable_every`, the
    packets at i % 11 == 7 go to in-net addresses no table maps (65534 and 65545 lie on either side of the seam)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 33, n).astype(np.uint32)
    dst = np.array(PEERS, np.uint32)[rng.integers(0, 5, n)]
    if unroutable_every:
        idx = np.flatnonzero(np.arange(n) % unroutable_every == 7)
        dst[idx] = np.array(UNIVERSE[4096:], np.uint32)[idx % 4096]
    arena = slots_with(rng, n, SMALL, dst.tolist(), True)
    nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    return arena, lens, dst, nonces


def payload_mask(lens, stride):
    col = np.arange(stride)[None, :]
    return (col >= 4) & (col < 4 + lens.astype(np.int64)[:, None])


def test_host_pipelines_take_a_second_chunk(torch, nodes):
    from quantum_amd import batch, route

    tx, rx, keys = nodes
    n = SEAM + 300
    t = {a: k for k, a in enumerate(PEERS)}
    arena_h, lens_h, dst, nonces_h = small_batch(0x5EA3, n, unroutable_every=11)
    route.routes_set(tx, t, NET, MASK, UNMAPPED_GW, OWN)
    want_peer = np.array([t.get(int(a), NO_PEER) for a in dst], np.uint32)  # every dst is in the net
    assert want_peer[SEAM - 2] == NO_PEER and want_peer[SEAM + 9] == NO_PEER
    want_st = (want_peer != NO_PEER).astype(np.uint8)
    # the device path on the same input (test_wire_parity pins it to the oracle)
    arena, peer, descs = resolve_dev(torch, tx, True, arena_h, lens_h, SMALL)
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    batch.seal_batch(tx, arena, descs, n, torch.from_numpy(nonces_h).cuda(), status=status)
    want_arena = arena.cpu().numpy().reshape(n, SMALL)
    assert np.array_equal(peer.cpu().numpy().view(np.uint32), want_peer) and np.array_equal(status.cpu().numpy(), want_st)
    # ... and the oracle itself around the seam and at the end
    own = np.frombuffer(OWN.to_bytes(4, "little"), np.uint8)
    for i in list(range(SEAM - 36, SEAM + 65)) + list(range(n - 64, n)):
        ref, length = arena_h[i].copy(), int(lens_h[i])
        if want_peer[i] != NO_PEER:
            ref[0:4] = own
            buf = bytearray(ref[4:4 + length + 28].tobytes())
            O.aesgo_encrypt(keys[want_peer[i]], buf, length, own.tobytes(), nonces_h[12 * i:12 * i + 12].tobytes())
            ref[4:4 + length + 28] = np.frombuffer(bytes(buf), np.uint8)
        assert np.array_equal(want_arena[i], ref), i
    before = read_block(tx, TX)
    work = arena_h.copy()  # pageable
    h_lens, h_peer, h_st = lens_h.copy(), np.zeros(n, np.uint32), np.full(n, 7, np.uint8)
    dropped = route.route_seal_host(tx, work.ctypes.data, SMALL, n, h_lens, nonces_h.ctypes.data, h_peer, h_st)
    assert dropped == int((want_st == 0).sum()) > 5000
    bad = np.flatnonzero((work != want_arena).any(axis=1))
    assert not len(bad), bad[:8]
    assert np.array_equal(h_peer, want_peer) and np.array_equal(h_st, want_st)
    assert np.array_equal(h_lens, np.where(want_st == 1, lens_h + 32, 0))
    after = read_block(tx, TX)
    tot, links = route_sums(TX, want_peer, lens_h, want_st, tx.max_keys)
    assert (after[0] - before[0]).tolist() == tot.tolist()
    assert np.array_equal(after[1] - before[1], links) and all(int(links[k][0]) > 10000 for k in range(5))
    # the peer behind key slot 2 opens the arena back: its own packets open, the other peers' fail their tag,
    # one of its datagrams is tampered with in each chunk
    route.routes_set(rx, {OWN: 3}, NET, MASK, UNMAPPED_GW, PEERS[2])
    mine = np.flatnonzero(want_peer == 2)
    tampered = [int(mine[mine < SEAM][-3]), int(mine[mine >= SEAM][2])]
    for i in tampered:
        work[i, 4 + 5] ^= 0x40
    sealed = work.copy()
    exp_peer = np.where(want_st == 1, 3, NO_PEER).astype(np.uint32)  # dropped slots arrive with length 0: no sender
    exp_st = (want_peer == 2).astype(np.uint8)
    exp_st[tampered] = 0
    rbefore = read_block(rx, RX)
    r_lens, r_peer, r_st = h_lens.copy(), np.zeros(n, np.uint32), np.full(n, 7, np.uint8)
    rdropped = route.route_open_host(rx, work.ctypes.data, SMALL, n, r_lens, r_peer, r_st)
    assert rdropped == n - int(exp_st.sum())
    assert np.array_equal(r_peer, exp_peer) and np.array_equal(r_st, exp_st)
    assert np.array_equal(r_lens, np.where(exp_st == 1, lens_h, 0))
    pay = payload_mask(lens_h, SMALL)
    opened, failed = exp_st == 1, (exp_peer == 3) & (exp_st == 0)
    assert np.array_equal(work[opened][pay[opened]], arena_h[opened][pay[opened]])  # the plaintext is back
    assert not work[failed][pay[failed]].any()                                      # errOpen: plaintext region zeroed
    assert np.array_equal(work[:, :4], sealed[:, :4])
    assert np.array_equal(work[exp_peer == NO_PEER], sealed[exp_peer == NO_PEER])   # never sealed: byte for byte
    rafter = read_block(rx, RX)
    rtot, rlinks = route_sums(RX, exp_peer, np.where(want_st == 1, lens_h + 28, 0), exp_st, rx.max_keys)
    assert (rafter[0] - rbefore[0]).tolist() == rtot.tolist()
    assert np.array_equal(rafter[1] - rbefore[1], rlinks) and int(rlinks[3][0]) > 10000 and int(rlinks[3][2]) > 40000


def test_route_seal_host_nonce_in_the_slot(torch, nodes):
    """h_nonces NULL: "the nonce is in the slot" -- at [4 + L + 16, 4 + L + 28), where qgcm_seal_batch's
    description in include/qgcm.h puts it ("the same three forms in every batch seal"; qgcm_seal_host's own
    paragraph does not repeat the place).  Equal, byte for byte, to the call that is handed the same nonces."""
    from quantum_amd import route

    tx, _, keys = nodes
    rng = random.Random(0x1575)
    n = 300
    t = {a: k for k, a in enumerate(PEERS)}
    arena_h, lens_h, dsts, nonces_h = wire_batch(
        n, rng, lambda i: rng.choice(UNIVERSE[4096:]) if i % 11 == 7 else PEERS[rng.randrange(5)])
    for i, length in enumerate(int(x) for x in lens_h):
        o = i * STRIDE + 4 + length + 16
        arena_h[o:o + 12] = nonces_h[12 * i:12 * i + 12]
    route.routes_set(tx, t, NET, MASK, UNMAPPED_GW, OWN)
    ref, ref_peers = oracle_seal(keys, t, arena_h, lens_h, dsts, nonces_h)
    got = {}
    for form, nonces in (("explicit", nonces_h.ctypes.data), ("in the slot", None)):
        work = arena_h.copy()
        h_lens, h_peer, h_st = lens_h.copy(), np.zeros(n, np.uint32), np.full(n, 7, np.uint8)
        dropped = route.route_seal_host(tx, work.ctypes.data, STRIDE, n, h_lens, nonces, h_peer, h_st)
        got[form] = (work, h_lens, h_peer, h_st, dropped)
        assert dropped == int((ref_peers == NO_PEER).sum()) >= 20, form
        assert np.array_equal(h_peer, ref_peers), form
        assert np.array_equal(work, ref), form
    for a, b in zip(got["explicit"][:4], got["in the slot"][:4]):
        assert np.array_equal(a, b)


def test_generated_nonces_across_the_seam(torch, nodes):
    from quantum_amd import batch, route

    tx, rx, _ = nodes
    n = SEAM + 300
    arena_h, lens_h, _, _ = small_batch(0x6E6E, n)
    route.routes_set(tx, {a: 2 for a in PEERS}, NET, MASK, UNMAPPED_GW, OWN)
    route.routes_set(rx, {OWN: 3}, NET, MASK, UNMAPPED_GW, PEERS[2])
    work = arena_h.copy()
    h_lens, h_peer = lens_h.copy(), np.zeros(n, np.uint32)
    assert route.route_seal_host(tx, work.ctypes.data, SMALL, n, h_lens, batch.GENERATE, h_peer) == 0
    assert np.array_equal(h_lens, lens_h + 32) and (h_peer == 2).all()
    at = (4 + lens_h.astype(np.int64) + 16)[:, None] + np.arange(12)[None, :]
    nonces = np.take_along_axis(work, at, axis=1)
    assert len(np.unique(nonces, axis=0)) == n  # one fresh nonce per packet, on both sides of the seam
    assert route.route_open_host(rx, work.ctypes.data, SMALL, n, h_lens, h_peer) == 0
    assert np.array_equal(h_lens, lens_h) and (h_peer == 3).all()
    pay = payload_mask(lens_h, SMALL)
    assert np.array_equal(work[pay], arena_h[pay])
