"""Routes and link metrics on the GPU (include/qgcm.h "routes resolved on the GPU").

Every expectation is computed here from a plain Python dict plus the net / gateway rule of
router/router.go:21-31 and the counter table of the header, never by the code under test; sealed bytes come
from the oracle as in the parity tests.  Addresses are common.IPtoInt values (little-endian uint32 of the
four bytes).
"""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

NO_PEER = 0xFFFFFFFF
STRIDE = 1472
DESC = np.dtype([("off", "<u8"), ("len", "<u4"), ("key", "<u4")])


def le(a, b, c, d):
    return a | b << 8 | c << 16 | d << 24


NET, MASK = le(10, 99, 0, 0), le(255, 255, 0, 0)
OWN = le(10, 99, 0, 1)
GATEWAY = le(10, 99, 255, 254)   # never one of UNIVERSE's addresses
OUTSIDE = [le(8, 8, 8, 8), le(11, 99, 0, 5), le(10, 98, 0, 5), le(0, 0, 0, 0)]
# 8192 in-net addresses in a fixed shuffled order: a table of `count` routes maps the first `count`, the
# rest are the in-net misses (they differ from mapped ones in any byte, the last one included)
UNIVERSE = [le(10, 99, j >> 8, j & 255) for j in range(2, 8194)]
random.Random(0x10C).shuffle(UNIVERSE)


@pytest.fixture(scope="module")
def torch():
    import torch as T

    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def table(count, gateway_mapped, max_keys, seed=0):
    """dict address -> key slot of `count` routes; a mapped gateway is one of them."""
    rng = random.Random(0x7AB1E + count + seed)
    t = {}
    if gateway_mapped and count:
        t[GATEWAY] = rng.randrange(max_keys)
    for a in UNIVERSE[:count - len(t)]:
        t[a] = rng.randrange(max_keys)
    assert len(t) == count
    return t


def rule(t, addr):
    """router.go:21-31 over the dict; None = no mapping."""
    return t.get(addr if (addr & MASK) == (NET & MASK) else GATEWAY)


def descs_of(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), DESC)


def outgoing_batch(n, count, rng):
    """n TUN packets of every class: mapped, in-net unmapped, out of net, and the four length edges."""
    mapped = UNIVERSE[:max(count - 1, 1)]  # mapped by both tables of `count` routes (one may hold the gateway)
    lens, dsts = [], []
    for i in range(n):
        c = i % 8
        dst = rng.choice(mapped)
        L = rng.randint(20, STRIDE - 32)
        if c == 1:
            dst = rng.choice(UNIVERSE[4096:])      # in the net, in no table
        elif c == 2:
            dst = rng.choice(OUTSIDE)              # out of the net: the gateway's mapping, if any
        elif c == 3:
            L = 19                                 # Packet[16:20] does not exist
        elif c == 4:
            L = 20
        elif c == 5:
            L = STRIDE - 31                        # 4 + L + 28 > stride
        elif c == 6:
            L = STRIDE - 32                        # fits exactly
        lens.append(L)
        dsts.append(dst)
    arena = np.frombuffer(rng.randbytes(n * STRIDE), np.uint8).copy()
    for i, d in enumerate(dsts):
        arena[i * STRIDE + 20:i * STRIDE + 24] = np.frombuffer(d.to_bytes(4, "little"), np.uint8)
    return arena, np.array(lens, np.uint32), dsts


def expect_outgoing(t, arena, lens, dsts):
    want, peers = arena.copy(), []
    for i, (L, d) in enumerate(zip(lens, dsts)):
        p = rule(t, d) if L >= 20 and 4 + int(L) + 28 <= STRIDE else None
        peers.append(NO_PEER if p is None else p)
        if p is not None:
            want[i * STRIDE:i * STRIDE + 4] = np.frombuffer(OWN.to_bytes(4, "little"), np.uint8)
    return want, np.array(peers, np.uint32)


def run_resolve(torch, ctx, outgoing, arena_h, lens_h, stream=None):
    from quantum_amd import route

    n = len(lens_h)
    arena = torch.from_numpy(arena_h.copy()).cuda()
    lens = torch.from_numpy(lens_h.astype(np.int64)).to(torch.int32).cuda()
    peer = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    descs = torch.full((16 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    (route.resolve_outgoing if outgoing else route.resolve_incoming)(ctx, arena, STRIDE, n, lens, peer, descs, stream)
    return arena, lens, peer, descs


def check_resolved(n, peer, descs, want_peer, want_len):
    got_peer = peer.cpu().numpy().view(np.uint32)
    d = descs_of(descs)
    assert np.array_equal(got_peer, want_peer)
    assert np.array_equal(d["off"], np.arange(n, dtype=np.uint64) * STRIDE)
    assert np.array_equal(d["len"], want_len)
    assert np.array_equal(d["key"], want_peer)


@pytest.mark.parametrize("count", [0, 1, 300, 4096])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_resolve_outgoing(torch, ctx, n, count):
    from quantum_amd import route

    rng = random.Random(1000 * n + count)
    arena_h, lens_h, dsts = outgoing_batch(n, count, rng)
    for gateway_mapped in (True, False):
        t = table(count, gateway_mapped, ctx.max_keys)
        route.routes_set(ctx, t, NET, MASK, GATEWAY, OWN)
        arena, _, peer, descs = run_resolve(torch, ctx, True, arena_h, lens_h)
        want, want_peer = expect_outgoing(t, arena_h, lens_h, dsts)
        check_resolved(n, peer, descs, want_peer, lens_h)
        # own_ip in the resolved slots' Raw[0:4], nothing else touched: unresolved slots whole
        assert np.array_equal(arena.cpu().numpy(), want)
        if n >= 63 and count >= 300:
            res = want_peer != NO_PEER
            cls = np.arange(n) % 8
            assert res[cls == 0].all() and res[cls == 7].all() and not res[cls == 1].any()
            assert res[cls == 2].all() if gateway_mapped else not res[cls == 2].any()
            assert not res[cls == 3].any() and res[cls == 4].all() and not res[cls == 5].any() and res[cls == 6].all()


@pytest.mark.parametrize("count", [0, 1, 300, 4096])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_resolve_incoming(torch, ctx, n, count):
    from quantum_amd import route

    rng = random.Random(7000 * n + count)
    lens_h = np.array([(3, 4, 31, 32, 1382)[i % 5] for i in range(n)], np.uint32)
    mapped = UNIVERSE[:max(count - 1, 1)]  # mapped by both tables of `count` routes (one may hold the gateway)
    srcs = [rng.choice(mapped) if i % 3 == 0 else rng.choice(UNIVERSE[4096:]) if i % 3 == 1 else rng.choice(OUTSIDE)
            for i in range(n)]
    arena_h = np.frombuffer(rng.randbytes(n * STRIDE), np.uint8).copy()
    for i, s in enumerate(srcs):
        arena_h[i * STRIDE:i * STRIDE + 4] = np.frombuffer(s.to_bytes(4, "little"), np.uint8)
    for gateway_mapped in (True, False):
        t = table(count, gateway_mapped, ctx.max_keys)
        route.routes_set(ctx, t, NET, MASK, GATEWAY, OWN)
        arena, _, peer, descs = run_resolve(torch, ctx, False, arena_h, lens_h)
        want_peer = np.array([NO_PEER if L < 4 or rule(t, s) is None else rule(t, s) for L, s in zip(lens_h, srcs)],
                             np.uint32)
        want_len = np.where(lens_h >= 4, lens_h - 4, 0).astype(np.uint32)  # Raw[:n] without its header; 3 -> 0
        check_resolved(n, peer, descs, want_peer, want_len)
        assert np.array_equal(arena.cpu().numpy(), arena_h)  # read only
        if n >= 63 and count >= 300 and gateway_mapped:
            assert (want_peer != NO_PEER).any() and (want_peer == NO_PEER).any()


def test_table_replace_is_whole(torch, ctx):
    """resolve, qgcm_routes_set of a table mapping the same addresses to other peers, resolve: the first result
    is wholly the old table's, the second wholly the new one's."""
    from quantum_amd import route

    rng = random.Random(0xAB)
    n = 1000
    a = table(300, True, ctx.max_keys)
    b = {k: (v + 1 + rng.randrange(ctx.max_keys - 1)) % ctx.max_keys for k, v in a.items()}  # every peer differs
    arena_h, lens_h, dsts = outgoing_batch(n, 300, rng)
    s = torch.cuda.Stream()
    route.routes_set(ctx, a, NET, MASK, GATEWAY, OWN)
    _, _, peer_a, descs_a = run_resolve(torch, ctx, True, arena_h, lens_h, s)
    route.routes_set(ctx, b, NET, MASK, GATEWAY, OWN)
    _, _, peer_b, descs_b = run_resolve(torch, ctx, True, arena_h, lens_h, s)
    s.synchronize()
    check_resolved(n, peer_a, descs_a, expect_outgoing(a, arena_h, lens_h, dsts)[1], lens_h)
    check_resolved(n, peer_b, descs_b, expect_outgoing(b, arena_h, lens_h, dsts)[1], lens_h)


# ---- two nodes: `tx` seals for five peers, `rx` is the peer behind key slot 2 of tx (its slot 3) ----

PEERS = [le(10, 99, 1, k) for k in (10, 11, 12, 13, 14)]
UNMAPPED_GW = GATEWAY  # the nodes' tables never map it: out-of-net traffic has no route


@pytest.fixture(scope="module")
def nodes(torch):
    from quantum_amd.crypto import Context

    rng = random.Random(0x20DE5)
    keys = [rng.randbytes(32) for _ in range(5)]
    tx, rx = Context(device=0, max_keys=8), Context(device=0, max_keys=8)
    tx.set_keys(0, b"".join(keys))
    rx.set_key(3, keys[2])
    yield tx, rx, keys
    tx.close()
    rx.close()


def wire_batch(n, rng, dst_of):
    lens = np.array([rng.choice([20, 64, 1350]) for _ in range(n)], np.uint32)
    dsts = [dst_of(i) for i in range(n)]
    arena = np.frombuffer(rng.randbytes(n * STRIDE), np.uint8).copy()
    for i, d in enumerate(dsts):
        arena[i * STRIDE + 20:i * STRIDE + 24] = np.frombuffer(d.to_bytes(4, "little"), np.uint8)
    nonces = np.frombuffer(rng.randbytes(12 * n), np.uint8).copy()
    return arena, lens, dsts, nonces


def oracle_seal(keys, t, arena, lens, dsts, nonces):
    """The sealed arena by the oracle: own_ip header as additional data, each resolved slot under its peer's key."""
    ref, peers = expect_outgoing(t, arena, lens, dsts)
    for i, L in enumerate(int(x) for x in lens):
        if peers[i] == NO_PEER:
            continue
        o = i * STRIDE
        buf = bytearray(ref[o + 4:o + 4 + L + 28].tobytes())
        O.aesgo_encrypt(keys[peers[i]], buf, L, bytes(ref[o:o + 4]), bytes(nonces[12 * i:12 * i + 12]))
        ref[o + 4:o + 4 + L + 28] = np.frombuffer(bytes(buf), np.uint8)
    return ref, peers


def test_wire_parity(torch, nodes):
    from quantum_amd import batch, route

    tx, rx, keys = nodes
    rng = random.Random(0x3172E)
    n = 257
    t = {a: k for k, a in enumerate(PEERS)}
    arena_h, lens_h, dsts, nonces_h = wire_batch(
        n, rng, lambda i: rng.choice(UNIVERSE[4096:] + OUTSIDE) if i % 9 == 4 else PEERS[rng.randrange(5)])
    route.routes_set(tx, t, NET, MASK, UNMAPPED_GW, OWN)
    arena, _, peer, descs = run_resolve(torch, tx, True, arena_h, lens_h)
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    batch.seal_batch(tx, arena, descs, n, torch.from_numpy(nonces_h).cuda(), status=status)
    ref, peers = oracle_seal(keys, t, arena_h, lens_h, dsts, nonces_h)
    assert (peers == NO_PEER).sum() >= 20 and all((peers == k).sum() >= 20 for k in range(5))
    assert np.array_equal(peer.cpu().numpy().view(np.uint32), peers)
    assert np.array_equal(status.cpu().numpy(), (peers != NO_PEER).astype(np.uint8))
    sealed = arena.cpu().numpy()
    assert np.array_equal(sealed, ref)  # resolved slots == the oracle's seal, unroutable ones unchanged
    # the receiving node: the sender's own_ip maps to the slot holding the key the two share (tx's key 2)
    route.routes_set(rx, {OWN: 3}, NET, MASK, UNMAPPED_GW, PEERS[2])
    mine = [i for i in range(n) if peers[i] == 2]
    stranger = mine[5]
    dgram = sealed.copy()
    dgram[stranger * STRIDE:stranger * STRIDE + 4] = np.frombuffer(le(10, 99, 9, 9).to_bytes(4, "little"), np.uint8)
    dlens = (lens_h + 32).astype(np.uint32)
    arena2, _, peer2, descs2 = run_resolve(torch, rx, False, dgram, dlens)
    senders = [int.from_bytes(dgram[i * STRIDE:i * STRIDE + 4].tobytes(), "little") for i in range(n)]
    want_peer2 = np.array([3 if rule({OWN: 3}, s) is not None else NO_PEER for s in senders], np.uint32)
    assert want_peer2[stranger] == NO_PEER
    check_resolved(n, peer2, descs2, want_peer2, lens_h + 28)
    status2 = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    batch.open_batch(rx, arena2, descs2, n, status=status2)
    st2, opened = status2.cpu().numpy(), arena2.cpu().numpy()
    for i in range(n):
        o, L = i * STRIDE, int(lens_h[i])
        if i in mine and i != stranger:
            assert st2[i] == 1 and np.array_equal(opened[o + 4:o + 4 + L], arena_h[o + 4:o + 4 + L]), i
            assert np.array_equal(opened[o:o + 4], dgram[o:o + 4])
        else:
            assert st2[i] == 0, i  # unmapped sender, unroutable slot, or another peer's key
        if want_peer2[i] == NO_PEER:
            assert np.array_equal(opened[o:o + STRIDE], dgram[o:o + STRIDE]), i  # stays sealed, byte for byte


# ---- link metrics ----

LINKS = [64, 3, 65, 1000, 2047, 0, 500]   # LINKS[0] carries ~90 % of the packets


def metric_batch(seed, n=1000):
    rng = np.random.default_rng(seed)
    peer = np.where(rng.random(n) < 0.9, LINKS[0], np.array(LINKS[1:])[rng.integers(0, 6, n)]).astype(np.uint32)
    peer[rng.random(n) < 0.05] = NO_PEER
    lens = rng.integers(0, 1401, n).astype(np.uint32)
    lens[::37] = np.arange(len(lens[::37])) % 28          # some shorter than tag + nonce
    status = (rng.random(n) >= 0.1).astype(np.uint8)
    return peer, lens, status


def metric_sums(direction, peer, lens, status):
    """The header's table, in numpy: {link or NO_PEER (totals): [Packets, Bytes, DroppedPackets, DroppedBytes]}."""
    out = {k: np.zeros(4, np.uint64) for k in LINKS + [NO_PEER, 1, 66, 2046]}
    for p, L, st in zip(peer.tolist(), lens.tolist(), (status if status is not None else np.ones(len(peer))).tolist()):
        if p == NO_PEER:
            out[NO_PEER][2] += np.uint64(1)
            continue
        if direction == 1 and L < 28:
            st = 0
        row = [1, 4 + L + 28 if direction == 0 else 4 + L - 28, 0, 0] if st == 1 else [0, 0, 1, 4 + L]
        out[NO_PEER] += np.array(row, np.uint64)
        out[p] += np.array(row, np.uint64)
    return out


def read_stats(ctx, direction, links):
    from quantum_amd import route

    return {k: np.array(list(route.route_stats(ctx, direction, k).values()), np.uint64) for k in links}


def device_batch(torch, peer, lens, status):
    from quantum_amd import batch

    n = len(peer)
    return (torch.from_numpy(peer.astype(np.int64)).to(torch.int32).cuda(),
            batch.make_descs(np.arange(n, dtype=np.uint64) * STRIDE, lens, peer, "cuda"),
            None if status is None else torch.from_numpy(status).cuda())


@pytest.mark.parametrize("direction", [0, 1], ids=["tx", "rx"])
def test_metrics(torch, ctx, direction):
    from quantum_amd import route

    route.routes_set(ctx, {}, NET, MASK, GATEWAY, OWN)
    links = LINKS + [NO_PEER, 1, 66, 2046]  # the seven links, the totals, three links nothing is sent on
    base = read_stats(ctx, direction, links)
    other = read_stats(ctx, 1 - direction, links)
    b1, b2, b3, b4 = (metric_batch(0xACC0 + 10 * direction + k) for k in range(4))
    want = {k: base[k].copy() for k in links}

    def add(b, with_status=True):
        s = metric_sums(direction, b[0], b[1], b[2] if with_status else None)
        for k in links:
            want[k] += s[k]

    p, d, st = device_batch(torch, *b1)
    route.route_account(ctx, direction, len(b1[0]), p, d, st)
    torch.cuda.synchronize()
    add(b1)
    got = read_stats(ctx, direction, links)
    for k in links:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert want[LINKS[0]][0] - base[LINKS[0]][0] > 600  # the hot link
    # a second call adds (status NULL: every resolved packet delivered)
    p, d, _ = device_batch(torch, *b2)
    route.route_account(ctx, direction, len(b2[0]), p, d, None)
    torch.cuda.synchronize()
    add(b2, with_status=False)
    got = read_stats(ctx, direction, links)
    for k in links:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    # two calls on two streams: the exact sum of both
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    args3, args4 = device_batch(torch, *b3), device_batch(torch, *b4)
    torch.cuda.synchronize()
    route.route_account(ctx, direction, len(b3[0]), *args3, stream=s1)
    route.route_account(ctx, direction, len(b4[0]), *args4, stream=s2)
    s1.synchronize()
    s2.synchronize()
    add(b3)
    add(b4)
    got = read_stats(ctx, direction, links)
    for k in links:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    # the other direction's counters did not move
    after = read_stats(ctx, 1 - direction, links)
    for k in links:
        assert np.array_equal(after[k], other[k])


# ---- host pipelines ----

def host_arena(kind, data):
    """(address, numpy view, release) of a pinned (qgcm_host_alloc) or pageable copy of `data`."""
    from quantum_amd import _lib

    if kind == "pageable":
        a = data.copy()
        return a.ctypes.data, a, lambda: None
    ptr = _lib.lib().qgcm_host_alloc(len(data))
    assert ptr
    view = np.frombuffer((C.c_uint8 * len(data)).from_address(ptr), np.uint8)
    view[:] = data
    return ptr, view, lambda: _lib.lib().qgcm_host_free(ptr)


def tx_sums(peers, lens, status):
    tot = np.zeros(4, np.uint64)
    for p, L, st in zip(peers.tolist(), lens.tolist(), status.tolist()):
        tot += np.array([0, 0, 1, 0] if p == NO_PEER else [1, 4 + L + 28, 0, 0] if st else [0, 0, 1, 4 + L], np.uint64)
    return tot


@pytest.mark.parametrize("kind", ["pinned", "pageable"])
def test_route_seal_host_and_open_back(torch, nodes, kind):
    from quantum_amd import batch, route

    tx, rx, keys = nodes
    rng = random.Random(0x4057 + len(kind))
    n = 300
    t = {a: 2 for a in PEERS}  # every mapped destination is the peer `rx` stands for
    arena_h, lens_h, dsts, nonces_h = wire_batch(
        n, rng, lambda i: rng.choice(UNIVERSE[4096:]) if i % 11 == 7 else PEERS[rng.randrange(5)])
    route.routes_set(tx, t, NET, MASK, UNMAPPED_GW, OWN)
    # the device path on the same input
    arena, _, peer, descs = run_resolve(torch, tx, True, arena_h, lens_h)
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    batch.seal_batch(tx, arena, descs, n, torch.from_numpy(nonces_h).cuda(), status=status)
    want_arena, want_peer, want_st = arena.cpu().numpy(), peer.cpu().numpy().view(np.uint32), status.cpu().numpy()
    assert 20 <= (want_st == 0).sum() < n and np.array_equal(want_st == 0, want_peer == NO_PEER)
    before = read_stats(tx, 0, [NO_PEER, 2])
    addr, view, release = host_arena(kind, arena_h)
    try:
        h_lens, h_peer, h_st = lens_h.copy(), np.zeros(n, np.uint32), np.full(n, 7, np.uint8)
        dropped = route.route_seal_host(tx, addr, STRIDE, n, h_lens, nonces_h.ctypes.data, h_peer, h_st)
        assert dropped == int((want_st == 0).sum())
        assert np.array_equal(view, want_arena)
        assert np.array_equal(h_peer, want_peer) and np.array_equal(h_st, want_st)
        assert np.array_equal(h_lens, np.where(want_st == 1, lens_h + 32, 0))
        after = read_stats(tx, 0, [NO_PEER, 2])
        sums = tx_sums(want_peer, lens_h, want_st)
        assert np.array_equal(after[NO_PEER] - before[NO_PEER], sums)
        link = sums.copy()
        link[2] -= np.uint64((want_peer == NO_PEER).sum())  # unresolved packets belong to no link
        assert np.array_equal(after[2] - before[2], link)
        # the receiving node opens the arena back, one datagram tampered with
        route.routes_set(rx, {OWN: 3}, NET, MASK, UNMAPPED_GW, PEERS[2])
        sealed = [i for i in range(n) if want_st[i]]
        bad = sealed[17]
        view[bad * STRIDE + 4 + 5] ^= 0x40
        rbefore = read_stats(rx, 1, [NO_PEER, 3])
        r_lens, r_peer, r_st = h_lens.copy(), np.zeros(n, np.uint32), np.full(n, 7, np.uint8)
        rdropped = route.route_open_host(rx, addr, STRIDE, n, r_lens, r_peer, r_st)
        assert rdropped == n - len(sealed) + 1
        for i in range(n):
            o, L = i * STRIDE, int(lens_h[i])
            if want_st[i] and i != bad:
                assert r_st[i] == 1 and r_peer[i] == 3 and r_lens[i] == L, i
                assert np.array_equal(view[o + 4:o + 4 + L], arena_h[o + 4:o + 4 + L]), i
            elif i == bad:
                assert r_st[i] == 0 and r_peer[i] == 3 and r_lens[i] == 0
                assert not view[o + 4:o + 4 + L].any()  # errOpen: the plaintext region zeroed
            else:
                assert r_st[i] == 0 and r_peer[i] == NO_PEER and r_lens[i] == 0  # length 0: no sender to read
                assert np.array_equal(view[o:o + STRIDE], want_arena[o:o + STRIDE])
        rafter = read_stats(rx, 1, [NO_PEER, 3])
        ok_bytes = sum(4 + int(lens_h[i]) for i in sealed if i != bad)  # 4 + (L + 28) - 28
        bad_bytes = 4 + int(lens_h[bad]) + 28                            # dropped: the length it came with
        assert (rafter[3] - rbefore[3]).tolist() == [len(sealed) - 1, ok_bytes, 1, bad_bytes]
        assert (rafter[NO_PEER] - rbefore[NO_PEER]).tolist() == [len(sealed) - 1, ok_bytes, 1 + n - len(sealed), bad_bytes]
    finally:
        del view
        release()


def test_route_seal_host_generates_nonces(torch, nodes):
    from quantum_amd import batch, route

    tx, rx, keys = nodes
    rng = random.Random(0x6E6)
    n = 300
    arena_h, lens_h, dsts, _ = wire_batch(n, rng, lambda i: PEERS[rng.randrange(5)])
    route.routes_set(tx, {a: 2 for a in PEERS}, NET, MASK, UNMAPPED_GW, OWN)
    route.routes_set(rx, {OWN: 3}, NET, MASK, UNMAPPED_GW, PEERS[2])
    work = arena_h.copy()
    h_lens, h_peer = lens_h.copy(), np.zeros(n, np.uint32)
    assert route.route_seal_host(tx, work.ctypes.data, STRIDE, n, h_lens, batch.GENERATE, h_peer) == 0
    assert np.array_equal(h_lens, lens_h + 32) and (h_peer == 2).all()
    nonces = {work[i * STRIDE + 4 + int(L) + 16:i * STRIDE + 4 + int(L) + 28].tobytes() for i, L in enumerate(lens_h)}
    assert len(nonces) == n  # one fresh nonce per packet
    assert route.route_open_host(rx, work.ctypes.data, STRIDE, n, h_lens, h_peer) == 0
    assert np.array_equal(h_lens, lens_h) and (h_peer == 3).all()
    for i, L in enumerate(int(x) for x in lens_h):
        assert np.array_equal(work[i * STRIDE + 4:i * STRIDE + 4 + L], arena_h[i * STRIDE + 4:i * STRIDE + 4 + L]), i


def test_arguments(torch):
    from quantum_amd import _lib, route
    from quantum_amd.crypto import Context

    L = _lib.lib()
    c = Context(device=0, max_keys=4)
    try:
        n = 8
        arena = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
        lens = torch.full((n,), 64, dtype=torch.int32, device="cuda")
        peer = torch.zeros(n, dtype=torch.int32, device="cuda")
        descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        a, l_, p, d = (int(x.data_ptr()) for x in (arena, lens, peer, descs))
        out = (C.c_uint64 * 4)()
        host = np.zeros(n * STRIDE, np.uint8)
        hl, hp = np.full(n, 64, np.uint32), np.zeros(n, np.uint32)

        def all_refused():
            assert L.qgcm_resolve_outgoing(c.handle, a, STRIDE, n, l_, p, d, None) == _lib.QGCM_E_ARG
            assert L.qgcm_resolve_incoming(c.handle, a, STRIDE, n, l_, p, d, None) == _lib.QGCM_E_ARG
            assert L.qgcm_resolve_outgoing(c.handle, a, STRIDE, 0, l_, p, d, None) == _lib.QGCM_E_ARG
            assert L.qgcm_route_account(c.handle, 0, n, p, d, None, None) == _lib.QGCM_E_ARG
            assert L.qgcm_route_stats(c.handle, 0, NO_PEER, C.addressof(out)) == _lib.QGCM_E_ARG
            assert L.qgcm_route_seal_host(c.handle, host.ctypes.data, STRIDE, n, hl.ctypes.data, None, hp.ctypes.data,
                                          None) == _lib.QGCM_E_ARG
            assert L.qgcm_route_open_host(c.handle, host.ctypes.data, STRIDE, n, hl.ctypes.data, hp.ctypes.data,
                                          None) == _lib.QGCM_E_ARG

        all_refused()  # before any qgcm_routes_set
        with pytest.raises(_lib.QgcmError):
            route.routes_set(c, {PEERS[0]: 1, PEERS[1]: 4}, NET, MASK, GATEWAY, OWN)  # peer >= max_keys
        all_refused()  # ... which installed nothing
        route.routes_set(c, {PEERS[0]: 3}, NET, MASK, GATEWAY, OWN)
        assert L.qgcm_resolve_outgoing(c.handle, a, STRIDE - 2, n, l_, p, d, None) == _lib.QGCM_E_ARG
        assert L.qgcm_resolve_incoming(c.handle, a, STRIDE + 1, n, l_, p, d, None) == _lib.QGCM_E_ARG
        assert L.qgcm_route_seal_host(c.handle, host.ctypes.data, STRIDE - 2, n, hl.ctypes.data, None, hp.ctypes.data,
                                      None) == _lib.QGCM_E_ARG
        too_many = (1 << 31) + 1
        assert L.qgcm_resolve_outgoing(c.handle, a, STRIDE, too_many, l_, p, d, None) == _lib.QGCM_E_ARG
        assert L.qgcm_resolve_incoming(c.handle, a, STRIDE, too_many, l_, p, d, None) == _lib.QGCM_E_ARG
        assert L.qgcm_route_account(c.handle, 0, too_many, p, d, None, None) == _lib.QGCM_E_ARG
        assert L.qgcm_route_account(c.handle, 2, n, p, d, None, None) == _lib.QGCM_E_ARG
        assert L.qgcm_route_stats(c.handle, 0, 4, C.addressof(out)) == _lib.QGCM_E_ARG
        for call in (L.qgcm_resolve_outgoing, L.qgcm_resolve_incoming):
            assert call(c.handle, None, STRIDE, 0, None, None, None, None) == _lib.QGCM_OK  # n == 0
        assert L.qgcm_route_account(c.handle, 1, 0, None, None, None, None) == _lib.QGCM_OK
        assert L.qgcm_route_seal_host(c.handle, None, STRIDE, 0, None, None, None, None) == 0
        assert L.qgcm_resolve_outgoing(c.handle, a, STRIDE, n, l_, p, d, None) == _lib.QGCM_OK
        torch.cuda.synchronize()
        assert L.qgcm_route_stats(c.handle, 0, NO_PEER, C.addressof(out)) == _lib.QGCM_OK and list(out) == [0, 0, 0, 0]
    finally:
        c.close()
