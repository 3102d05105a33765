"""GPU: qgcm_train_pack (quantum_amd/csrc/train_kernels.hip) writes exactly what tests/train_pack_model.py writes
-- the packed area whole, inside sentinel margins on both sides (so the zero padding, the bytes shared granules
keep and the untouched bytes behind the used part are all proven), ptrains[0:t) and pcounts -- and the packed
outgoing pipeline gives what qgcm_route_chain_seal_host gives, with its datagrams as qgcm_send_plan_cpu and
qgcm_train_pack_cpu plan and pack them.

The scan works in tiles of 256 trains (one workgroup per tile, one lane per train); the spine is one workgroup of
1024 lanes, so from 1025 tiles on (262 145 trains) a lane folds more than one tile.  The copy gives 16 lanes to a
datagram and 16 datagrams to a workgroup, and its grid stops at 4096 workgroups: 70 000 datagrams take 4 375
workgroups' worth, so the grid-stride loop runs."""
import numpy as np
import pytest

import train_pack_model as M
from quantum_amd import _lib, route
from send_plan_wire import Wire
from test_gpu_chain_route import BOTH, MAX_KEYS, addr, stats
from test_gpu_gro import loop_ctx

pytestmark = pytest.mark.gpu

TILE = 256
MARGIN = 64


def as_plan(order, trains):
    return np.ascontiguousarray(order, np.uint32), np.ascontiguousarray(trains, np.uint32).reshape(-1, 4)


class DevTrain:
    """One qgcm_train_pack call enqueued on `stream` over sentinel-filled outputs; read() after a synchronize.
    The plan comes from the host (order, trains, m, t), or, with `plan_from` = (lens, peer), from
    qgcm_send_plan on the same stream with nothing in between."""

    def __init__(self, ctx, arena, stride, n, order, trains, m=None, t=None, packed_cap=None, stream=None, arena_shift=0,
                 plan_from=None):
        import torch

        order, trains = as_plan(order, trains)
        self.n, self.stride = n, stride
        self.m, self.t = len(order) if m is None else m, len(trains) if t is None else t
        self.cap = M.need(trains) if packed_cap is None else packed_cap
        self.whole = torch.empty(arena.size + arena_shift, dtype=torch.uint8, device="cuda")
        self.arena = self.whole[arena_shift:]
        self.arena.copy_(torch.from_numpy(arena))
        packed, ptrains, pcounts = M.fresh(n, MARGIN + self.cap + MARGIN)
        self.area = torch.from_numpy(packed).cuda()
        self.packed = self.area[MARGIN:]
        self.ptrains = torch.from_numpy(ptrains.view(np.int32).reshape(-1)).cuda()
        self.pcounts = torch.from_numpy(pcounts.view(np.int64)).cuda()
        self.work = route.train_pack_work(n)
        self.work.fill_(0xEE)  # the scan takes nothing for zero
        rows = max(1, n)
        if plan_from is None:
            h_order, h_trains = np.full(rows, 0xFFFFFFF0, np.uint32), np.full((rows, 4), M.PT_SENTINEL, np.uint32)
            h_order[:len(order)], h_trains[:len(trains)] = order, trains
            self.order = torch.from_numpy(h_order.view(np.int32)).cuda()
            self.trains = torch.from_numpy(h_trains.view(np.int32).reshape(-1)).cuda()
            self.plan_counts = torch.from_numpy(np.array([self.m, self.t], np.uint32).view(np.int32)).cuda()
            torch.cuda.synchronize()  # the inputs are there whatever stream packs
        else:
            lens, peer = plan_from
            self.lens, self.peer = torch.from_numpy(lens.view(np.int32)).cuda(), torch.from_numpy(peer.view(np.int32)).cuda()
            self.order = torch.zeros(rows, dtype=torch.int32, device="cuda")
            self.trains = torch.zeros(4 * rows, dtype=torch.int32, device="cuda")
            self.plan_counts = torch.zeros(2, dtype=torch.int32, device="cuda")
            self.plan_work = route.send_plan_work(n)
            torch.cuda.synchronize()
            route.send_plan(ctx, n, self.lens, self.peer, self.order, self.trains, self.plan_counts, self.plan_work, None, stream)
        route.train_pack(ctx, self.arena, stride, n, self.order, self.trains, self.plan_counts, self.packed, self.cap,
                         self.ptrains, self.pcounts, self.work, stream)

    def read(self):
        return (self.area.cpu().numpy(), self.ptrains.cpu().numpy().view(np.uint32).reshape(-1, 4),
                self.pcounts.cpu().numpy().view(np.uint64))


def check(dev, arena, order, trains, bytes_determined=True):
    order, trains = as_plan(order, trains)
    want_area = np.full(MARGIN + dev.cap + MARGIN, M.SENTINEL, np.uint8)
    model = M.pack if dev.m <= 4096 or not M.well_formed(dev.stride, dev.n, order, dev.m, trains, dev.t) else M.pack_fast
    # the model writes into a view that ends at packed_cap: a write past it would raise
    want, (t, total) = model(arena, dev.stride, dev.n, order, trains, dev.m, dev.t, want_area[MARGIN:MARGIN + dev.cap], dev.cap)
    area, ptrains, pcounts = dev.read()
    assert pcounts.tolist() == [t, total]
    bad = np.flatnonzero(np.any(ptrains[:t] != want, axis=1))
    assert bad.size == 0, [(int(k), ptrains[k].tolist(), want[k].tolist()) for k in bad[:8]]
    assert np.all(ptrains[t:] == M.PT_SENTINEL) or t == dev.n
    assert np.all(area[:MARGIN] == M.SENTINEL) and np.all(area[MARGIN + dev.cap:] == M.SENTINEL)  # the margins
    if bytes_determined and not np.array_equal(area, want_area):
        at = np.flatnonzero(area != want_area)
        raise AssertionError(f"{at.size} packed bytes differ, the first at {int(at[0]) - MARGIN} of {dev.cap}")
    return want


def run(ctx, arena, stride, n, order, trains, **kw):
    import torch

    dev = DevTrain(ctx, arena, stride, n, order, trains, **kw)
    torch.cuda.synchronize()
    return check(dev, arena, order, trains)


# ---- 1. edges ----

@pytest.mark.parametrize("stride,shift", ((1536, 0), (1388, 0), (1536, 4)))
def test_edges(ctx, stride, shift):
    """Every seg_len x count pair of the model's edge batch, peers interleaved.  Stride 1536 takes the 16-byte
    path, 1388 the dword path, and an arena 4 bytes off its 16-B boundary sends stride 1536 down the dword path.
    (A slot of 1388 bytes holds no 1472-byte datagram: there the batch has the lengths up to 1383 and 1388.)"""
    arena, lens, peer, max_keys = M.edge_batch(stride)
    order, trains = M.plan_of(lens, peer, max_keys)
    want = run(ctx, arena, stride, len(lens), order, trains, arena_shift=shift)
    assert {1, 5, 17, 1383, min(stride, 1472)} <= set(want[:, 3].tolist()) and {1, 2, 3, 16, 17} <= set(want[:, 1].tolist())


# ---- 2. scan tiles, 3. spine ----

@pytest.mark.parametrize("t", (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1))
def test_around_the_scan_tile(ctx, t):
    arena, lens, peer, max_keys = M.random_batch(0x711E + t, t, 256, lengths=(1, 36, 60, 255), junk=0.0)
    order, trains = M.plan_of(lens, peer, max_keys, max_segs=1)
    assert len(trains) == t
    run(ctx, arena, 256, t, order, trains)


def test_the_spine_folds_two_tiles_a_lane(ctx):
    """1026 tiles of trains of one for the spine's 1024 lanes: slots of 8 bytes, datagrams of 4."""
    n = 1025 * TILE + 45
    arena = M.arena_of(0x5B1AE, n, 8)
    order = np.random.default_rng(0x5B1AF).permutation(n).astype(np.uint32)
    trains = np.stack([np.arange(n), np.ones(n, np.int64), np.arange(n) % 1024, np.full(n, 4)], axis=1).astype(np.uint32)
    want = run(ctx, arena, 8, n, order, trains)
    assert int(want[-1, 0]) == 16 * (n - 1)


# ---- 4. grid-stride wrap ----

def test_the_grid_stride_loop_wraps(ctx):
    n = 70000
    rng = np.random.default_rng(0x70000)
    arena = M.arena_of(0x70001, n, 64)
    lens = np.array((20, 33, 64), np.uint32)[rng.integers(0, 3, n)]
    peer = rng.integers(0, 5, n).astype(np.uint32)
    order, trains = route.send_plan_cpu(lens, peer, 8)
    assert len(order) == n > 4096 * 16
    run(ctx, arena, 64, n, order, trains)


# ---- 5. packed_cap cuts ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_packed_cap_cuts_the_batch(ctx, stride):
    """Caps at a train's start, one byte before its end, at a value off the 16-byte grid inside it and exactly at
    its end: off == 0xffffffff for a suffix, pcounts[1] the full need, and the bytes behind the last train that
    fits keep their sentinel (check() compares the whole area with the model's)."""
    arena, lens, peer, max_keys = M.random_batch(0xCA9 + stride, 600, stride)
    order, trains = M.plan_of(lens, peer, max_keys)
    full = run(ctx, arena, stride, 600, order, trains)
    k = 2 * len(full) // 3
    start, size = int(full[k, 0]), M.train_bytes(int(full[k, 1]), int(full[k, 3]))
    assert size > 32
    for cap, fitted in ((start, k), (start + size - 1, k), (start + size - 9, k), (start + size, k + 1), (0, 0)):
        want = run(ctx, arena, stride, 600, order, trains, packed_cap=cap)
        assert np.all(want[:fitted, 0] != M.NO_ROOM) and np.all(want[fitted:, 0] == M.NO_ROOM)


# ---- 6. two streams ----

def test_two_streams_at_once(ctx):
    import torch

    a = M.random_batch(61, 4099, 1536)
    b = M.random_batch(62, 5000, 1388, peers=40)
    plans = [M.plan_of(x[1], x[2], x[3]) for x in (a, b)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = [(a, 1536, plans[0], s1, None), (b, 1388, plans[1], s2, None), (a, 1536, plans[0], s2, 100000),
            (b, 1388, plans[1], s1, None)]
    devs = [DevTrain(ctx, x[0], stride, len(x[1]), *plan, stream=s, packed_cap=cap) for x, stride, plan, s, cap in jobs]
    torch.cuda.synchronize()
    for dev, (x, _, plan, _, _) in zip(devs, jobs):
        check(dev, x[0], *plan)


# ---- 7. the plan straight from qgcm_send_plan ----

@pytest.mark.parametrize("n,stride", ((3000, 1536), (70001, 64)))
def test_the_plan_comes_from_the_device_planner_on_the_same_stream(ctx, n, stride):
    """qgcm_send_plan and qgcm_train_pack enqueued back to back on one stream: the pack reads m and t where the
    planner left them.  (The session's context has 2048 key slots.)"""
    import torch

    arena, lens, peer, _ = M.random_batch(0xD0 + n, n, stride, peers=9)
    order, trains = route.send_plan_cpu(lens, peer, 2048)
    s = torch.cuda.Stream()
    dev = DevTrain(ctx, arena, stride, n, order, trains, stream=s, plan_from=(lens, peer))
    torch.cuda.synchronize()
    assert dev.plan_counts.cpu().numpy().view(np.uint32).tolist() == [len(order), len(trains)]
    check(dev, arena, order, trains)


# ---- 8. argument errors ----

def test_argument_errors_launch_nothing(ctx):
    import torch

    L = _lib.lib()
    arena, lens, peer, max_keys = M.random_batch(0xA46, 200, 1536)
    order, trains = M.plan_of(lens, peer, max_keys)
    dev = DevTrain(ctx, arena, 1536, 200, order, trains)
    torch.cuda.synchronize()
    check(dev, arena, order, trains)
    packed, ptrains, pcounts = M.fresh(200, dev.cap + MARGIN)
    d_packed, d_pt = torch.from_numpy(packed).cuda(), torch.from_numpy(ptrains.view(np.int32).reshape(-1)).cuda()
    d_counts = torch.from_numpy(np.concatenate([pcounts, pcounts]).view(np.int64)).cuda()
    ptr = lambda x: int(x.data_ptr())
    good = [ctx.handle, ptr(dev.arena), 1536, 200, ptr(dev.order), ptr(dev.trains), ptr(dev.plan_counts), ptr(d_packed),
            dev.cap, ptr(d_pt), ptr(d_counts), ptr(dev.work), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_train_pack(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a3=(1 << 31) + 1) == _lib.QGCM_E_ARG                             # n > QGCM_MAX_BATCH
    assert call(a2=1538) == _lib.QGCM_E_ARG and call(a2=0) == _lib.QGCM_E_ARG  # stride no multiple of 4, or none
    assert call(a8=(1 << 32) - 15) == _lib.QGCM_E_ARG                           # off is 32 bits
    for k in (1, 4, 5, 6, 7, 9, 10, 11):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a1=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a4=ptr(dev.order) + 2) == _lib.QGCM_E_ARG and call(a6=ptr(dev.plan_counts) + 2) == _lib.QGCM_E_ARG
    assert call(a5=ptr(dev.trains) + 8) == _lib.QGCM_E_ARG   # the plan's table off its 16-B boundary
    assert call(a7=ptr(d_packed) + 4) == _lib.QGCM_E_ARG     # the packed area off its 16-B boundary
    assert call(a9=ptr(d_pt) + 8) == _lib.QGCM_E_ARG         # the packed table off its 16-B boundary
    assert call(a10=ptr(d_counts) + 4) == _lib.QGCM_E_ARG    # the counts off their 8-B boundary
    assert call(a11=ptr(dev.work) + 4) == _lib.QGCM_E_ARG
    torch.cuda.synchronize()
    assert np.all(d_packed.cpu().numpy() == M.SENTINEL) and np.all(d_pt.cpu().numpy().view(np.uint32) == M.PT_SENTINEL)
    assert np.all(d_counts.cpu().numpy().view(np.uint64) == M.COUNT_SENTINEL)
    # n == 0 writes the counts and nothing else; then the good call
    assert call(a3=0, a1=None, a4=None, a5=None, a6=None, a7=None, a9=None, a11=None, a10=ptr(d_counts) + 16) == 0
    torch.cuda.synchronize()
    assert d_counts.cpu().numpy().view(np.uint64).tolist() == [M.COUNT_SENTINEL] * 2 + [0, 0]
    assert np.all(d_packed.cpu().numpy() == M.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    want = np.full(dev.cap + MARGIN, M.SENTINEL, np.uint8)
    want_pt, (t, total) = M.pack(arena, 1536, 200, order, trains, len(order), len(trains), want, dev.cap)
    assert np.array_equal(d_packed.cpu().numpy(), want) and d_counts.cpu().numpy().view(np.uint64)[:2].tolist() == [t, total]
    assert np.array_equal(d_pt.cpu().numpy().view(np.uint32).reshape(-1, 4)[:t], want_pt)


# ---- 9. malformed plans ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_malformed_plans_stay_inside_their_bounds(ctx, stride):
    """Every class of plan that is not well-formed returns QGCM_OK and gives the model's void and zero rules; the
    margins on both sides of the packed area keep their sentinel.  The cap is the well-formed plan's need, which
    every one of these plans stays below; a second run under a cap that cuts mid-way shows nothing at or past it
    changes either."""
    import torch

    n = 300
    arena, lens, peer, max_keys = M.random_batch(0xBAD, n, stride, peers=3)
    order, trains = M.plan_of(lens, peer, max_keys)
    cap = M.need(trains)
    for name, o, tr, m, t, tiles in M.malformed_plans(stride, n, order, trains):
        assert not M.well_formed(stride, n, o, m, tr, t), name
        for c in (cap, cap // 2 + 5):
            dev = DevTrain(ctx, arena, stride, n, o, tr, m=m, t=t, packed_cap=c)
            torch.cuda.synchronize()
            want = check(dev, arena, o, tr, bytes_determined=tiles)
            if c == cap and name not in ("order-at-n", "order-wraps", "m-above-n"):
                assert np.any(want[:, 0] == M.NO_ROOM), name  # a void train


# ---- 10 - 12. the packed outgoing pipeline ----

SEAL_STRIDE = 1472


def tun_batch(f, n, seed, stride=SEAL_STRIDE):
    """n TUN packets of random bytes (they do not compress, so a peer's packets of one length stay one length) to
    the peers of flags f -- f + 4 has no key: its packets are dropped by the seal -- in stretches of 25 packets of
    64, 700 and 1350 bytes, a stranger now and then.  -> (head (n, 1472): the slots' first bytes, lens, nonces)."""
    from test_gpu_chain_route import STRANGER

    dests = (f, f + 8, f + 4)
    rng = np.random.default_rng(seed)
    head = rng.integers(0, 256, (n, SEAL_STRIDE), dtype=np.uint8)
    for i in range(n):
        dst = STRANGER if i % 37 == 11 else addr(dests[(i // 10) % 3])
        head[i, 20:24] = np.frombuffer(dst.to_bytes(4, "little"), np.uint8)
    lens = np.array((64, 700, 1350), np.uint32)[(np.arange(n) // 25) % 3]
    return head, lens, rng.integers(0, 256, 12 * n, dtype=np.uint8)


def slots_of(head, stride):
    n = len(head)
    if stride == SEAL_STRIDE:
        return head.reshape(-1).copy()
    arena = np.zeros(n * stride, np.uint8)
    arena.reshape(n, stride)[:, :SEAL_STRIDE] = head
    return arena


def existing(c, arena, stride, n, lens, nonces):
    """qgcm_route_chain_seal_host on a copy -> (arena out, lens, peer, status, rc, Tx counters added)."""
    out, h_lens = arena.copy(), lens.copy()
    peer, status = np.full(n, 7, np.uint32), np.full(n, 0xAB, np.uint8)
    t0, l0 = stats(c, route.TX)
    rc = route.route_chain_seal_host(c, out.ctypes.data, stride, n, h_lens, nonces.ctypes.data, BOTH, peer, status)
    t1, l1 = stats(c, route.TX)
    return out, h_lens, peer, status, rc, (t1 - t0, l1 - l0)


def planned_and_packed(arena, stride, lens, peer, fill=0, first_slot=0):
    """qgcm_send_plan_cpu + qgcm_train_pack_cpu of a chunk, rebased -> (bytes, ptrains, order)."""
    order, trains = route.send_plan_cpu(lens, peer, MAX_KEYS)
    packed = np.zeros(M.need(trains), np.uint8)
    ptrains, total = route.train_pack_cpu(arena, stride, len(lens), order, trains, packed)
    assert total == packed.size
    ptrains = ptrains.copy()
    ptrains[:, 0] += fill
    return packed, ptrains, order + np.uint32(first_slot)


def packed_call(c, arena, stride, n, lens, nonces, out_bytes):
    before = arena.copy() if arena.size < (1 << 26) else None
    h_lens, peer, status = lens.copy(), np.full(n, 7, np.uint32), np.full(n, 0xAB, np.uint8)
    out_buf = np.full(out_bytes, M.SENTINEL, np.uint8)
    ptrains, order = np.full((n, 4), M.PT_SENTINEL, np.uint32), np.full(n, M.PT_SENTINEL, np.uint32)
    t0, l0 = stats(c, route.TX)
    rc, pt, od, out = route.route_chain_seal_packed_host(c, arena.ctypes.data, stride, n, h_lens, nonces.ctypes.data, BOTH,
                                                         peer, status, out_buf, None, ptrains, order)
    t1, l1 = stats(c, route.TX)
    if before is not None:
        assert np.array_equal(arena, before)  # h_arena is never written
    assert np.all(ptrains[len(pt):] == M.PT_SENTINEL) and np.all(order[len(od):] == M.PT_SENTINEL)
    return rc, pt, od, out, out_buf, (h_lens, peer, status), (t1 - t0, l1 - l0)


def same_tx(got, want):
    assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1])


def one_chunk(f, n=150, seed=0x7A0):
    """The existing call on one context, the packed one on a second with the same keys and nonces."""
    c, c2 = loop_ctx(f), loop_ctx(f)
    try:
        head, lens, nonces = tun_batch(f, n, seed + f)
        arena = slots_of(head, SEAL_STRIDE)
        ref_arena, ref_lens, ref_peer, ref_status, ref_rc, ref_tx = existing(c, arena, SEAL_STRIDE, n, lens, nonces)
        want_bytes, want_pt, want_order = planned_and_packed(ref_arena, SEAL_STRIDE, ref_lens, ref_peer)
        assert len(want_order) >= 60 and ref_rc >= 1 and len({int(x) % 16 for x in want_pt[:, 3]}) >= 2
        rc, pt, od, out, out_buf, got, tx = packed_call(c2, arena, SEAL_STRIDE, n, lens, nonces, want_bytes.size + 64)
        assert rc == ref_rc and out.tolist() == [n, len(want_pt), want_bytes.size, len(want_order)]
        for g, w in zip(got, (ref_lens, ref_peer, ref_status)):
            assert np.array_equal(g, w)
        same_tx(tx, ref_tx)
        assert np.array_equal(pt, want_pt) and np.array_equal(od, want_order)
        assert np.array_equal(out_buf[:want_bytes.size], want_bytes) and np.all(out_buf[want_bytes.size:] == M.SENTINEL)
        return c, head, lens, out_buf[:want_bytes.size].copy(), pt.copy(), od.copy()
    finally:
        c2.close()


@pytest.mark.parametrize("f", (0, 1, 2, 3))
def test_packed_pipeline_matches_the_existing_one(f):
    one_chunk(f)[0].close()


def test_packed_pipeline_in_two_chunks():
    """Slots of 1 MiB: a chunk holds 256 of them, so 300 packets are sealed, planned and packed in two chunks and
    the second chunk's trains are rebased (off by the first chunk's bytes, order by its packets).  Then an h_out
    16 bytes short of the second chunk's need: QGCM_E_NOMEM with the first chunk done and accounted alone; a
    second call from packet out[0] completes, and both calls together give the one call's result."""
    stride, n, first = 1 << 20, 300, 256
    ctxs = [loop_ctx(3) for _ in range(4)]
    c, c2, c3, c4 = ctxs
    try:
        head, lens, nonces = tun_batch(3, n, 0x2C5)
        arena = slots_of(head, stride)
        ref_arena, ref_lens, ref_peer, ref_status, ref_rc, ref_tx = existing(c, arena, stride, n, lens, nonces)
        b1, pt1, od1 = planned_and_packed(ref_arena[:first * stride], stride, ref_lens[:first], ref_peer[:first])
        b2, pt2, od2 = planned_and_packed(ref_arena[first * stride:], stride, ref_lens[first:], ref_peer[first:], b1.size, first)
        del ref_arena
        want_bytes, want_pt, want_order = np.concatenate([b1, b2]), np.concatenate([pt1, pt2]), np.concatenate([od1, od2])
        assert len(od2) >= 20 and b1.size % 16 == 0
        rc, pt, od, out, out_buf, got, tx = packed_call(c2, arena, stride, n, lens, nonces, want_bytes.size)
        assert rc == ref_rc and out.tolist() == [n, len(want_pt), want_bytes.size, len(want_order)]
        for g, w in zip(got, (ref_lens, ref_peer, ref_status)):
            assert np.array_equal(g, w)
        same_tx(tx, ref_tx)
        assert np.array_equal(pt, want_pt) and np.array_equal(od, want_order) and np.array_equal(out_buf, want_bytes)

        # what the first chunk alone adds to the counters: the existing call on it, on a context of its own
        _, lens4, peer4, status4, rc4, first_tx = existing(c4, arena[:first * stride], stride, first, lens[:first], nonces[:12 * first])
        rc, pt, od, out, out_buf, got, tx = packed_call(c3, arena, stride, n, lens, nonces, want_bytes.size - 16)
        assert rc == _lib.QGCM_E_NOMEM and out.tolist() == [first, len(pt1), b1.size, len(od1)]
        same_tx(tx, first_tx)
        assert np.array_equal(pt, pt1) and np.array_equal(od, od1)
        assert np.array_equal(out_buf[:b1.size], b1) and np.all(out_buf[b1.size:] == M.SENTINEL)
        for g, w in zip(got, (lens4, peer4, status4)):
            assert np.array_equal(g[:first], w)
        assert np.array_equal(got[0][first:], lens[first:])  # the remainder's input is whole
        # the remainder, from packet out[0]
        rc_b, pt_b, od_b, out_b, buf_b, got_b, tx_b = packed_call(c3, arena[first * stride:], stride, n - first, lens[first:],
                                                                  nonces[12 * first:], b2.size)
        assert rc_b >= 0 and rc4 + rc_b == ref_rc
        assert out_b.tolist() == [n - first, len(pt2), b2.size, len(od2)]
        same_tx((tx[0] + tx_b[0], tx[1] + tx_b[1]), ref_tx)  # both calls together
        assert np.array_equal(buf_b, b2)
        assert np.array_equal(pt_b.astype(np.int64) + [b1.size, 0, 0, 0], pt2) and np.array_equal(od_b + np.uint32(first), od2)
        for g, gb, w in zip(got, got_b, (ref_lens, ref_peer, ref_status)):
            assert np.array_equal(np.concatenate([g[:first], gb]), w)
    finally:
        for x in ctxs:
            x.close()


def test_the_packed_output_crosses_the_wire_and_opens():
    """The packed output of the one-chunk pipeline, sent by qgcm_udp_send_packed over loopback, received into
    slots by qgcm_udp_recv_slots and opened by the peer context: the original packets, in table order."""
    f = 3
    c, head, lens, packed, ptrains, order = one_chunk(f)
    wire = Wire(1)
    try:
        m = len(order)
        addrs = route.peer_addrs([("127.0.0.1", wire.L.qgcm_udp_port(wire.rx[0]))] * MAX_KEYS)
        sent_stats = np.zeros(3, np.uint64)
        assert route.udp_send_packed(wire.tx, packed, packed.size, ptrains, addrs, MAX_KEYS, sent_stats) == m
        grams = wire.drain(0, m)
        assert len(grams) == m and int(sent_stats[0]) <= m
        arena, got_lens = np.zeros((m, SEAL_STRIDE), np.uint8), np.zeros(m, np.uint32)
        for j, g in enumerate(grams):
            arena[j, :len(g)] = np.frombuffer(g, np.uint8)
            got_lens[j] = len(g)
        peer, status = np.zeros(m, np.uint32), np.full(m, 0xAB, np.uint8)
        assert route.route_chain_open_host(c, arena.ctypes.data, SEAL_STRIDE, m, got_lens, BOTH, peer, status) == 0
        for j, src in enumerate(order.tolist()):  # one sender, one receiver: arrival order is table order
            L = int(lens[src])
            assert status[j] == 1 and peer[j] == 20 and got_lens[j] == L, (j, src)
            assert np.array_equal(arena[j, 4:4 + L], head[src, 4:4 + L]), (j, src)
    finally:
        wire.close()
        c.close()
