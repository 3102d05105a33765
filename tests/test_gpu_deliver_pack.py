"""GPU: qgcm_deliver_pack (quantum_amd/csrc/pack_kernels.hip) writes exactly what tests/deliver_pack_model.py
writes -- the packed area whole (over sentinels, so the zero padding and the untouched bytes behind the used part
are both proven), recs[0:m) and counts -- and the two packed pipelines give what the existing pipelines give, with
the delivered packets as qgcm_deliver_pack_cpu packs them.

The scan works in tiles of 256 packets (kPackTile, one workgroup per tile, one lane per packet); the spine is one
workgroup of 1024 lanes, so from 1025 tiles on (262 145 packets) a lane folds more than one tile.  The copy gives
16 lanes to a record and 16 records to a workgroup, and its grid stops at 4096 workgroups: the 70 001-packet
batches take 4 376 workgroups' worth of records, so the grid-stride loop runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import deliver_pack_model as M
import test_gpu_gro as G
from quantum_amd import _lib, route
from test_gpu_chain_route import BOTH, stats

pytestmark = pytest.mark.gpu

TILE = 256


class DevPack:
    """One qgcm_deliver_pack call enqueued on `stream` over sentinel-filled outputs; read() after a synchronize."""

    def __init__(self, ctx, case, stride, packed_cap=None, stream=None, arena_shift=0):
        import torch

        arena, lens, peer, status = case
        self.n = n = len(lens)
        self.cap = M.need(lens, status, stride) if packed_cap is None else packed_cap
        self.whole = torch.empty(arena.size + arena_shift, dtype=torch.uint8, device="cuda")
        self.arena = self.whole[arena_shift:]
        self.arena.copy_(torch.from_numpy(arena))
        self.lens = torch.from_numpy(lens.view(np.int32)).cuda()
        self.peer = torch.from_numpy(peer.view(np.int32)).cuda()
        self.status = None if status is None else torch.from_numpy(status).cuda()
        packed, recs, counts = M.fresh(n, self.cap + 64)
        self.packed = torch.from_numpy(packed).cuda()
        self.recs = torch.from_numpy(recs.view(np.int32).reshape(-1)).cuda()
        self.counts = torch.from_numpy(counts.view(np.int64)).cuda()
        self.work = route.deliver_pack_work(n)
        self.work.fill_(0xEE)  # the scan takes nothing for zero
        torch.cuda.synchronize()  # the inputs are there whatever stream packs
        route.deliver_pack(ctx, self.arena, stride, n, self.lens, self.peer, self.status, self.packed, self.cap,
                           self.recs, self.counts, self.work, stream)

    def read(self):
        return (self.packed.cpu().numpy(), self.recs.cpu().numpy().view(np.uint32).reshape(-1, 4),
                self.counts.cpu().numpy().view(np.uint64))


def check(dev, case, stride):
    arena, lens, peer, status = case
    want_packed = np.full(dev.cap + 64, M.SENTINEL, np.uint8)
    model = M.pack if dev.n <= 4096 else M.pack_fast
    want_recs, (m, total) = model(arena, stride, dev.n, lens, peer, status, want_packed, dev.cap)
    packed, recs, counts = dev.read()
    assert counts.tolist() == [m, total]
    bad = np.flatnonzero(np.any(recs[:m] != want_recs, axis=1))
    assert bad.size == 0, [(int(k), recs[k].tolist(), want_recs[k].tolist()) for k in bad[:8]]
    if not np.array_equal(packed, want_packed):
        at = np.flatnonzero(packed != want_packed)
        raise AssertionError(f"{at.size} packed bytes differ, the first at {int(at[0])} of {dev.cap} + 64")
    if m == 0:
        assert np.all(recs == M.REC_SENTINEL)
    return want_recs


def run(ctx, case, stride, **kw):
    import torch

    dev = DevPack(ctx, case, stride, **kw)
    torch.cuda.synchronize()
    return check(dev, case, stride)


@functools.lru_cache(maxsize=None)
def big_arena():
    """70 001 slots of 1536 random bytes, made once for the tests that need them."""
    return M.arena_of(0x70001, 70001, 1536)


@pytest.mark.parametrize("stride", (1536, 1388))
def test_edges(ctx, stride):
    """Stride 1536 takes the 16-byte path, 1388 the dword path."""
    recs = run(ctx, M.edge_case(stride), stride)
    assert {0, 1, 11, 12, 13, 1382, stride - 4} <= set(recs[:, 1].tolist())


def test_edges_dword_path_under_a_16_byte_stride(ctx):
    """An arena that is only 4-B aligned sends a stride of 1536 down the dword path."""
    run(ctx, M.edge_case(1536), 1536, arena_shift=4)


def test_all_dropped_all_delivered_and_no_status(ctx):
    arena, lens, peer, status = M.random_batch(0xA11, 700, 1536)
    assert len(run(ctx, (arena, lens, peer, np.zeros(700, np.uint8)), 1536)) == 0  # m == 0: nothing written
    assert len(run(ctx, (arena, np.full(700, 1533, np.uint32), peer, None), 1536)) == 0  # none fits its slot
    assert len(run(ctx, (arena, lens, peer, np.ones(700, np.uint8)), 1536)) == 700
    assert len(run(ctx, (arena, lens, peer, None), 1536)) == 700
    assert len(run(ctx, (arena, lens, peer, None), 1388)) < 700  # lengths above 1384 are left out


@pytest.mark.parametrize("n", (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1))
def test_around_the_scan_tile(ctx, n):
    run(ctx, M.random_batch(0x711E + n, n, 256, max_len=252, drop=0.3), 256)


def test_the_spine_folds_two_tiles_a_lane(ctx):
    """1026 tiles for the spine's 1024 lanes, in slots of 16 bytes (L <= 12, every record 16 bytes)."""
    n = 1025 * TILE + 45
    recs = run(ctx, M.random_batch(0x5B1AE, n, 16, max_len=13, drop=0.25), 16)
    assert 150000 < len(recs) < 200000


def test_several_workgroups_all_delivered(ctx):
    rng = np.random.default_rng(0x70002)
    lens, peer = rng.integers(0, 1501, 70001).astype(np.uint32), rng.integers(0, 1 << 20, 70001).astype(np.uint32)
    assert len(run(ctx, (big_arena(), lens, peer, np.ones(70001, np.uint8)), 1536)) == 70001


def test_several_workgroups_half_dropped(ctx):
    rng = np.random.default_rng(0x70003)
    lens, peer = rng.integers(0, 1501, 70001).astype(np.uint32), rng.integers(0, 1 << 20, 70001).astype(np.uint32)
    status = (rng.random(70001) < 0.5).astype(np.uint8)
    assert 34000 < len(run(ctx, (big_arena(), lens, peer, status), 1536)) < 36000


@pytest.mark.parametrize("stride", (1536, 1388))
def test_packed_cap_cuts_the_batch(ctx, stride):
    """Caps at a record's start, one byte before its end and exactly at its end: the model's result, off ==
    0xffffffff for the suffix and counts[1] the full need (check() compares both with the model's)."""
    case = M.random_batch(0xCA9 + stride, 600, stride, max_len=stride - 4)
    full = run(ctx, case, stride)
    k = 2 * len(full) // 3
    start, size = int(full[k, 0]), M.rec_bytes(int(full[k, 1]))
    for cap, fitted in ((start, k), (start + size - 1, k), (start + size, k + 1), (0, 0)):
        recs = run(ctx, case, stride, packed_cap=cap)
        assert np.all(recs[:fitted, 0] != M.NO_ROOM) and np.all(recs[fitted:, 0] == M.NO_ROOM)


def test_two_streams_at_once(ctx):
    import torch

    a, b = M.random_batch(61, 4099, 1536), M.random_batch(62, 5000, 1388, max_len=1384, drop=0.4)
    c = (a[0], a[1], a[2], None)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    devs = [DevPack(ctx, a, 1536, stream=s1), DevPack(ctx, b, 1388, stream=s2), DevPack(ctx, c, 512, stream=s2),
            DevPack(ctx, b, 1388, stream=s1, packed_cap=100000)]
    torch.cuda.synchronize()
    for dev, (case, stride) in zip(devs, ((a, 1536), (b, 1388), (c, 512), (b, 1388))):
        check(dev, case, stride)


def test_argument_errors_launch_nothing(ctx):
    import torch

    L = _lib.lib()
    case = M.edge_case(1536)
    dev = DevPack(ctx, case, 1536)
    torch.cuda.synchronize()
    check(dev, case, 1536)
    packed, recs, counts = M.fresh(dev.n, dev.cap + 64)
    d_packed, d_recs = torch.from_numpy(packed).cuda(), torch.from_numpy(recs.view(np.int32).reshape(-1)).cuda()
    d_counts = torch.from_numpy(np.concatenate([counts, counts]).view(np.int64)).cuda()
    ptr = lambda t: int(t.data_ptr())
    good = [ctx.handle, ptr(dev.arena), 1536, dev.n, ptr(dev.lens), ptr(dev.peer), ptr(dev.status), ptr(d_packed), dev.cap,
            ptr(d_recs), ptr(d_counts), ptr(dev.work), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_deliver_pack(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a3=(1 << 31) + 1) == _lib.QGCM_E_ARG
    assert call(a2=1538) == _lib.QGCM_E_ARG and call(a2=0) == _lib.QGCM_E_ARG  # stride no multiple of 4, or none
    assert call(a8=(1 << 32) - 15) == _lib.QGCM_E_ARG                           # off is 32 bits
    for k in (1, 4, 5, 7, 9, 10, 11):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a7=ptr(d_packed) + 4) == _lib.QGCM_E_ARG   # the packed area off its 16-B boundary
    assert call(a9=ptr(d_recs) + 8) == _lib.QGCM_E_ARG     # the table off its 16-B boundary
    assert call(a10=ptr(d_counts) + 4) == _lib.QGCM_E_ARG  # the counts off their 8-B boundary
    assert call(a1=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a4=ptr(dev.lens) + 2) == _lib.QGCM_E_ARG and call(a5=ptr(dev.peer) + 2) == _lib.QGCM_E_ARG
    assert call(a11=ptr(dev.work) + 4) == _lib.QGCM_E_ARG
    torch.cuda.synchronize()
    assert np.all(d_packed.cpu().numpy() == M.SENTINEL) and np.all(d_recs.cpu().numpy().view(np.uint32) == M.REC_SENTINEL)
    assert np.all(d_counts.cpu().numpy().view(np.uint64) == M.COUNT_SENTINEL)
    # n == 0 writes the counts and nothing else; then the good call
    assert call(a3=0, a1=None, a4=None, a5=None, a7=None, a9=None, a11=None, a10=ptr(d_counts) + 16) == 0
    torch.cuda.synchronize()
    assert d_counts.cpu().numpy().view(np.uint64).tolist() == [M.COUNT_SENTINEL] * 2 + [0, 0]
    assert np.all(d_packed.cpu().numpy() == M.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    dev.packed, dev.recs, dev.counts = d_packed, d_recs, d_counts[:2]
    check(dev, case, 1536)


# ---- the packed pipelines ----

class Capture:
    """tests/test_gpu_gro.py's over_the_wire, run as it stands, with what its two pipeline calls were given and
    what they gave recorded on the way: the slots-in call (qgcm_route_chain_open_host) and the coalesced one
    (qgcm_route_chain_open_gro_host), each with the Rx counters it added and with qgcm_deliver_pack_cpu of the
    arena it left."""

    def __init__(self, monkeypatch, c, f, n, open_stride, seed):
        real_slots, real_gro = route.route_chain_open_host, route.route_chain_open_gro_host
        cap = self

        def view(ptr, size):
            return np.ctypeslib.as_array((C.c_uint8 * size).from_address(ptr))

        def counted(call):
            t0, l0 = stats(c, route.RX)
            rc = call()
            t1, l1 = stats(c, route.RX)
            return rc, (t1 - t0, l1 - l0)

        def packed_of(arena, stride, m, lens, peer, status):
            out = np.zeros(M.need(lens, status, stride), np.uint8)
            recs, total = route.deliver_pack_cpu(arena, stride, m, lens, peer, status, out)
            assert total == out.size
            return out, recs.copy()

        def slots(ctx, arena_ptr, stride, m, lens, plugins, peer, status=None):
            cap.stride, cap.m = stride, m
            cap.in_arena, cap.in_lens = view(arena_ptr, m * stride).copy(), lens.copy()
            cap.slots_rc, cap.slots_rx = counted(lambda: real_slots(ctx, arena_ptr, stride, m, lens, plugins, peer, status))
            cap.slots_out = (lens.copy(), peer.copy(), status.copy())
            cap.slots_packed = packed_of(view(arena_ptr, m * stride), stride, m, lens, peer, status)
            return cap.slots_rc

        def gro(ctx, packed, used, bufs, arena_ptr, stride, m, lens, plugins, peer, status=None):
            cap.packed, cap.used, cap.bufs = packed.copy(), used, bufs.copy()
            cap.gro_rc, cap.gro_rx = counted(lambda: real_gro(ctx, packed, used, bufs, arena_ptr, stride, m, lens, plugins,
                                                             peer, status))
            cap.gro_out = (lens.copy(), peer.copy(), status.copy())
            cap.gro_packed = packed_of(view(arena_ptr, m * stride), stride, m, lens, peer, status)
            return cap.gro_rc

        monkeypatch.setattr(route, "route_chain_open_host", slots)
        monkeypatch.setattr(route, "route_chain_open_gro_host", gro)
        try:
            assert G.over_the_wire(c, f, n, open_stride, seed) == self.m
        finally:
            monkeypatch.undo()


def outputs(m):
    return np.full(m, M.REC_SENTINEL, np.uint32), np.full(m, 7, np.uint32), np.full(m, 0xAB, np.uint8)


def same_rx(ctx, before, want):
    t, l = stats(ctx, route.RX)
    assert (t - before[0]).tolist() == want[0].tolist() and np.array_equal(l - before[1], want[1])


def run_gro_packed(c2, cap, bufs, m, out_bytes):
    lens, peer, status = outputs(m)
    out_buf = np.full(out_bytes, M.SENTINEL, np.uint8)
    rc, recs, out = route.route_chain_open_gro_packed_host(c2, cap.packed, cap.used, bufs, cap.stride, m, lens, BOTH, peer,
                                                           status, out_buf)
    return rc, recs, out, out_buf, (lens, peer, status)


def run_slots_packed(c2, cap, first, m, out_bytes):
    arena = cap.in_arena[first * cap.stride:(first + m) * cap.stride].copy()
    lens, (_, peer, status) = cap.in_lens[first:first + m].copy(), outputs(m)
    out_buf = np.full(out_bytes, M.SENTINEL, np.uint8)
    rc, recs, out = route.route_chain_open_packed_host(c2, arena.ctypes.data, cap.stride, m, lens, BOTH, peer, status, out_buf)
    assert np.array_equal(arena, cap.in_arena[first * cap.stride:(first + m) * cap.stride])  # h_arena is never written
    return rc, recs, out, out_buf, (lens, peer, status)


def check_whole(c2, cap, which, rc, recs, out, out_buf, got):
    want_rc, want_rx, want_out, (want_packed, want_recs) = (
        (cap.gro_rc, cap.gro_rx, cap.gro_out, cap.gro_packed) if which == "gro" else
        (cap.slots_rc, cap.slots_rx, cap.slots_out, cap.slots_packed))
    assert rc == want_rc and out.tolist() == [cap.m, len(want_recs), want_packed.size]
    for g, w in zip(got, want_out):
        assert np.array_equal(g, w)
    assert np.array_equal(recs, want_recs)
    assert np.array_equal(out_buf[:want_packed.size], want_packed) and np.all(out_buf[want_packed.size:] == M.SENTINEL)


@pytest.mark.parametrize("f", (0, 1, 2, 3))
def test_packed_pipelines_match_the_existing_ones(monkeypatch, f):
    """A sealed batch with a forged datagram and an unroutable sender in it, over loopback: on a second context
    with the same keys both packed forms give the peers, statuses, lengths, return value and Rx counters of the
    existing calls, and the packed bytes and the table qgcm_deliver_pack_cpu makes of those calls' arenas."""
    c, c2 = G.loop_ctx(f), G.loop_ctx(f)
    try:
        cap = Capture(monkeypatch, c, f, 150, 1472, 0x6A0 + f)
        before = stats(c2, route.RX)
        res = run_gro_packed(c2, cap, cap.bufs, cap.m, cap.gro_packed[0].size + 64)
        check_whole(c2, cap, "gro", *res)
        same_rx(c2, before, cap.gro_rx)
        before = stats(c2, route.RX)
        res = run_slots_packed(c2, cap, 0, cap.m, cap.slots_packed[0].size + 64)
        check_whole(c2, cap, "slots", *res)
        same_rx(c2, before, cap.slots_rx)
    finally:
        c.close()
        c2.close()


@pytest.mark.parametrize("which", ("gro", "slots"))
def test_packed_pipelines_in_two_chunks(monkeypatch, which):
    """Slots of 1 MiB: a chunk holds 256 of them, so the 300 datagrams that cross are opened in two chunks and the
    second chunk's records are rebased (off by the first chunk's bytes, slot by its packets).  Then an h_out that
    holds the first chunk only: QGCM_E_NOMEM with the first chunk done (256 packets for the slots-in form; for the
    coalesced form the chunk ends at the last buffer boundary at or below 256) and accounted alone; a second call
    on the remainder completes, and both calls together give the one call's result."""
    ctxs = [G.loop_ctx(3) for _ in range(4)]
    c, c2, c3, c4 = ctxs
    try:
        cap = Capture(monkeypatch, c, 3, 450, 1 << 20, 0x2C4)
        m = cap.m
        assert m > 256
        want_packed, want_recs = cap.gro_packed if which == "gro" else cap.slots_packed
        want_rc, want_rx = (cap.gro_rc, cap.gro_rx) if which == "gro" else (cap.slots_rc, cap.slots_rx)
        assert int(want_recs[-1, 2]) >= 256 and np.all(np.diff(want_recs[:, 0].astype(np.int64)) > 0)
        before = stats(c2, route.RX)
        res = (run_gro_packed(c2, cap, cap.bufs, m, want_packed.size) if which == "gro" else
               run_slots_packed(c2, cap, 0, m, want_packed.size))
        check_whole(c2, cap, which, *res)
        same_rx(c2, before, want_rx)

        # the first chunk: whole buffers while they fit 256 slots
        if which == "gro":
            ends = cap.bufs[:, 3].astype(np.int64) + [G.M.count(int(b[1]), int(b[2])) for b in cap.bufs]
            nb1 = int(np.sum(ends <= 256))
            first = int(ends[nb1 - 1])
            assert first == 256 or int(ends[nb1]) > 256
        else:
            first = 256
        k1 = int(np.sum(want_recs[:, 2] < first))
        fill1 = int(want_recs[k1, 0])
        # what the first chunk alone adds to the counters: the existing call on it, on a context of its own
        lens4, peer4, status4 = outputs(first)
        before = stats(c4, route.RX)
        arena4 = np.empty(first << 20, np.uint8)
        if which == "gro":
            rc4 = route.route_chain_open_gro_host(c4, cap.packed, cap.used, cap.bufs[:nb1], arena4.ctypes.data, 1 << 20,
                                                  first, lens4, BOTH, peer4, status4)
        else:
            arena4[:] = cap.in_arena[:first << 20]
            lens4[:] = cap.in_lens[:first]
            rc4 = route.route_chain_open_host(c4, arena4.ctypes.data, 1 << 20, first, lens4, BOTH, peer4, status4)
        t, l = stats(c4, route.RX)
        first_rx = (t - before[0], l - before[1])
        del arena4

        before = stats(c3, route.RX)
        room = want_packed.size - 16  # one record short of the second chunk's need
        rc, recs, out, out_buf, got = (run_gro_packed(c3, cap, cap.bufs, m, room) if which == "gro" else
                                       run_slots_packed(c3, cap, 0, m, room))
        assert rc == _lib.QGCM_E_NOMEM and out.tolist() == [first, k1, fill1]
        same_rx(c3, before, first_rx)
        assert np.array_equal(recs, want_recs[:k1]) and np.array_equal(out_buf[:fill1], want_packed[:fill1])
        assert np.all(out_buf[fill1:] == M.SENTINEL)
        for g, w in zip(got, (lens4, peer4, status4)):
            assert np.array_equal(g[:first], w)
        # the remainder, from the chunk's first packet (the coalesced form: its first buffer, the table rebased)
        if which == "gro":
            rest = cap.bufs[nb1:].copy()
            rest[:, 3] -= first
            rc_b, recs_b, out_b, buf_b, got_b = run_gro_packed(c3, cap, rest, m - first, want_packed.size - fill1)
        else:
            rc_b, recs_b, out_b, buf_b, got_b = run_slots_packed(c3, cap, first, m - first, want_packed.size - fill1)
        assert rc_b >= 0 and rc4 + rc_b == want_rc
        assert out_b.tolist() == [m - first, len(want_recs) - k1, want_packed.size - fill1]
        same_rx(c3, before, want_rx)  # both calls together
        assert np.array_equal(buf_b, want_packed[fill1:])
        moved = recs_b.astype(np.int64) + [fill1, 0, first, 0]
        assert np.array_equal(moved, want_recs[k1:])
        want_out = cap.gro_out if which == "gro" else cap.slots_out
        for g, gb, w in zip(got, got_b, want_out):
            assert np.array_equal(np.concatenate([g[:first], gb]), w)
    finally:
        for x in ctxs:
            x.close()
