"""GPU: qgcm_deliver_coalesce (quantum_amd/csrc/coalesce_kernels.hip) writes exactly what tests/coalesce_model.py
writes -- the packed area whole, over sentinels and inside sentinel margins, the table and the counts -- and the two
coalesced pipelines give the model applied chunk by chunk to what the existing pipeline opens.

Classify and copy give 16 lanes to a slot, 4 slots to a wave and 16 to a workgroup, and their grids stop at 4096
workgroups (65 536 slots a pass); the scans work in tiles of 256 slots.  The mixed batch has runs across slots
63/64 and 255/256."""
import functools

import numpy as np
import pytest

import coalesce_cases as K
import coalesce_model as M
import test_gpu_gro as G
from quantum_amd import _lib, route
from test_gpu_chain_route import BOTH, addr

pytestmark = pytest.mark.gpu

S = K.SENTINEL
MARGIN = 64


def area(n, stride):
    return n * (((stride + 15) & ~15) + 16)


class DevCoalesce:
    """One qgcm_deliver_coalesce call enqueued on `stream` over sentinel-filled outputs; read() after a synchronize."""

    def __init__(self, ctx, case, stride, packed_cap=None, stream=None, arena_shift=0):
        import torch

        arena, lens, peer, status = case
        self.n = n = len(lens)
        self.cap = area(n, stride) if packed_cap is None else packed_cap
        self.whole = torch.empty(arena.size + arena_shift, dtype=torch.uint8, device="cuda")
        self.arena = self.whole[arena_shift:]
        self.arena.copy_(torch.from_numpy(arena))
        self.lens = torch.from_numpy(lens.view(np.int32)).cuda()
        self.peer = torch.from_numpy(peer.view(np.int32)).cuda()
        self.status = None if status is None else torch.from_numpy(status).cuda()
        self.packed = torch.full((self.cap + MARGIN,), S, dtype=torch.uint8, device="cuda")
        self.frames = torch.full((32 * (n + 2),), S, dtype=torch.uint8, device="cuda")
        self.counts = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        self.work = route.deliver_coalesce_work(n)
        self.work.fill_(0xEE)  # the scans take nothing for zero
        torch.cuda.synchronize()  # the inputs are there whatever stream coalesces
        route.deliver_coalesce(ctx, self.arena, stride, n, self.lens, self.peer, self.status, self.packed, self.cap,
                               self.frames, self.counts, self.work, stream)

    def read(self):
        return (self.packed.cpu().numpy(), self.frames.cpu().numpy().view(M.GSO_FRAME),
                self.counts.cpu().numpy().view(np.uint64))


def check(dev, case, stride):
    arena, lens, peer, status = case
    want_packed, want_frames, want_counts = M.coalesce(arena, stride, dev.n, lens, peer, status,
                                                       np.full(dev.cap + MARGIN, S, np.uint8), dev.cap)
    packed, frames, counts = dev.read()
    assert counts.tolist() == want_counts.tolist()
    k = len(want_frames)
    bad = np.flatnonzero(frames[:k] != want_frames)
    assert bad.size == 0, [(int(j), frames[j].tolist(), want_frames[j].tolist()) for j in bad[:8]]
    assert np.all(frames[dev.n:].view(np.uint8) == S)  # nothing past entry n of the table
    if not np.array_equal(packed, want_packed):
        at = np.flatnonzero(packed != want_packed)
        raise AssertionError(f"{at.size} packed bytes differ, the first at {int(at[0])} of {dev.cap} + {MARGIN}")
    return packed, want_frames, counts


def run(ctx, case, stride, **kw):
    import torch

    dev = DevCoalesce(ctx, case, stride, **kw)
    torch.cuda.synchronize()
    return check(dev, case, stride)


@functools.lru_cache(maxsize=None)
def mixed(stride):
    return K.mixed(stride)


@pytest.mark.parametrize("stride,shift", ((1536, 0), (1388, 0), (1536, 4)))
def test_mixed_batch(ctx, stride, shift):
    """(a) Stride 1536 takes the 16-byte path; 1388, and 1536 under an arena that is only 4-B aligned, the dword path."""
    case = mixed(stride)
    n = len(case[1])
    assert n > 2048 and n % 256 != 0
    packed, frames, counts = run(ctx, case, stride, arena_shift=shift)
    assert counts[2] > 50 and (frames["count"] == 64).any() and (frames["count"] == 59).sum() == 2
    heads = frames["first"][frames["kind"] == M.TCP4].astype(np.int64)
    ends = heads + frames["count"][frames["kind"] == M.TCP4]
    for edge in (64, 256):  # a frame with members on both sides of the wave's and the tile's edge
        assert ((heads < edge) & (ends > edge)).any()
    assert len(set((frames["gso_size"][frames["kind"] == M.TCP4] % 16).tolist())) == 16
    # NULL status, and the round trip through the parent's host segmentation
    run(ctx, case[:3] + (None,), stride, arena_shift=shift)
    delivered = np.flatnonzero((case[3] == 1) & (4 + case[1].astype(np.int64) <= stride))
    t = frames.copy()
    t["first"], t["reserved"] = np.cumsum(t["count"]) - t["count"], 0
    back, blens = np.zeros(len(delivered) * stride, np.uint8), np.zeros(len(delivered), np.uint32)
    route.gso_unpack_cpu(packed, int(counts[1]), t, len(delivered), back, stride, blens)
    assert np.array_equal(blens, case[1][delivered])
    live = np.arange(stride - 4)[None, :] < blens[:, None]
    assert np.array_equal(np.where(live, back.reshape(-1, stride)[:, 4:], 0),
                          np.where(live, case[0].reshape(-1, stride)[delivered, 4:], 0))


@pytest.mark.parametrize("stride", (128, 144))
def test_small_slots(ctx, stride):
    """Headers of up to 120 bytes in slots that hold little else, on both paths (144 is a multiple of 16, 128 + 4 is not)."""
    run(ctx, K.mixed(stride), stride)
    run(ctx, K.mixed(stride + 4, seed=9), stride + 4)


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 513))
def test_around_the_scan_tile(ctx, n):
    run(ctx, K.trains(n, 128, (1, 60), 7, seed=n, drop=0.1), 128)
    run(ctx, K.trains(n, 128, 33, 300, seed=n), 128)  # one stretch over every tile, cut at 64


@pytest.mark.parametrize("stride", (1536, 1388))
def test_packed_cap_cuts_inside_a_frame(ctx, stride):
    """(b) Caps at a region's start, inside its lead, inside its packet, one byte before its end and at its end."""
    case = mixed(stride)
    _, full, _ = run(ctx, case, stride)
    k = int(np.flatnonzero(full["count"] == 59)[0])  # a frame of 64 940 bytes in the middle of the batch
    start, size = int(full["off"][k]) - 16, 16 + ((int(full["len"][k]) + 15) & ~15)
    for cap, fitted in ((start, k), (start + 8, k), (start + 700, k), (start + size - 1, k), (start + size, k + 1), (0, 0), (15, 0)):
        _, frames, _ = run(ctx, case, stride, packed_cap=cap)
        assert np.all(frames["off"][:fitted] != M.NO_ROOM) and np.all(frames["off"][fitted:] == M.NO_ROOM)


def test_grid_stride_loop(ctx):
    """(c) 2^19 + 4099 slots of 128 bytes holding 64..100-byte segments: more than the grids take in one pass."""
    n = (1 << 19) + 4099
    case = K.trains(n, 128, (24, 60), 45, seed=19, drop=0.02)
    _, frames, counts = run(ctx, case, 128)
    assert counts[3] > 500000 and counts[2] > 10000 and frames["count"].max() == 45


def test_two_streams_at_once_and_two_runs_alike(ctx):
    """(d), (e) Calls on two streams share nothing; the same input twice gives the same bytes (one writer a byte)."""
    import torch

    a, b = mixed(1536), K.trains(5000, 1388, (1, 1300), 9, seed=2, drop=0.3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    devs = [DevCoalesce(ctx, a, 1536, stream=s1), DevCoalesce(ctx, b, 1388, stream=s2), DevCoalesce(ctx, a, 1536, stream=s2),
            DevCoalesce(ctx, b, 1388, stream=s1, packed_cap=100000)]
    torch.cuda.synchronize()
    for dev, (case, stride) in zip(devs, ((a, 1536), (b, 1388), (a, 1536), (b, 1388))):
        check(dev, case, stride)
    x, y = devs[0].read(), devs[2].read()
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


def test_argument_errors_launch_nothing(ctx):
    """(f)"""
    import torch

    L = _lib.lib()
    case = mixed(1536)
    dev = DevCoalesce(ctx, case, 1536)
    torch.cuda.synchronize()
    check(dev, case, 1536)
    d_packed = torch.full((dev.cap + MARGIN,), S, dtype=torch.uint8, device="cuda")
    d_frames = torch.full((32 * (dev.n + 2),), S, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    ptr = lambda t: int(t.data_ptr())
    good = [ctx.handle, ptr(dev.arena), 1536, dev.n, ptr(dev.lens), ptr(dev.peer), ptr(dev.status), ptr(d_packed), dev.cap,
            ptr(d_frames), ptr(d_counts), ptr(dev.work), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_deliver_coalesce(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a3=(1 << 31) + 1) == _lib.QGCM_E_ARG
    assert call(a2=1538) == _lib.QGCM_E_ARG and call(a2=0) == _lib.QGCM_E_ARG
    assert call(a8=(1 << 32) - 15) == _lib.QGCM_E_ARG
    for k in (1, 4, 5, 7, 9, 10, 11):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a7=ptr(d_packed) + 4) == _lib.QGCM_E_ARG and call(a9=ptr(d_frames) + 8) == _lib.QGCM_E_ARG
    assert call(a10=ptr(d_counts) + 4) == _lib.QGCM_E_ARG and call(a1=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a4=ptr(dev.lens) + 2) == _lib.QGCM_E_ARG and call(a5=ptr(dev.peer) + 2) == _lib.QGCM_E_ARG
    assert call(a11=ptr(dev.work) + 4) == _lib.QGCM_E_ARG
    torch.cuda.synchronize()
    assert bool((d_packed == S).all()) and bool((d_frames == S).all()) and bool((d_counts == -1).all())
    # n == 0 writes the counts and nothing else; then the good call
    assert call(a3=0, a1=None, a4=None, a5=None, a7=None, a9=None, a11=None, a10=ptr(d_counts) + 32) == 0
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [-1] * 4 + [0] * 4 and bool((d_packed == S).all())
    assert call() == 0
    torch.cuda.synchronize()
    dev.packed, dev.frames, dev.counts = d_packed, d_frames, d_counts[:4]
    check(dev, case, 1536)


# ---- the coalesced pipelines ----

def sealed_tcp(c, n, seed, segs=45):
    """n TCP segments in `segs`-segment trains to the peer of flags 3, sealed by qgcm_route_chain_seal_host at stride
    1472; one datagram forged."""
    stride = 1472
    rng = np.random.default_rng(seed)
    f = M.fields(n)
    k = np.arange(n)
    train, at = k // segs, k % segs
    f["P"][:] = 1300
    f["seq"] = (9 + 70001 * train + at * 1300) & 0xFFFFFFFF
    f["id"] = (train * 7 + at) & 0xFFFF
    f["sport"] = 2000 + train % 30000
    f["dst"][:] = int.from_bytes(addr(3).to_bytes(4, "little"), "big")
    slots, lens = M.build(f, stride, rng)
    peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    route.route_chain_seal_host(c, slots.ctypes.data, stride, n, lens, nonces.ctypes.data, BOTH, peer, status)
    assert (status == 1).all()
    slots[(n // 3) * stride + 50] ^= 1
    return slots, lens


@pytest.mark.parametrize("n", (300, 65536 + 348))
def test_coalesced_pipelines_match_the_model_chunk_by_chunk(n):
    """(g) One chunk, and two: 65 536 is no multiple of the trains' 45 segments, so a run straddles the chunk edge and
    comes out as two entries."""
    stride, chunk = 1472, 65536
    c = G.loop_ctx(3)
    try:
        sealed, dlens = sealed_tcp(c, n, 0xC0A + n)
        ref, lens, peer, status = sealed.copy(), dlens.copy(), np.zeros(n, np.uint32), np.full(n, 0xAB, np.uint8)
        dropped = route.route_chain_open_host(c, ref.ctypes.data, stride, n, lens, BOTH, peer, status)
        assert dropped == 1 and status.sum() == n - 1 and (lens[status == 1] == 1340).all()
        want_area, want_frames, want = M.coalesce_chunks(ref, stride, n, lens, peer, status, chunk)
        assert want[2] >= n // 45 and want[3] == n - 1
        if n > chunk:
            j = int(np.flatnonzero(want_frames["first"] == chunk)[0])
            assert want_frames["count"][j - 1] == chunk % 45 and want_frames["count"][j] == 45 - chunk % 45

        def outputs():
            return dlens.copy(), np.full(n, 7, np.uint32), np.full(n, 0xAB, np.uint8)

        def check_out(rc, frames, out, out_buf, got):
            assert rc == dropped and out.tolist() == [n] + want[:2].tolist() + want[2:].tolist()
            assert np.array_equal(frames, want_frames)
            assert np.array_equal(out_buf[:want_area.size], want_area) and np.all(out_buf[want_area.size:] == S)
            for g, w in zip(got, (lens, peer, status)):
                assert np.array_equal(g, w)

        # the slots-in form
        arena, got = sealed.copy(), outputs()
        out_buf = np.full(want_area.size + 64, S, np.uint8)
        rc, frames, out = route.route_chain_open_coalesced_host(c, arena.ctypes.data, stride, n, got[0], BOTH, got[1], got[2], out_buf)
        assert np.array_equal(arena, sealed)  # h_arena is never written
        check_out(rc, frames, out, out_buf, got)
        # the coalesced-receive form: every datagram a buffer of its own, so the chunks are the same
        size = ((dlens.astype(np.int64) + 15) & ~15)
        offs = np.cumsum(size) - size
        packed = np.zeros(int(size.sum()), np.uint8)
        rows = sealed.reshape(n, stride)
        for L in np.unique(dlens):
            sel = np.flatnonzero(dlens == L)
            packed[(offs[sel][:, None] + np.arange(L)[None, :]).reshape(-1)] = rows[sel, :L].reshape(-1)
        bufs = np.stack([offs, dlens, dlens, np.arange(n)], axis=1).astype(np.uint32)
        got, out_buf = outputs(), np.full(want_area.size + 64, S, np.uint8)
        got[0][:] = 0xEEEEEEEE
        rc, frames, out = route.route_chain_open_gro_coalesced_host(c, packed, packed.size, bufs, stride, n, got[0], BOTH, got[1],
                                                                    got[2], out_buf)
        check_out(rc, frames, out, out_buf, got)
        # an h_out one region short: QGCM_E_NOMEM before the last chunk, nothing of it written
        small = np.full(want_area.size - 16, S, np.uint8)
        arena, got = sealed.copy(), outputs()
        rc, frames, out = route.route_chain_open_coalesced_host(c, arena.ctypes.data, stride, n, got[0], BOTH, got[1], got[2], small)
        assert rc == _lib.QGCM_E_NOMEM
        first = (n - 1) // chunk * chunk
        k1 = int((want_frames["first"] < first).sum())
        fill1 = int(want_frames["off"][k1]) - 16
        assert out.tolist()[:3] == [first, k1, fill1] and np.array_equal(frames, want_frames[:k1])
        assert np.array_equal(small[:fill1], want_area[:fill1]) and np.all(small[fill1:] == S)
    finally:
        c.close()
