"""GPU: qgcm_gro_resolve (quantum_amd/csrc/gro_resolve_kernels.hip) leaves exactly what tests/gro_resolve_model.py
leaves -- the arena whole inside sentinel margins on both sides, and lens, peer and descs whole, all pre-filled with
sentinels, so slot tails and the slots no buffer names are proven untouched -- and exactly what qgcm_gro_unpack +
qgcm_resolve_incoming leave; and the three coalesced-receive pipelines give on a context created under
QGCM_GRO_FUSED=1, which runs the one launch, what they give on one created under QGCM_GRO_FUSED=0, which runs the
pair.

A wave resolves 64 slots with one lane each and then copies them with 16 lanes each; a workgroup is four waves and
the grid stops at 2048 workgroups, so a pass takes 524 288 slots."""
import numpy as np
import pytest

import gro_model as G
import gro_resolve_model as M
from quantum_amd import _lib, route
from route_model import NO_PEER
from test_gpu_chain_route import BOTH, MAX_KEYS, OWN, STRANGER, addr, stats
from test_gpu_deliver_pack import outputs
from test_gpu_frames import DSTS, MARGIN, NETS, OUTSIDE, nets  # noqa: F401 (nets: the fixture)
from test_gpu_gro import loop_ctx, sealed_batch

pytestmark = pytest.mark.gpu

GRID_PASS = 2048 * 256  # kGrrMaxBlocks workgroups x 256 slots


class Dev:
    """One qgcm_gro_resolve call enqueued on `stream` over outputs at their sentinels (`before(arena, lens)` fills
    in what the slots no buffer names hold); read() after a synchronize."""

    def __init__(self, ctx, packed, packed_len, bufs, n, stride, stream=None, arena_shift=0, before=None, launch=True):
        import torch

        assert packed.size % 16 == 0
        self.n, self.stride, self.shift, self.before = n, stride, arena_shift, before
        self.n_bufs = len(bufs)
        table = np.ascontiguousarray(bufs, np.uint32).view(np.int32).reshape(-1)
        self.packed = torch.from_numpy(packed).cuda()
        self.bufs = torch.from_numpy(np.concatenate([table, np.zeros(4, np.int32)])).cuda()  # never NULL
        arena, lens, peer, descs = self.start()
        whole = np.full(MARGIN + arena_shift + arena.size + MARGIN, M.SENTINEL, np.uint8)
        whole[MARGIN + arena_shift:MARGIN + arena_shift + arena.size] = arena
        self.whole = torch.from_numpy(whole).cuda()
        self.arena = self.whole[MARGIN + arena_shift:]
        self.lens = torch.from_numpy(lens.view(np.int32)).cuda()
        self.peer = torch.from_numpy(peer.view(np.int32)).cuda()
        self.descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()  # the inputs are there whatever stream resolves
        if launch:
            route.gro_resolve(ctx, self.packed, packed_len, self.bufs, self.n_bufs, n, self.arena, stride, self.lens,
                              self.peer, self.descs, stream)

    def start(self):
        arena, lens, peer, descs = M.fresh(self.n, self.stride)
        if self.before:
            self.before(arena, lens)
        return arena, lens, peer, descs

    def read(self):
        return (self.whole.cpu().numpy(), self.lens.cpu().numpy().view(np.uint32), self.peer.cpu().numpy().view(np.uint32),
                self.descs.cpu().numpy().view(M.DESC))


def compare(dev, arena, lens, peer, descs):
    want = np.full(MARGIN + dev.shift + arena.size + MARGIN, M.SENTINEL, np.uint8)
    want[MARGIN + dev.shift:MARGIN + dev.shift + arena.size] = arena
    got, got_lens, got_peer, got_descs = dev.read()
    for name, g, w in (("lens", got_lens, lens), ("peer", got_peer, peer)):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, [(int(i), int(g[i]), int(w[i])) for i in bad[:8]])
    bad = np.flatnonzero(got_descs != descs)
    assert bad.size == 0, [(int(i), got_descs[i].tolist(), descs[i].tolist()) for i in bad[:8]]
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want) - MARGIN - dev.shift
        raise AssertionError(f"{at.size} bytes differ, the first in slot {int(at[0]) // dev.stride} at byte {int(at[0]) % dev.stride}")


def check(dev, net, packed, packed_len, bufs, n):
    arena, lens, peer, descs = dev.start()
    M.gro_resolve(net, packed, packed_len, bufs, n, arena, dev.stride, lens, peer, descs)
    compare(dev, arena, lens, peer, descs)
    return lens[:n], peer[:n]


def run(ctx, net, case, stride, **kw):
    import torch

    dev = Dev(ctx, *case, stride, **kw)
    torch.cuda.synchronize()
    return check(dev, net, *case)


def planted(case, seed=0):
    packed, packed_len, bufs, n = case
    return M.plant(packed, bufs, DSTS, seed), packed_len, bufs, n


# ---- 1. edges ----

@pytest.mark.parametrize("stride,shift", ((1536, 0), (1388, 0), (1536, 4)))
def test_edges(nets, stride, shift):
    """gro_model.edge_case with planted senders: 2001 datagrams in 661 buffers, 1425 of them readable and starting
    at every residue of 16 (tests/test_gro_resolve_model.py counts them), the 4-byte ones at residues 13-15 with a
    header that straddles a 16-byte boundary; 480 shorter than 4 bytes, 96 longer than the stride.  Stride 1536
    takes the 16-byte path, 1388 the dword path, and an arena 4 bytes off its 16-B boundary sends stride 1536 down
    the dword path."""
    for name, (c, net) in nets.items():
        case = planted(G.edge_case(stride))
        lens, peer = run(c, net, case, stride, arena_shift=shift)
        hits = {int(l) for l, p in zip(lens, peer) if p != NO_PEER}
        assert hits >= {4, 15, 16, 17, 1382, stride} and max(hits) == stride and min(hits) == 4
        long = lens == stride + 1
        assert long.sum() == 96 and np.all(peer[long] == NO_PEER)
        assert (18 in peer.tolist()) == (name == "gateway") and 3 in peer.tolist()


# ---- 2. unnamed and skipped slots ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_unnamed_and_skipped_slots_are_resolved_from_what_they_held(nets, stride):
    c, net = nets["gateway"]
    packed, packed_len, bufs, n = G.layout([(300, 100, 1), (4146, 1382, 2), (64, 0, 3), (500, 77, 4), (2764, 1382, 5),
                                            (1382, 0, 6), (200, 100, 7)], 21)
    assert bufs[:, 3].tolist() == [0, 3, 6, 7, 14, 16, 17] and n == 19
    bufs[2:, 3] += 2               # a gap in `first`: slots 6 and 7
    bufs[5:, 3] += 3               # and slots 18, 19, 20
    bufs[1, 0] = packed_len - 4145  # one byte past the packed area: slots 3, 4, 5
    bufs[3, 0] = 0xFFFFFFF0        # off + len wraps 32 bits: slots 9 .. 15
    n = 23                         # the last buffer names slots 22 and 23: skipped whole, slot 22 unnamed
    assert [G.skipped(b, packed_len, n) for b in bufs] == [False, True, False, True, False, False, True]
    M.plant(packed, bufs[[0, 2, 4, 5]], DSTS)
    unnamed = [3, 4, 5, 6, 7] + list(range(9, 16)) + [18, 19, 20, 22]
    known = np.frombuffer(addr(5).to_bytes(4, "little"), np.uint8)

    def before(arena, lens):
        for j, i in enumerate(unnamed):  # sentinels, a packet of 64 bytes from peer 5, a packet of 3 bytes
            if j % 3 == 1:
                lens[i] = 64
                arena[i * stride:i * stride + 4] = known
            elif j % 3 == 2:
                lens[i] = 3
                arena[i * stride:i * stride + 4] = known
    lens, peer = run(c, net, (packed, packed_len, bufs, n), stride, before=before)
    assert [int(lens[i]) for i in unnamed] == [(M.LEN_SENTINEL, 64, 3)[j % 3] for j in range(len(unnamed))]
    assert [int(peer[i]) for i in unnamed] == [(NO_PEER, 5, NO_PEER)[j % 3] for j in range(len(unnamed))]
    assert lens[[0, 1, 2, 8, 16, 17, 21]].tolist() == [100, 100, 100, 64, 1382, 1382, 1382]


# ---- 3. counts ----

@pytest.mark.parametrize("n", (1, 15, 16, 17, 63, 64, 65, 257))
def test_counts(nets, n):
    """Across the 16-lane group, the wave and the workgroup, on both paths."""
    c, net = nets["gateway"]
    run(c, net, planted(G.random_batch(0xC00 + n, n), n), 1536)
    run(c, net, planted(G.random_batch(0xD00 + n, n), n + 1), 1388)


# ---- 4. no table ----

def test_without_a_table_it_is_resolve_incoming(nets):
    import torch

    c, net = nets["gateway"]
    n, stride = 300, 128
    rng = np.random.default_rng(0x300)
    pick = (0, 3, 4, 64, stride, stride + 1)
    held = np.array(pick, np.uint32)[rng.integers(0, len(pick), n)]
    src = np.array(DSTS, np.uint32)[rng.integers(0, 3, n)]
    fill = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    fill[:, :4] = src.view(np.uint8).reshape(n, 4)

    def before(arena, lens):
        arena[:] = fill.reshape(-1)
        lens[:] = held
    dev = Dev(c, np.zeros(16, np.uint8), 0, np.zeros((0, 4), np.uint32), n, stride, before=before)
    torch.cuda.synchronize()
    lens, peer = check(dev, net, np.zeros(16, np.uint8), 0, np.zeros((0, 4), np.uint32), n)
    assert (peer != NO_PEER).sum() > 50 and np.array_equal(lens, held)
    arena, lens0, peer0, descs0 = dev.start()
    d_arena = torch.from_numpy(arena).cuda()
    d_lens, d_peer = torch.from_numpy(lens0.view(np.int32)).cuda(), torch.from_numpy(peer0.view(np.int32)).cuda()
    d_descs = torch.from_numpy(descs0.view(np.uint8).copy()).cuda()
    route.resolve_incoming(c, d_arena, stride, n, d_lens, d_peer, d_descs)
    torch.cuda.synchronize()
    compare(dev, d_arena.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32), d_peer.cpu().numpy().view(np.uint32),
            d_descs.cpu().numpy().view(M.DESC))


# ---- 5. the grid-stride loop ----

def lone_case(net, n, size, stride, seed):
    """n lone datagrams of `size` bytes (a multiple of 16) back to back, senders cycling through DSTS, and what the
    call leaves of them, computed whole arrays at a time."""
    rng = np.random.default_rng(seed)
    body = rng.integers(0, 256, (n, size), dtype=np.uint8)
    src = np.array(DSTS, np.uint32)[np.arange(n) % 3]
    body[:, :4] = src.view(np.uint8).reshape(n, 4)
    at = np.arange(n, dtype=np.uint32)
    bufs = np.stack([at * size, np.full(n, size, np.uint32), np.zeros(n, np.uint32), at], axis=1)
    arena, lens, peer, descs = M.fresh(n, stride)
    arena.reshape(n, stride)[:, :size] = body
    lens[:] = size
    peer[:] = np.array([M.lookup(net, int(d)) for d in DSTS], np.uint32)[np.arange(n) % 3]
    descs["off"], descs["len"], descs["key"] = np.arange(n, dtype=np.uint64) * stride, size - 4, peer
    return (body.reshape(-1), size * n, bufs, n), (arena, lens, peer, descs)


def test_the_grid_stride_loop_wraps(nets):
    """n = 2048 * 256 + 4099 = 528 387: one pass of the grid (kGrrMaxBlocks = 2048 workgroups of 256 slots) and
    4 099 slots more; lone 32-byte datagrams in slots of 64 bytes.  Then trains on the dword path."""
    import torch

    c, net = nets["gateway"]
    small, want = lone_case(net, 300, 32, 64, 5)  # the whole-array expectation is the model's
    arena, lens, peer, descs = M.fresh(300, 64)
    M.gro_resolve(net, *small, arena, 64, lens, peer, descs)
    for g, w in zip((arena, lens, peer, descs), want):
        assert np.array_equal(g, w)
    n = GRID_PASS + 4099
    case, want = lone_case(net, n, 32, 64, 0x80000)
    dev = Dev(c, *case, 64)
    torch.cuda.synchronize()
    compare(dev, *want)
    assert set(want[2][GRID_PASS:].tolist()) == {3, 18, NO_PEER}
    run(c, net, planted(G.random_batch(0x4099, 4099)), 1388)


# ---- 6. streams ----

def test_two_streams_at_once(nets):
    import torch

    (c1, n1), (c2, n2) = nets["gateway"], nets["no-gateway"]
    a, b = planted(G.random_batch(61, 4099)), planted(G.random_batch(62, 5000, 64), 1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = [(c1, n1, a, 1536, s1), (c2, n2, b, 1388, s2), (c2, n2, a, 1388, s2), (c1, n1, b, 1536, s1)]
    devs = [Dev(c, *case, stride, stream) for c, _, case, stride, stream in jobs]
    torch.cuda.synchronize()
    for dev, (_, net, case, _, _) in zip(devs, jobs):
        check(dev, net, *case)


# ---- 7. argument errors ----

def test_argument_errors_launch_nothing(nets):
    import torch

    from quantum_amd.crypto import Context

    L = _lib.lib()
    c, net = nets["gateway"]
    case = planted(G.layout([(300, 100, 1), (64, 0, 3), (1382, 0, 5)], 12))
    packed, packed_len, bufs, n = case
    dev = Dev(c, *case, 1536, launch=False)
    ptr = lambda t: int(t.data_ptr())
    good = [c.handle, ptr(dev.packed), packed_len, ptr(dev.bufs), len(bufs), n, ptr(dev.arena), 1536, ptr(dev.lens),
            ptr(dev.peer), ptr(dev.descs), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_gro_resolve(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a5=(1 << 31) + 1) == _lib.QGCM_E_ARG
    assert call(a4=n + 1) == _lib.QGCM_E_ARG  # more buffers than datagrams
    for stride in (0, 2, 1538):
        assert call(a7=stride) == _lib.QGCM_E_ARG, stride
    for k in (1, 3, 6, 8, 9, 10):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
        assert call(**{f"a{k}": None}, a4=0) == _lib.QGCM_E_ARG, k  # also without a table
    assert call(a1=ptr(dev.packed) + 8) == _lib.QGCM_E_ARG  # the packed area off its 16-B boundary
    assert call(a3=ptr(dev.bufs) + 8) == _lib.QGCM_E_ARG    # the table off its 16-B boundary
    assert call(a10=ptr(dev.descs) + 8) == _lib.QGCM_E_ARG
    assert call(a6=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a8=ptr(dev.lens) + 2) == _lib.QGCM_E_ARG and call(a9=ptr(dev.peer) + 2) == _lib.QGCM_E_ARG
    fresh_ctx = Context(device=0, max_keys=MAX_KEYS)  # no qgcm_routes_set yet
    try:
        assert call(a0=fresh_ctx.handle) == _lib.QGCM_E_ARG
        assert call(a0=fresh_ctx.handle, a5=0, a4=0) == _lib.QGCM_E_ARG
    finally:
        fresh_ctx.close()
    assert call(a5=0, a4=0) == 0  # n == 0: nothing launched
    torch.cuda.synchronize()
    got, lens, peer, descs = dev.read()
    assert np.all(got == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL) and np.all(peer == M.PEER_SENTINEL)
    assert np.all(descs.view(np.uint8) == M.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    check(dev, net, *case)


# ---- 8. the existing pair on the device ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_equals_gro_unpack_then_resolve_incoming(nets, stride):
    """4096 seeded datagrams in trains: byte-identical arena, lens, peer and descs to qgcm_gro_unpack followed by
    qgcm_resolve_incoming, both from the same sentinel-filled memory."""
    import torch

    c, net = nets["gateway"]
    case = planted(G.random_batch(0xE8, 4096))
    packed, packed_len, bufs, n = case
    dev = Dev(c, *case, stride)
    pair = Dev(c, *case, stride, launch=False)
    route.gro_unpack(c, pair.packed, packed_len, pair.bufs, len(bufs), n, pair.arena, stride, pair.lens)
    route.resolve_incoming(c, pair.arena, stride, n, pair.lens, pair.peer, pair.descs)
    torch.cuda.synchronize()
    got, got_lens, got_peer, got_descs = dev.read()
    want, want_lens, want_peer, want_descs = pair.read()
    assert np.array_equal(got, want) and np.array_equal(got_lens, want_lens)
    assert np.array_equal(got_peer, want_peer) and (got_peer != NO_PEER).sum() > 1000
    assert np.array_equal(got_descs, want_descs)


# ---- 9. the pipelines ----

def ctx_pair(monkeypatch, f):
    """Two contexts with the same keys: (one that runs the pair of launches, one that runs the one launch).  The
    knob is read when a context is created."""
    monkeypatch.setenv("QGCM_GRO_FUSED", "0")
    pair = loop_ctx(f)
    monkeypatch.setenv("QGCM_GRO_FUSED", "1")
    fused = loop_ctx(f)
    monkeypatch.delenv("QGCM_GRO_FUSED")
    return pair, fused


def coalesced(datagrams, seed, train=45):
    """The datagrams (byte arrays) as a receive would leave them: runs of equal length as buffers of up to `train`
    segments, every buffer on a 16-byte boundary -> (packed, packed_len, bufs, n)."""
    specs, runs, i = [], [], 0
    while i < len(datagrams):
        j = i
        while j < len(datagrams) and j - i < train and len(datagrams[j]) == len(datagrams[i]) and len(datagrams[i]) > 0:
            j += 1
        j = max(j, i + 1)
        L = len(datagrams[i])
        specs.append((L * (j - i), L if j - i > 1 else 0, 0))
        runs.append((i, j))
        i = j
    packed, packed_len, bufs, n = G.layout(specs, seed)
    assert n == len(datagrams)
    for (i, j), b in zip(runs, bufs):
        packed[int(b[0]):int(b[0]) + int(b[1])] = np.concatenate([datagrams[k] for k in range(i, j)] or [np.zeros(0, np.uint8)])
    return packed, packed_len, bufs, n


def sealed_datagrams(c, f, n, seed):
    """What crosses the wire of tests/test_gpu_gro.py's sealed batch, in slot order, with one datagram forged and
    one from a sender no route knows."""
    _, slots, lens, _, status = sealed_batch(c, f, n, seed)
    send = np.flatnonzero((status == 1) & (lens != 0))
    assert len(send) >= 100
    grams = [slots[i, :int(lens[i])].copy() for i in send]
    grams[7][40] ^= 1
    grams[19][0:4] = np.frombuffer(STRANGER.to_bytes(4, "little"), np.uint8)
    return grams


def counted(c, call):
    t0, l0 = stats(c, route.RX)
    rc = call()
    t1, l1 = stats(c, route.RX)
    return rc, (t1 - t0).tolist(), l1 - l0


def slots_call(c, case, stride, chain, plugins=BOTH):
    """qgcm_route_open_gro_host / qgcm_route_chain_open_gro_host -> everything the caller can see, the arena as its
    specified ranges: Raw[:4 + h_lens[i]] of a delivered packet, Raw[:datagram length] of a dropped one."""
    packed, packed_len, bufs, n = case
    arena = np.full(n * stride, M.SENTINEL, np.uint8)
    lens, peer, status = outputs(n)
    if chain:
        rc, rx, links = counted(c, lambda: route.route_chain_open_gro_host(c, packed, packed_len, bufs, arena.ctypes.data, stride, n,
                                                                           lens, plugins, peer, status))
    else:
        rc, rx, links = counted(c, lambda: route.route_open_gro_host(c, packed, packed_len, bufs, arena.ctypes.data, stride, n, lens,
                                                                     peer, status))
    dgram = np.zeros(n, np.uint32)
    for b in bufs:
        if int(b[0]) + int(b[1]) <= packed_len:
            for slot, _, L in G.datagrams(b):
                dgram[slot] = L
    rows = arena.reshape(n, stride)
    spec = [rows[i, :min(stride, 4 + int(lens[i]) if status[i] == 1 else int(dgram[i]))].tobytes() for i in range(n)]
    return dict(rc=rc, rx=rx, links=links, lens=lens, peer=peer, status=status, spec=spec)


def packed_call(c, case, stride, out_bytes, plugins=BOTH):
    """qgcm_route_chain_open_gro_packed_host -> everything the caller can see."""
    packed, packed_len, bufs, n = case
    lens, peer, status = outputs(n)
    out_buf = np.full(out_bytes, M.SENTINEL, np.uint8)
    (rc, recs, out), rx, links = counted(c, lambda: route.route_chain_open_gro_packed_host(c, packed, packed_len, bufs, stride, n, lens,
                                                                                         plugins, peer, status, out_buf))
    return dict(rc=rc, rx=rx, links=links, lens=lens, peer=peer, status=status, recs=recs.copy(), out=out.tolist(), buf=out_buf)


def same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), k
        else:
            assert got[k] == want[k], k


def test_open_pipeline_is_unchanged(monkeypatch):
    pair, fused = ctx_pair(monkeypatch, 2)
    try:
        case = coalesced(sealed_datagrams(pair, 2, 150, 0x9A0), 1)
        want, got = slots_call(pair, case, 1472, False), slots_call(fused, case, 1472, False)
        same(got, want)
        assert want["rc"] == 2 and (want["status"] == 1).sum() >= 98 and set(want["peer"].tolist()) == {20, NO_PEER}
    finally:
        pair.close()
        fused.close()


@pytest.mark.parametrize("f", (0, 1, 2, 3))
def test_chain_pipeline_is_unchanged(monkeypatch, f):
    pair, fused = ctx_pair(monkeypatch, f)
    try:
        case = coalesced(sealed_datagrams(pair, f, 150, 0x9B0 + f), 2)
        assert int(case[2][:, 2].max()) > 0  # trains among the buffers
        want, got = slots_call(pair, case, 1472, True), slots_call(fused, case, 1472, True)
        same(got, want)
        assert want["rc"] >= 1 and (want["rc"] == 2 or not f & 2) and (want["status"] == 1).sum() >= 98
    finally:
        pair.close()
        fused.close()


def test_packed_pipeline_in_one_chunk_and_with_a_buffer_past_packed_len(monkeypatch):
    pair, fused = ctx_pair(monkeypatch, 3)
    try:
        case = coalesced(sealed_datagrams(pair, 3, 150, 0x9C0), 3)
        want, got = packed_call(pair, case, 1472, 1 << 18), packed_call(fused, case, 1472, 1 << 18)
        same(got, want)
        assert want["out"][0] == case[3] and want["out"][1] >= 98 and want["rc"] == 2
        # the last buffer one byte past packed_len: its slots are datagrams of length 0
        short = (case[0], case[1] - 1, case[2], case[3])
        want2, got2 = packed_call(pair, short, 1472, 1 << 18), packed_call(fused, short, 1472, 1 << 18)
        same(got2, want2)
        lost = G.count(int(case[2][-1][1]), int(case[2][-1][2]))
        assert want2["out"][1] == want["out"][1] - lost and want2["rc"] == want["rc"] + lost
    finally:
        pair.close()
        fused.close()


def test_packed_pipeline_in_two_chunks(monkeypatch):
    """70 000 lone 64-byte datagrams at stride 128: a chunk of 65 536 and one of 4 464.  Without plugins the chain
    passes every routed datagram through, so the senders decide what is delivered."""
    pair, fused = ctx_pair(monkeypatch, 3)
    try:
        n = 70000
        rng = np.random.default_rng(0x2C9)
        body = rng.integers(0, 256, (n, 64), dtype=np.uint8)
        src = np.array([OWN, STRANGER, OUTSIDE], np.uint32)[rng.integers(0, 3, n)]
        body[:, :4] = src.view(np.uint8).reshape(n, 4)
        at = np.arange(n, dtype=np.uint32)
        bufs = np.stack([at * 64, np.full(n, 64, np.uint32), np.zeros(n, np.uint32), at], axis=1)
        case = (body.reshape(-1), 64 * n, bufs, n)
        want, got = packed_call(pair, case, 128, n * 64, 0), packed_call(fused, case, 128, n * 64, 0)
        same(got, want)
        assert want["out"][0] == n and 20000 < want["out"][1] < 50000
        assert set(want["peer"][65536:].tolist()) == {20, NO_PEER}
    finally:
        pair.close()
        fused.close()
