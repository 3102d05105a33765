"""GPU: qgcm_gso_resolve (quantum_amd/csrc/gso_kernels.hip) leaves exactly what tests/gso_model.py leaves -- the
arena whole inside sentinel margins on both sides, and lens, peer and descs whole with sentinel entries behind
them, all pre-filled with sentinels, so slot tails, the headers of missed packets, the slots of void entries and
the slots no entry names are proven untouched -- and exactly what qgcm_frames_resolve leaves for the model's
packets laid out as frames; and qgcm_route_chain_seal_gso_host gives what qgcm_route_chain_seal_frames_host gives
for the packets qgcm_gso_unpack_cpu makes.

A wave resolves 64 slots with one lane each and then copies them with 16 lanes each; a workgroup is four waves and
the grid stops at 2048 workgroups, so a pass takes 524 288 slots: the batch of 524 288 + 4 099 makes the grid-stride
loop run."""
import numpy as np
import pytest

import frames_model as FM
import gso_model as M
from quantum_amd import _lib, route
from route_model import NO_PEER
from test_gpu_chain_route import BOTH, MAX_KEYS, STRANGER, addr, le
from test_gpu_frames import MARGIN, NETS, finish, padded, same
from test_gpu_gro import loop_ctx

pytestmark = pytest.mark.gpu

TAIL = 16  # sentinel entries behind lens, peer and descs
OUTSIDE = le("8.8.8.8")
DSTS = (addr(3), STRANGER, OUTSIDE)  # an in-net hit, an in-net miss, out of the net: the gateway, mapped or not


@pytest.fixture(scope="module")
def nets():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quantum_amd.crypto import Context

    made = {}
    for name, net in NETS.items():
        c = Context(device=0, max_keys=MAX_KEYS)
        route.routes_set(c, net.table, net.net, net.mask, net.gateway, net.own_ip)
        made[name] = (c, net)
    yield made
    for c, _ in made.values():
        c.close()


def fresh(n, stride):
    """FM.fresh with TAIL sentinel entries behind lens, peer and descs."""
    arena, _, _, _ = FM.fresh(n, stride)
    _, lens, peer, descs = FM.fresh(n + TAIL, 4)
    return arena, lens, peer, descs


class DevGso:
    """One qgcm_gso_resolve call enqueued on `stream` over sentinel-filled outputs; read() after a synchronize."""

    def __init__(self, ctx, packed, packed_len, frames, n, stride, stream=None, arena_shift=0):
        import torch

        self.n, self.stride, self.shift = n, stride, arena_shift
        self.packed = torch.from_numpy(padded(packed)).cuda()
        table = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
        self.frames = torch.from_numpy(np.concatenate([table, np.zeros(32, np.uint8)])).cuda()
        arena, lens, peer, descs = fresh(n, stride)
        self.whole = torch.full((MARGIN + arena_shift + arena.size + MARGIN,), M.SENTINEL, dtype=torch.uint8, device="cuda")
        self.arena = self.whole[MARGIN + arena_shift:]
        self.lens = torch.from_numpy(lens.view(np.int32)).cuda()
        self.peer = torch.from_numpy(peer.view(np.int32)).cuda()
        self.descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()  # the inputs are there whatever stream resolves
        route.gso_resolve(ctx, self.packed, packed_len, self.frames, len(frames), n, self.arena, stride, self.lens, self.peer,
                          self.descs, stream)

    def read(self):
        return (self.whole.cpu().numpy(), self.lens.cpu().numpy().view(np.uint32), self.peer.cpu().numpy().view(np.uint32),
                self.descs.cpu().numpy().view(M.DESC))


def check(dev, net, packed, packed_len, frames, n):
    stride = dev.stride
    arena, lens, peer, descs = fresh(n, stride)
    M.gso_resolve(net, packed, packed_len, frames, n, arena, stride, lens, peer, descs)
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
        raise AssertionError(f"{at.size} bytes differ, the first in slot {int(at[0]) // stride} at byte {int(at[0]) % stride}")
    return lens[:n], peer[:n]


def run(ctx, net, case, stride, **kw):
    import torch

    dev = DevGso(ctx, *case, stride, **kw)
    torch.cuda.synchronize()
    return check(dev, net, *case)


# ---- 1. every shape that can go wrong, in one table ----

GSO_SIZES = (1, 3, 4, 15, 16, 17, 1347, 1348, 1448)


def edge_items(seed=0x6E0):
    rng = np.random.default_rng(seed)
    items, d = [], 0

    def dst():
        nonlocal d
        d += 1
        return DSTS[d % 3]

    # every gso_size with every last-segment payload, id and sequence number wrapping inside the frame
    for gso in GSO_SIZES:
        for tail in sorted({1, 2, 3, gso - 1, gso} - {0}):
            items.append(M.tcp_frame(rng, 2 * gso + tail, gso, dst(), ident=0xFFFE, seq=0xFFFFFFFF - gso))
    # every header length: 40, 44 (IHL 6), 52, 100, the longest (60 + 60) and UDP's 28; 1448 under 100 and 120 bytes
    # of header is clamped at stride - 4, under 60 bytes it fits the slot but not the sealed datagram
    for ihl, tcp_hl in ((20, 20), (24, 20), (20, 32), (40, 60), (60, 60), (20, 40)):
        items.append(M.tcp_frame(rng, 3 * 1448 + 77, 1448, dst(), ihl=ihl, tcp_hl=tcp_hl))
        items.append(M.tcp_frame(rng, 2 * 1348 + 1, 1348, dst(), ihl=ihl, tcp_hl=tcp_hl))
    for gso in (1, 17, 1347, 1472):
        items.append(M.udp_frame(rng, 2 * gso + (gso + 1) // 2, gso, dst()))
    # a wave's edge
    for count in (1, 2, 63, 64, 65):
        items.append(M.tcp_frame(rng, 24 * count - 5, 24, dst()))
        items.append(M.udp_frame(rng, 31 * count - 30, 31, dst(), ihl=24, ident=0xFFF0))
    from test_gso_model import udp_zero_checksum_item

    items.append(udp_zero_checksum_item())
    for tcp in (True, False):
        for L in (0, 1, 2, 3, 100, 1349, 1500, 3000):
            items.append(M.csum_packet(rng, L, dst(), tcp, ihl=24 if L == 100 else 20))
    for L in (0, 1, 19, 20, 21, 64, 1350, 1504, 1505, 1532, 1533, 3000):
        items.append(M.plain_packet(rng, L, dst()))
    items.append(M.tcp_frame(rng, M.SEGS * 5 - 2, 5, addr(3)))  # QGCM_GSO_SEGS segments
    return items


@pytest.fixture(scope="module")
def edges():
    return M.layout(edge_items(), 2, slot_gaps=True)


@pytest.mark.parametrize("stride,shift", ((1536, 0), (1388, 0), (1536, 4)))
def test_edges(nets, edges, stride, shift):
    """Stride 1536 takes the 16-byte path, 1388 the dword path, and an arena 4 bytes off its 16-B boundary sends
    stride 1536 down the dword path.  The table leaves slots out (gaps in `first`): they keep every sentinel."""
    packed, packed_len, frames, n = edges
    assert all(M.valid(f, packed_len, n) for f in frames) and int(frames["count"].sum()) < n
    for name, (c, net) in nets.items():
        lens, peer = run(c, net, edges, stride, arena_shift=shift)
        named = lens != M.LEN_SENTINEL
        assert named.sum() == int(frames["count"].sum())
        hits = lens[named & (peer != NO_PEER)]
        assert hits.size > 1000 and hits.max() <= stride - 32 and hits.min() >= 20
        assert (lens[named] > stride - 4).any() and ((lens[named] > stride - 32) & (lens[named] <= stride - 4)).any()
        assert (18 in peer.tolist()) == (name == "gateway") and 3 in peer.tolist()


# ---- 2. void entries ----

def void_case():
    """Valid entries with one void entry for every rule of the header between them."""
    rng = np.random.default_rng(0x701D)
    T = lambda: M.tcp_frame(rng, 3 * 100 + 7, 100, addr(3))
    U = lambda: M.udp_frame(rng, 3 * 100 + 7, 100, addr(3))
    Cs = lambda: M.csum_packet(rng, 100, addr(3), True)
    Pl = lambda: M.plain_packet(rng, 100, addr(3))
    rules = [
        (T, lambda f, end: f.__setitem__("off", int(f["off"]) + 4)),
        (Pl, lambda f, end: f.__setitem__("len", end - int(f["off"]) + 1)),
        (Pl, lambda f, end: (f.__setitem__("off", 0xFFFFFFF0), f.__setitem__("len", 0x20))),
        (Pl, lambda f, end: f.__setitem__("kind", 4)),
        (Pl, lambda f, end: f.__setitem__("kind", 0xFFFFFFFF)),
        (Pl, lambda f, end: f.__setitem__("count", 2)),
        (Cs, lambda f, end: f.__setitem__("count", 3)),
        (Cs, lambda f, end: f.__setitem__("l4_off", 21)),
        (Cs, lambda f, end: f.__setitem__("csum_off", 17)),
        (Cs, lambda f, end: f.__setitem__("csum_off", (int(f["len"]) - int(f["l4_off"]) + 1) & ~1)),
        (T, lambda f, end: f.__setitem__("l4_off", 16)),
        (T, lambda f, end: (f.__setitem__("l4_off", 64), f.__setitem__("hdr_len", 84))),
        (T, lambda f, end: (f.__setitem__("l4_off", 22), f.__setitem__("hdr_len", 42))),
        (U, lambda f, end: f.__setitem__("hdr_len", 32)),
        (T, lambda f, end: f.__setitem__("hdr_len", 36)),
        (T, lambda f, end: f.__setitem__("hdr_len", 84)),
        (T, lambda f, end: f.__setitem__("hdr_len", 42)),
        (T, lambda f, end: (f.__setitem__("len", 40), f.__setitem__("count", 1))),
        (U, lambda f, end: f.__setitem__("gso_size", 0)),
        (T, lambda f, end: f.__setitem__("count", 3)),
        (U, lambda f, end: f.__setitem__("count", 5)),
        (T, lambda f, end: (f.__setitem__("gso_size", 1), f.__setitem__("count", 307))),  # right, but first + count > n
        (Pl, lambda f, end: f.__setitem__("first", 1 << 30)),                             # first >= n: nothing at all
        (Pl, lambda f, end: f.__setitem__("count", 0)),                                   # no slot named: nothing at all
    ]
    items = []
    for make, _ in rules:
        items += [make(), Pl(), U()]
    packed, packed_len, frames, n = M.layout(items, 3)
    for i, (_, spoil) in enumerate(rules):
        spoil(frames[3 * i], packed_len)
    n_void = sum(not M.valid(f, packed_len, n) for f in frames)
    assert n_void == len(rules)
    return packed, packed_len, frames, n


@pytest.mark.parametrize("stride", (1536, 1388))
def test_every_void_rule(nets, stride):
    c, net = nets["gateway"]
    case = void_case()
    _, packed_len, frames, n = case
    lens, peer = run(c, net, case, stride)
    firsts = [int(f["first"]) for f in frames if not M.valid(f, packed_len, n)]
    assert sorted(set(lens[firsts[:-2]].tolist())) == [0] and lens[firsts[-1]] == M.LEN_SENTINEL
    assert (lens == M.LEN_SENTINEL).sum() > 20  # the further slots of void entries


def test_a_table_that_does_not_ascend_is_memory_safe(nets, edges):
    """Margins and the entries behind lens, peer and descs keep their sentinels; nothing more is claimed."""
    import torch

    c, _ = nets["gateway"]
    packed, packed_len, frames, n = edges
    rng = np.random.default_rng(0xA5CE)
    for stride in (1536, 1388):
        table = frames[rng.permutation(len(frames))].copy()
        table["first"][::7] = rng.integers(0, 1 << 32, len(table["first"][::7]), dtype=np.uint64).astype(np.uint32)
        dev = DevGso(c, packed, packed_len, table, n, stride)
        torch.cuda.synchronize()
        got, lens, peer, descs = dev.read()
        assert np.all(got[:MARGIN] == M.SENTINEL) and np.all(got[-MARGIN:] == M.SENTINEL)
        assert np.all(lens[n:] == M.LEN_SENTINEL) and np.all(peer[n:] == M.PEER_SENTINEL)
        assert np.all(descs[n:].view(np.uint8) == M.SENTINEL)


# ---- 3. the parent's launch on the same packets ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_equals_frames_resolve_on_the_segmented_packets(nets, stride):
    import torch

    c, net = nets["gateway"]
    packed, packed_len, frames, n = M.layout(edge_items(0x6E1), 4)
    dev = DevGso(c, packed, packed_len, frames, n, stride)
    fp, fp_len, ftable = FM.layout(M.packets(packed, packed_len, frames, n), 5)
    d_packed = torch.from_numpy(padded(fp)).cuda()
    d_table = torch.from_numpy(ftable.view(np.int32).reshape(-1).copy()).cuda()
    arena, lens, peer, descs = fresh(n, stride)
    whole = torch.full((MARGIN + n * stride + MARGIN,), M.SENTINEL, dtype=torch.uint8, device="cuda")
    d_lens, d_peer = torch.from_numpy(lens.view(np.int32)).cuda(), torch.from_numpy(peer.view(np.int32)).cuda()
    d_descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
    route.frames_resolve(c, d_packed, fp_len, d_table, n, whole[MARGIN:], stride, d_lens, d_peer, d_descs)
    torch.cuda.synchronize()
    got, got_lens, got_peer, got_descs = dev.read()
    assert np.array_equal(got, whole.cpu().numpy())
    assert np.array_equal(got_lens, d_lens.cpu().numpy().view(np.uint32))
    assert np.array_equal(got_peer, d_peer.cpu().numpy().view(np.uint32)) and (got_peer[:n] != NO_PEER).sum() > 1000
    assert np.array_equal(got_descs, d_descs.cpu().numpy().view(M.DESC))


# ---- 4. the grid, streams, arguments ----

def small_segments(n_full, extra, seed, peers=(1, 2, 3), gso=24):
    """n_full TCP frames of QGCM_GSO_SEGS segments of 40 + gso bytes and one of `extra` segments."""
    rng = np.random.default_rng(seed)
    dsts = [addr(p) for p in peers] + [STRANGER]
    items = [M.tcp_frame(rng, M.SEGS * gso, gso, dsts[i % len(dsts)], ident=i * 977, seq=i * 0x01010101) for i in range(n_full)]
    if extra:
        items.append(M.tcp_frame(rng, extra * gso - 1, gso, dsts[1]))
    return M.layout(items, seed)


def test_the_grid_stride_loop_wraps(nets):
    """One pass of the grid is 2048 workgroups x 256 slots; 4 099 slots more, 64-byte segments in slots of 96."""
    c, net = nets["gateway"]
    case = small_segments(258, 3, 0x80000)
    assert case[3] == 2048 * 256 + 4099
    lens, peer = run(c, net, case, 96)
    assert set(peer[2048 * 256:].tolist()) == {1, 2} and lens[-1] == 63


def test_a_second_stream(nets):
    import torch

    c, net = nets["no-gateway"]
    case = small_segments(2, 45, 0x5EC0)
    dev = DevGso(c, *case, 128, stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    check(dev, net, *case)


def test_argument_errors_launch_nothing(nets, edges):
    import torch

    from quantum_amd.crypto import Context

    L = _lib.lib()
    c, net = nets["gateway"]
    packed, packed_len, frames, n = edges
    dev = DevGso(c, packed, packed_len, frames[:0], n, 1536)  # n_frames == 0: nothing launched
    ptr = lambda t: int(t.data_ptr())
    d_frames = torch.from_numpy(np.concatenate([frames.view(np.uint8).reshape(-1), np.zeros(32, np.uint8)])).cuda()
    good = [c.handle, ptr(dev.packed), packed_len, ptr(d_frames), len(frames), n, ptr(dev.arena), 1536, ptr(dev.lens),
            ptr(dev.peer), ptr(dev.descs), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_gso_resolve(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a5=(1 << 31) + 1) == _lib.QGCM_E_ARG
    assert call(a4=n + 1) == _lib.QGCM_E_ARG  # more entries than slots
    for k in (1, 3, 6, 8, 9, 10):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a1=ptr(dev.packed) + 8) == _lib.QGCM_E_ARG   # the packed area off its 16-B boundary
    assert call(a3=ptr(d_frames) + 8) == _lib.QGCM_E_ARG     # the table off its 16-B boundary
    assert call(a6=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a8=ptr(dev.lens) + 2) == _lib.QGCM_E_ARG and call(a9=ptr(dev.peer) + 2) == _lib.QGCM_E_ARG
    assert call(a10=ptr(dev.descs) + 8) == _lib.QGCM_E_ARG
    for stride in (0, 4, 1538):
        assert call(a7=stride) == _lib.QGCM_E_ARG, stride
    fresh_ctx = Context(device=0, max_keys=MAX_KEYS)  # no qgcm_routes_set yet
    try:
        assert call(a0=fresh_ctx.handle) == _lib.QGCM_E_ARG
    finally:
        fresh_ctx.close()
    assert call(a5=0, a4=0) == 0
    torch.cuda.synchronize()
    got, lens, peer, descs = dev.read()
    assert np.all(got == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL) and np.all(peer == M.PEER_SENTINEL)
    assert np.all(descs.view(np.uint8) == M.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    check(dev, net, *edges)


# ---- 5. the pipeline ----

def host_segmented(packed, packed_len, frames, n, stride):
    """The packets qgcm_gso_unpack_cpu makes, laid out as the frames qgcm_tun_read_packed would have read."""
    arena, lens = np.zeros(n * stride, np.uint8), np.zeros(n, np.uint32)
    route.gso_unpack_cpu(packed, packed_len, frames, n, arena, stride, lens)
    a2 = arena.reshape(n, stride)
    return FM.layout([a2[i, 4:4 + int(lens[i])] for i in range(n)], 7)


def pipeline(case, stride, out_bytes, seed):
    """qgcm_route_chain_seal_frames_host over the host-segmented packets on one context, the new call on a second
    with the same keys and caller nonces: datagrams, tables, lens, peers, status and Tx counters."""
    packed, packed_len, frames, n = case
    c, c2 = loop_ctx(3), loop_ctx(3)
    try:
        nonces = np.random.default_rng(seed).integers(0, 256, 12 * n, dtype=np.uint8)
        fp, fp_len, ftable = host_segmented(packed, packed_len, frames, n, stride)
        ref_lens = np.full(n, M.LEN_SENTINEL, np.uint32)
        want = finish(c, n, ref_lens, out_bytes, lambda *a: route.route_chain_seal_frames_host(
            c, fp, fp_len, ftable, stride, n, ref_lens, nonces.ctypes.data, BOTH, *a))
        lens = np.full(n, M.LEN_SENTINEL, np.uint32)
        before = packed.copy()
        got = finish(c2, n, lens, out_bytes, lambda *a: route.route_chain_seal_gso_host(
            c2, packed, packed_len, frames, stride, n, lens, nonces.ctypes.data, BOTH, *a))
        assert np.array_equal(packed, before)
        same(got, want)
        return want
    finally:
        c.close()
        c2.close()


def pipeline_items(seed, n_big=0):
    rng = np.random.default_rng(seed)
    dsts = (addr(3), addr(11), addr(7), STRANGER)  # 7 has no key
    items = [M.tcp_frame(rng, M.SEGS * 24, 24, dsts[i % 2]) for i in range(n_big)]
    for i in range(6):
        items.append(M.tcp_frame(rng, 44 * 60 + 13, 60, dsts[i % 4], ihl=20 + 4 * (i % 2)))
        items.append(M.udp_frame(rng, 10 * 50 + 1, 50, dsts[(i + 1) % 4]))
        items.append(M.csum_packet(rng, 70 + i, dsts[i % 4], i % 2 == 0))
        items.append(M.plain_packet(rng, 20 + 9 * i, dsts[(i + 2) % 4]))
    return items


def test_pipeline_matches_the_frames_one():
    want = pipeline(M.layout(pipeline_items(0x91FE), 8), 160, 1 << 17, 0x91FF)
    assert want["out"][0] == 6 * (45 + 11 + 2) and want["out"][3] >= 150 and want["rc"] >= 50


def test_pipeline_in_two_chunks():
    """32 entries of 2048 slots fill a chunk of 65 536 exactly; the rest is a second chunk, as it is for
    qgcm_route_chain_seal_frames_host."""
    case = M.layout(pipeline_items(0x2C80, n_big=32), 9)
    want = pipeline(case, 160, case[3] * 128, 0x2C81)
    assert want["out"][0] == 65536 + 348 and want["out"][3] > 60000


def test_pipeline_refuses_bad_tables_and_null_nonces():
    L = _lib.lib()
    c = loop_ctx(3)
    try:
        packed, packed_len, frames, n = M.layout(pipeline_items(0xBAD7), 10)
        nonces = np.zeros(12 * n, np.uint8)
        void, gap = frames.copy(), frames.copy()
        void[1]["hdr_len"] += 4
        gap["first"][3:] += 1
        lens, peer, status = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint8)
        out_buf, pt, od, out = np.zeros(1 << 17, np.uint8), np.zeros((n + 1, 4), np.uint32), np.zeros(n + 1, np.uint32), np.zeros(4, np.uint64)

        def call(table, m, non):
            return L.qgcm_route_chain_seal_gso_host(c.handle, packed.ctypes.data, packed_len, table.ctypes.data, len(table), 160, m,
                                                    lens.ctypes.data, non, BOTH, None, peer.ctypes.data, status.ctypes.data,
                                                    out_buf.ctypes.data, out_buf.size, pt.ctypes.data, od.ctypes.data, out.ctypes.data)

        assert call(void, n, nonces.ctypes.data) == _lib.QGCM_E_ARG
        assert call(gap, n + 1, nonces.ctypes.data) == _lib.QGCM_E_ARG
        assert call(frames, n - 1, nonces.ctypes.data) == _lib.QGCM_E_ARG
        assert call(frames, n, None) == _lib.QGCM_E_ARG
        assert not out_buf.any() and not status.any()
        assert call(frames, n, nonces.ctypes.data) >= 0 and out[0] == n
    finally:
        c.close()
