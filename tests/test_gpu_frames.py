"""GPU: qgcm_frames_resolve (quantum_amd/csrc/frames_kernels.hip) leaves exactly what tests/frames_model.py leaves
-- the arena whole inside sentinel margins on both sides, and lens, peer and descs whole, all pre-filled with
sentinels, so slot tails, the headers of missed packets and the slots of void frames are proven untouched -- and
exactly what qgcm_gro_unpack + qgcm_resolve_outgoing leave; and qgcm_route_chain_seal_frames_host gives what
qgcm_route_chain_seal_packed_host gives for the arena qgcm_frames_unpack_cpu makes of the same input.

A wave resolves 64 frames with one lane each and then copies them with 16 lanes each; a workgroup is four waves
and the grid stops at 2048 workgroups, so a pass takes 524 288 frames: 70 000 frames take 274 workgroups, and the
batch of 524 288 + 4 099 makes the grid-stride loop run."""
import numpy as np
import pytest

import chain_model as CM
import frames_model as M
from quantum_amd import _lib, batch, route
from route_model import NO_PEER
from send_plan_wire import Wire
from test_gpu_chain_route import BOTH, MAX_KEYS, OWN, STRANGER, addr, le, make_ctx, stats
from test_gpu_gro import loop_ctx
from test_gpu_train_pack import SEAL_STRIDE, same_tx, tun_batch

pytestmark = pytest.mark.gpu

MARGIN = 64
GATEWAY, OUTSIDE = le("10.99.7.7"), le("8.8.8.8")
TABLE = {addr(p): p for p in range(17)}
NETS = {"gateway": M.Net({**TABLE, GATEWAY: 18}, le("10.99.0.0"), route.mask_of(16), GATEWAY, OWN),
        "no-gateway": M.Net(TABLE, le("10.99.0.0"), route.mask_of(16), GATEWAY, OWN)}
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


def padded(packed):
    out = np.zeros((packed.size + 15) & ~15, np.uint8)
    out[:packed.size] = packed
    return out


class DevFrames:
    """One qgcm_frames_resolve call enqueued on `stream` over sentinel-filled outputs; read() after a synchronize."""

    def __init__(self, ctx, packed, packed_len, frames, stride, stream=None, arena_shift=0):
        import torch

        self.n, self.stride, self.shift = len(frames), stride, arena_shift
        n = self.n
        self.packed = torch.from_numpy(padded(packed)).cuda()
        self.frames = torch.from_numpy(np.ascontiguousarray(frames, np.uint32).view(np.int32).reshape(-1).copy()).cuda()
        arena, lens, peer, descs = M.fresh(n, stride)
        self.whole = torch.full((MARGIN + arena_shift + arena.size + MARGIN,), M.SENTINEL, dtype=torch.uint8, device="cuda")
        self.arena = self.whole[MARGIN + arena_shift:]
        self.lens = torch.from_numpy(lens.view(np.int32)).cuda()
        self.peer = torch.from_numpy(peer.view(np.int32)).cuda()
        self.descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()  # the inputs are there whatever stream resolves
        route.frames_resolve(ctx, self.packed, packed_len, self.frames, n, self.arena, stride, self.lens, self.peer,
                             self.descs, stream)

    def read(self):
        return (self.whole.cpu().numpy(), self.lens.cpu().numpy().view(np.uint32), self.peer.cpu().numpy().view(np.uint32),
                self.descs.cpu().numpy().view(M.DESC))


def check(dev, net, packed, packed_len, frames):
    n, stride = dev.n, dev.stride
    arena, lens, peer, descs = M.fresh(n, stride)
    M.frames_resolve(net, packed, packed_len, frames, arena, stride, lens, peer, descs)
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
    return lens, peer


def run(ctx, net, case, stride, **kw):
    import torch

    dev = DevFrames(ctx, *case, stride, **kw)
    torch.cuda.synchronize()
    return check(dev, net, *case)


# ---- 1. edges ----

@pytest.mark.parametrize("stride,shift", ((1536, 0), (1388, 0), (1536, 4)))
def test_edges(nets, stride, shift):
    """Every edge length to every kind of destination under both nets.  Stride 1536 takes the 16-byte path, 1388
    the dword path, and an arena 4 bytes off its 16-B boundary sends stride 1536 down the dword path."""
    for name, (c, net) in nets.items():
        case = M.layout(M.edge_packets(stride, DSTS), stride, gaps=True)
        lens, peer = run(c, net, case, stride, arena_shift=shift)
        hits = {int(l) for l, p in zip(lens, peer) if p != NO_PEER}
        assert hits >= {20, 21, 1350, stride - 32} and max(hits) == stride - 32 and min(hits) == 20
        assert (18 in peer.tolist()) == (name == "gateway") and 3 in peer.tolist()


# ---- 2. void frames ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_void_frames_between_valid_ones(nets, stride):
    c, net = nets["gateway"]
    rng = np.random.default_rng(0x701D)
    packets = [M.packet(rng, L, addr(1 + i)) for i, L in enumerate((64, 100, 700, 33, 1350, 20, 257, 64, 77))]
    packed, packed_len, frames = M.layout(packets, 5)
    assert packed_len % 16 == 13 and int(frames[-1, 0]) + int(frames[-1, 1]) == packed_len  # ends exactly at packed_len
    frames[2, 0] += 4                                # off not a multiple of 16
    frames[4, 1] = packed_len - int(frames[4, 0]) + 1  # off + len one past packed_len
    frames[6] = (0xFFFFFFF0, 0x20)                   # off + len wraps 32 bits
    assert [M.valid(int(o), int(l), packed_len) for o, l in frames] == [True, True, False, True, False, True, False, True, True]
    lens, peer = run(c, net, (packed, packed_len, frames), stride)
    assert lens.tolist() == [64, 100, 0, 33, 0, 20, 0, 64, 77] and peer[8] == 9 and peer[2] == NO_PEER


# ---- 3. counts ----

@pytest.mark.parametrize("n", (1, 15, 16, 17, 257))
def test_counts(nets, n):
    c, net = nets["gateway"]
    run(c, net, M.layout(M.random_packets(0xC0 + n, n, DSTS), n, gaps=True), SEAL_STRIDE)
    run(c, net, M.layout(M.random_packets(0xD0 + n, n, DSTS), n), 1388)


def small_frames(n, seed, peers=(1, 2, 3), size=64):
    """n frames of `size` (a multiple of 16) random bytes to keyed-or-not peers, back to back: (packed, packed_len,
    frames)."""
    rng = np.random.default_rng(seed)
    body = rng.integers(0, 256, (n, size), dtype=np.uint8)
    dst = np.array([addr(p) for p in peers] + [STRANGER], np.uint32)[rng.integers(0, len(peers) + 1, n)]
    body[:, 16:20] = dst.view(np.uint8).reshape(n, 4)
    frames = np.stack([np.arange(n, dtype=np.uint32) * size, np.full(n, size, np.uint32)], axis=1)
    return body.reshape(-1), size * n, frames


def test_seventy_thousand_frames(nets):
    c, net = nets["no-gateway"]
    lens, peer = run(c, net, small_frames(70000, 0x70000), 128)
    assert peer[65536:].tolist().count(NO_PEER) > 100 and set(peer[65536:].tolist()) == {1, 2, 3, NO_PEER}


def test_the_grid_stride_loop_wraps(nets):
    """One pass of the grid is 2048 workgroups x 256 frames; 4 099 frames more, 32 bytes each in slots of 64."""
    c, net = nets["gateway"]
    n = 2048 * 256 + 4099
    lens, peer = run(c, net, small_frames(n, 0x80000, size=32), 64)
    assert set(peer[2048 * 256:].tolist()) == {1, 2, 3, NO_PEER}


# ---- 4. streams and errors ----

def test_two_streams_at_once(nets):
    import torch

    (c1, n1), (c2, n2) = nets["gateway"], nets["no-gateway"]
    a = M.layout(M.random_packets(61, 4099, DSTS), 1, gaps=True)
    b = small_frames(5000, 62)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = [(c1, n1, a, 1536, s1), (c2, n2, b, 128, s2), (c2, n2, a, 1388, s2), (c1, n1, b, 64, s1)]
    devs = [DevFrames(c, case[0], case[1], case[2], stride, stream) for c, _, case, stride, stream in jobs]
    torch.cuda.synchronize()
    for dev, (_, net, case, _, _) in zip(devs, jobs):
        check(dev, net, *case)


def test_argument_errors_launch_nothing(nets):
    import torch

    from quantum_amd.crypto import Context

    L = _lib.lib()
    c, net = nets["gateway"]
    case = M.layout(M.random_packets(71, 12, DSTS), 2)
    packed, packed_len, frames = case
    dev = DevFrames(c, packed, packed_len, frames[:0], 1536)  # n == 0: nothing launched
    dev.n = 12
    spare = M.fresh(12, 1536)
    dev.whole = torch.full((MARGIN + spare[0].size + MARGIN,), M.SENTINEL, dtype=torch.uint8, device="cuda")
    dev.arena = dev.whole[MARGIN:]
    dev.lens = torch.from_numpy(spare[1].view(np.int32)).cuda()
    dev.peer = torch.from_numpy(spare[2].view(np.int32)).cuda()
    dev.descs = torch.from_numpy(spare[3].view(np.uint8).copy()).cuda()
    ptr = lambda t: int(t.data_ptr())
    d_frames = torch.from_numpy(np.concatenate([frames.view(np.int32).reshape(-1), np.zeros(2, np.int32)])).cuda()
    good = [c.handle, ptr(dev.packed), packed_len, ptr(d_frames), 12, ptr(dev.arena), 1536, ptr(dev.lens), ptr(dev.peer),
            ptr(dev.descs), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_frames_resolve(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a4=(1 << 31) + 1) == _lib.QGCM_E_ARG
    for k in (1, 3, 5, 7, 8, 9):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a1=ptr(dev.packed) + 8) == _lib.QGCM_E_ARG   # the packed area off its 16-B boundary
    assert call(a3=ptr(d_frames) + 4) == _lib.QGCM_E_ARG     # the table off its 8-B boundary
    assert call(a5=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a7=ptr(dev.lens) + 2) == _lib.QGCM_E_ARG and call(a8=ptr(dev.peer) + 2) == _lib.QGCM_E_ARG
    assert call(a9=ptr(dev.descs) + 8) == _lib.QGCM_E_ARG
    for stride in (0, 4, 1538):
        assert call(a6=stride) == _lib.QGCM_E_ARG, stride
    fresh_ctx = Context(device=0, max_keys=MAX_KEYS)  # no qgcm_routes_set yet
    try:
        assert call(a0=fresh_ctx.handle) == _lib.QGCM_E_ARG
    finally:
        fresh_ctx.close()
    assert call(a4=0) == 0
    torch.cuda.synchronize()
    got, lens, peer, descs = dev.read()
    assert np.all(got == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL) and np.all(peer == M.PEER_SENTINEL)
    assert np.all(descs.view(np.uint8) == M.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    check(dev, net, *case)


# ---- 5. the existing pair on the device ----

@pytest.mark.parametrize("stride", (1536, 1388))
def test_equals_gro_unpack_then_resolve_outgoing(nets, stride):
    """4096 seeded frames: byte-identical arena, lens, peer and descs to qgcm_gro_unpack with a table of lone
    buffers and the destination d_arena + 4, followed by qgcm_resolve_outgoing, from the same sentinel-filled arena."""
    import torch

    c, net = nets["gateway"]
    n = 4096
    packed, packed_len, frames = M.layout(M.random_packets(0xE4, n, DSTS, lens=(0, 1, 19, 20, 21, 64, 700, 1350, stride - 32, stride - 4)),
                                          3, gaps=True)
    dev = DevFrames(c, packed, packed_len, frames, stride)
    bufs = np.stack([frames[:, 0], frames[:, 1], np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32)], axis=1)
    d_bufs = torch.from_numpy(bufs.view(np.int32).reshape(-1).copy()).cuda()
    whole = torch.full((MARGIN + n * stride + MARGIN,), M.SENTINEL, dtype=torch.uint8, device="cuda")
    arena = whole[MARGIN:]
    _, lens, peer, descs = M.fresh(n, stride)
    d_lens, d_peer = torch.from_numpy(lens.view(np.int32)).cuda(), torch.from_numpy(peer.view(np.int32)).cuda()
    d_descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
    route.gro_unpack(c, dev.packed, packed_len, d_bufs, n, n, arena[4:], stride, d_lens)
    route.resolve_outgoing(c, arena, stride, n, d_lens, d_peer, d_descs)
    torch.cuda.synchronize()
    got, got_lens, got_peer, got_descs = dev.read()
    assert np.array_equal(got, whole.cpu().numpy())
    assert np.array_equal(got_lens, d_lens.cpu().numpy().view(np.uint32))
    assert np.array_equal(got_peer, d_peer.cpu().numpy().view(np.uint32)) and (got_peer != NO_PEER).sum() > 1000
    assert np.array_equal(got_descs, d_descs.cpu().numpy().view(M.DESC))


# ---- 6. the pipeline ----

def frames_of(head, lens, seed=0):
    return M.layout([head[i, 4:4 + int(lens[i])] for i in range(len(lens))], seed, gaps=True)


def reference(c, packed, packed_len, frames, stride, nonces, out_bytes):
    """qgcm_frames_unpack_cpu into a zeroed arena, then qgcm_route_chain_seal_packed_host."""
    n = len(frames)
    arena, lens = np.zeros(n * stride, np.uint8), np.zeros(n, np.uint32)
    route.frames_unpack_cpu(packed, packed_len, frames, arena, stride, lens)
    return finish(c, n, lens, out_bytes, lambda *a: route.route_chain_seal_packed_host(c, arena.ctypes.data, stride, n, lens, nonces,
                                                                                      BOTH, *a))


def frames_call(c, packed, packed_len, frames, stride, nonces, out_bytes):
    n = len(frames)
    lens = np.full(n, M.LEN_SENTINEL, np.uint32)  # output only
    before = packed.copy()
    got = finish(c, n, lens, out_bytes, lambda *a: route.route_chain_seal_frames_host(c, packed, packed_len, frames, stride, n, lens,
                                                                                     nonces, BOTH, *a))
    assert np.array_equal(packed, before)
    return got


def finish(c, n, lens, out_bytes, call):
    peer, status = np.full(n, 7, np.uint32), np.full(n, 0xAB, np.uint8)
    out_buf = np.full(out_bytes, M.SENTINEL, np.uint8)
    ptrains, order = np.full((n, 4), M.PEER_SENTINEL, np.uint32), np.full(n, M.PEER_SENTINEL, np.uint32)
    t0, l0 = stats(c, route.TX)
    rc, pt, od, out = call(peer, status, out_buf, None, ptrains, order)
    t1, l1 = stats(c, route.TX)
    assert np.all(ptrains[len(pt):] == M.PEER_SENTINEL) and np.all(order[len(od):] == M.PEER_SENTINEL)
    assert np.all(out_buf[int(out[2]):] == M.SENTINEL)
    return dict(rc=rc, pt=pt.copy(), od=od.copy(), out=out.tolist(), buf=out_buf[:int(out[2])].copy(), lens=lens.copy(), peer=peer,
                status=status, tx=(t1 - t0, l1 - l0))


def same(got, want):
    """Every output; the lengths up to out[0]: behind it the existing call's are its input, the new call's unwritten."""
    assert got["rc"] == want["rc"] and got["out"] == want["out"]
    done = got["out"][0]
    assert np.array_equal(got["lens"][:done], want["lens"][:done]) and np.all(got["lens"][done:] == M.LEN_SENTINEL)
    for k in ("peer", "status", "pt", "od", "buf"):
        assert np.array_equal(got[k], want[k]), k
    same_tx(got["tx"], want["tx"])


def one_chunk(f, nonces_of, n=150, seed=0xF7A0):
    """The existing call on one context, the new one on a second with the same keys and nonces."""
    c, c2 = loop_ctx(f), loop_ctx(f)
    try:
        head, lens, nonces = tun_batch(f, n, seed + f)
        case = frames_of(head, lens, f)
        want = reference(c, *case, SEAL_STRIDE, nonces_of(c, nonces), 1 << 18)
        assert want["out"][3] >= 60 and want["rc"] >= 1
        got = frames_call(c2, *case, SEAL_STRIDE, nonces_of(c2, nonces), 1 << 18)
        same(got, want)
        return c, head, lens, got
    finally:
        c2.close()


@pytest.mark.parametrize("f", (0, 1, 2, 3))
def test_pipeline_matches_the_packed_one(f):
    one_chunk(f, lambda c, nonces: nonces.ctypes.data)[0].close()


def test_pipeline_with_generated_nonces():
    def seeded(c, nonces):
        batch.nonce_seed(c, bytes(range(32)), (77).to_bytes(16, "big"))
        return batch.GENERATE

    one_chunk(3, seeded)[0].close()


def test_pipeline_in_two_chunks_and_the_restart():
    """70 000 frames of 64 bytes at stride 128: a chunk of 65 536 and one of 4 464.  Then an h_out 16 bytes short of
    the whole: QGCM_E_NOMEM with the first chunk done; the call repeated with frames + out[0] over the same packed
    area completes.  The existing call over the host-unpacked arena does the same at every step."""
    n, stride = 70000, 128
    ctxs = [loop_ctx(3) for _ in range(4)]
    c, c2, c3, c4 = ctxs
    try:
        packed, packed_len, frames = small_frames(n, 0x2C70, peers=(3, 11, 7))  # 7 has no key
        nonces = np.random.default_rng(0x2C71).integers(0, 256, 12 * n, dtype=np.uint8)
        want = reference(c, packed, packed_len, frames, stride, nonces.ctypes.data, n * 96)
        assert want["out"][0] == n and want["rc"] > 1000 and want["out"][3] > 30000
        same(frames_call(c2, packed, packed_len, frames, stride, nonces.ctypes.data, n * 96), want)
        short = want["out"][2] - 16
        want1 = reference(c3, packed, packed_len, frames, stride, nonces.ctypes.data, short)
        got1 = frames_call(c4, packed, packed_len, frames, stride, nonces.ctypes.data, short)
        assert got1["rc"] == _lib.QGCM_E_NOMEM and got1["out"][0] == 65536
        same(got1, want1)
        done = got1["out"][0]
        rest = nonces[12 * done:]
        arena, lens = np.zeros(n * stride, np.uint8), np.zeros(n, np.uint32)
        route.frames_unpack_cpu(packed, packed_len, frames, arena, stride, lens)
        tail = arena[done * stride:]
        l2 = lens[done:].copy()
        want2 = finish(c3, n - done, l2, n * 96,
                       lambda *a: route.route_chain_seal_packed_host(c3, tail.ctypes.data, stride, n - done, l2, rest.ctypes.data, BOTH, *a))
        got2 = frames_call(c4, packed, packed_len, frames[done:], stride, rest.ctypes.data, n * 96)  # offsets are absolute
        same(got2, want2)
        assert got1["out"][2] + got2["out"][2] == want["out"][2]
        assert np.array_equal(np.concatenate([got1["buf"], got2["buf"]]), want["buf"])
    finally:
        for x in ctxs:
            x.close()


def test_pipeline_refuses_bad_tables_and_null_nonces():
    L = _lib.lib()
    c = loop_ctx(3)
    try:
        head, lens, nonces = tun_batch(3, 40, 0xBAD7)
        packed, packed_len, frames = frames_of(head, lens)
        n = len(frames)
        unsorted, overlapping, void = frames.copy(), frames.copy(), frames.copy()
        unsorted[[5, 6]] = unsorted[[6, 5]]
        overlapping[7, 1] = int(frames[8, 0]) - int(frames[7, 0]) + 1
        void[9, 0] += 4
        assert M.table_ok(unsorted, packed_len) and M.table_ok(overlapping, packed_len) and not M.table_ok(void, packed_len)
        assert not M.ascends(unsorted, packed_len) and not M.ascends(overlapping, packed_len) and M.ascends(frames, packed_len)
        out_lens, peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        out_buf, pt, od, out = np.zeros(1 << 17, np.uint8), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32), np.zeros(4, np.uint64)

        def call(table, non):
            return L.qgcm_route_chain_seal_frames_host(c.handle, packed.ctypes.data, packed_len, table.ctypes.data, SEAL_STRIDE, n,
                                                       out_lens.ctypes.data, non, BOTH, None, peer.ctypes.data, status.ctypes.data,
                                                       out_buf.ctypes.data, out_buf.size, pt.ctypes.data, od.ctypes.data,
                                                       out.ctypes.data)

        t0, l0 = stats(c, route.TX)
        for table in (unsorted, overlapping, void):
            assert call(table, nonces.ctypes.data) == _lib.QGCM_E_ARG
        assert call(frames, None) == _lib.QGCM_E_ARG
        assert L.qgcm_route_chain_seal_frames_host(c.handle, None, 0, None, SEAL_STRIDE, 0, None, None, BOTH, None, None, None, None, 0,
                                                   None, None, out.ctypes.data) == _lib.QGCM_E_ARG  # NULL nonces, even for no packet
        t1, l1 = stats(c, route.TX)
        same_tx((t1, l1), (t0, l0))
        assert not out_buf.any() and not status.any()
        assert call(frames, nonces.ctypes.data) >= 0 and out[0] == n and out[3] > 10
    finally:
        c.close()


# ---- 7. the wire ----

def cross_the_wire(c, packed, ptrains, order, expect):
    """Send the packed trains over loopback, receive into slots, open with the peer context `c`: packet j is
    expect(order[j]) (one sender, one receiver: arrival order is table order)."""
    wire = Wire(1)
    try:
        m = len(order)
        addrs = route.peer_addrs([("127.0.0.1", wire.L.qgcm_udp_port(wire.rx[0]))] * MAX_KEYS)
        assert route.udp_send_packed(wire.tx, packed, packed.size, ptrains, addrs, MAX_KEYS) == m
        grams = wire.drain(0, m)
        assert len(grams) == m
        arena, got_lens = np.zeros((m, SEAL_STRIDE), np.uint8), np.zeros(m, np.uint32)
        for j, g in enumerate(grams):
            arena[j, :len(g)] = np.frombuffer(g, np.uint8)
            got_lens[j] = len(g)
        peer, status = np.zeros(m, np.uint32), np.full(m, 0xAB, np.uint8)
        assert route.route_chain_open_host(c, arena.ctypes.data, SEAL_STRIDE, m, got_lens, BOTH, peer, status) == 0
        for j, src in enumerate(order.tolist()):
            want = expect(src)
            assert status[j] == 1 and peer[j] == 20 and got_lens[j] == len(want), (j, src)
            assert np.array_equal(arena[j, 4:4 + len(want)], want), (j, src)
    finally:
        wire.close()


def test_the_output_crosses_the_wire_and_opens():
    c, head, lens, got = one_chunk(3, lambda c, nonces: nonces.ctypes.data)
    try:
        cross_the_wire(c, got["buf"], got["pt"], got["od"], lambda src: head[src, 4:4 + int(lens[src])])
    finally:
        c.close()


def test_tun_to_wire_end_to_end():
    """qgcm_tun_read_packed -> qgcm_route_chain_seal_frames_host -> qgcm_udp_send_packed -> the peer's open: the
    packets the kernel routed into the TUN device."""
    import ctypes as C
    import socket

    from test_tun_batch import HOST_IP, PEER_IP

    L = _lib.lib()
    fds, name = (C.c_int * 1)(), C.create_string_buffer(16)
    rc = L.qgcm_tun_open(b"qgcmf%d", 1, fds, name, 16)
    if rc < 0:
        pytest.skip(f"TUN device refused (errno {-rc})")
    key = bytes(range(9, 41))
    own, peer_ip = le(HOST_IP), le(PEER_IP)
    net = CM.Net({peer_ip: 3, own: 20}, le("10.213.7.0"), route.mask_of(24), le("10.213.7.254"), own)
    c = None
    try:
        if L.qgcm_tun_up(name.value, HOST_IP.encode(), 24, 1433) < 0:
            pytest.skip("TUN link set-up refused")
        c = make_ctx(CM.Peers({3: 3, 20: 3}, {3: key, 20: key}, MAX_KEYS), net)
        sk = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        sk.bind((HOST_IP, 0))
        sent = [bytes([j]) * (40 + 13 * j) for j in range(60)]
        for msg in sent:
            sk.sendto(msg, (PEER_IP, 9300))
        sk.close()
        packed, frames = np.zeros(1 << 20, np.uint8), np.zeros((256, 2), np.uint32)
        seen = []
        for _ in range(40):
            out = np.zeros(2, np.uint64)
            n = route.tun_read_packed(fds[0], packed, frames, 256, 50, out)
            assert n >= 0
            if n == 0:
                if len(seen) >= len(sent):
                    break
                continue
            t = frames[:n].copy()
            nonces = np.random.default_rng(n).integers(0, 256, 12 * n, dtype=np.uint8)
            got = frames_call(c, packed, int(out[1]), t, SEAL_STRIDE, nonces.ctypes.data, 1 << 19)
            assert got["rc"] >= 0 and got["out"][0] == n
            frame = lambda src: packed[int(t[src, 0]):int(t[src, 0]) + int(t[src, 1])].copy()
            cross_the_wire(c, got["buf"], got["pt"], got["od"], frame)
            for src in got["od"].tolist():
                pkt = frame(src).tobytes()
                assert pkt[0] >> 4 == 4 and pkt[16:20] == socket.inet_aton(PEER_IP)
                seen.append(pkt[(pkt[0] & 15) * 4 + 8:])
        assert seen == sent
    finally:
        if c is not None:
            c.close()
        L.qgcm_tun_close(fds[0])
