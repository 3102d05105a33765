"""GPU: qgcm_gro_unpack (quantum_amd/csrc/gro_kernels.hip) writes exactly what tests/gro_model.py writes -- the
whole arena and all lengths, pre-filled with sentinels, so slot tails and unnamed slots are proven untouched --
and a sealed routed batch sent with qgcm_udp_send_plan comes back through qgcm_udp_recv_gro and
qgcm_route_chain_open_gro_host as qgcm_route_chain_open_host gives it for the host-unpacked arena.

The kernel gives 16 lanes to a slot and 16 slots to a workgroup, and its grid stops at 4096 workgroups: the
70 001-datagram batches take 4 376 workgroups' worth of slots, so the grid-stride loop runs."""
import numpy as np
import pytest

import chain_model as CM
import gro_model as M
from quantum_amd import _lib, route
from route_model import NO_PEER
from send_plan_wire import Wire
from test_gpu_chain_route import BOTH, FLAGS, MAX_KEYS, NET, OWN, STRANGER, addr, make_ctx, stats

pytestmark = pytest.mark.gpu


class DevUnpack:
    """One qgcm_gro_unpack call enqueued on `stream` over sentinel-filled outputs; read() after a synchronize."""

    def __init__(self, ctx, packed, packed_len, bufs, n, stride, stream=None, arena_shift=0):
        import torch

        assert packed.size % 16 == 0
        self.n, self.stride = n, stride
        self.packed = torch.from_numpy(packed).cuda()
        self.bufs = torch.from_numpy(np.ascontiguousarray(bufs, np.uint32).view(np.int32).reshape(-1).copy()).cuda()
        self.whole = torch.full((max(1, n) * stride + arena_shift,), M.SENTINEL, dtype=torch.uint8, device="cuda")
        self.arena = self.whole[arena_shift:]
        self.lens = torch.from_numpy(np.full(max(1, n), M.LEN_SENTINEL, np.uint32).view(np.int32)).cuda()
        torch.cuda.synchronize()  # the inputs are there whatever stream unpacks
        route.gro_unpack(ctx, self.packed, packed_len, self.bufs, len(bufs), n, self.arena, stride, self.lens, stream)

    def read(self):
        return (self.arena.cpu().numpy()[:self.n * self.stride], self.lens.cpu().numpy().view(np.uint32)[:self.n],
                self.whole.cpu().numpy()[:len(self.whole) - len(self.arena)])


def check(dev, packed, packed_len, bufs, n, stride):
    want_arena, want_lens = M.fresh(n, stride)
    M.unpack(packed, packed_len, bufs, n, want_arena, stride, want_lens)
    arena, lens, before = dev.read()
    bad = np.flatnonzero(lens != want_lens)
    assert bad.size == 0, [(int(i), int(lens[i]), int(want_lens[i])) for i in bad[:8]]
    if not np.array_equal(arena, want_arena):
        at = np.flatnonzero(arena != want_arena)
        raise AssertionError(f"{at.size} bytes differ, the first in slot {int(at[0]) // stride} at byte {int(at[0]) % stride}")
    assert np.all(before == M.SENTINEL)


def run(ctx, case, stride, **kw):
    import torch

    dev = DevUnpack(ctx, *case, stride, **kw)
    torch.cuda.synchronize()
    check(dev, *case, stride)


@pytest.mark.parametrize("stride", (1536, 1388))
def test_edges(ctx, stride):
    """Stride 1536 takes the 16-byte path, 1388 the dword path."""
    run(ctx, M.edge_case(stride), stride)


def test_edges_dword_path_under_a_16_byte_stride(ctx):
    """An arena that is only 4-B aligned sends a stride of 1536 down the dword path."""
    run(ctx, M.edge_case(1536), 1536, arena_shift=4)


@pytest.mark.parametrize("stride", (1536, 1388))
def test_bad_buffers_are_skipped_and_their_neighbours_unpacked(ctx, stride):
    packed, packed_len, bufs, n = M.layout([(300, 100, 1), (4146, 1382, 2), (64, 0, 3), (500, 77, 4), (2764, 1382, 5),
                                            (1382, 0, 6)], 11)
    bad = bufs.copy()
    bad[1, 0] = packed_len - 4145  # one byte past the packed area
    bad[3, 0] = 0xFFFFFFF0         # off + len wraps 32 bits
    assert M.skipped(bad[1], packed_len, n) and M.skipped(bad[3], packed_len, n)
    run(ctx, (packed, packed_len, bad, n), stride)
    # the last buffer names a slot past n; the one before it a datagram more than n leaves it
    run(ctx, (packed, packed_len, bufs, n - 1), stride)
    assert M.skipped(bufs[4], packed_len, n - 2) and M.skipped(bufs[5], packed_len, n - 2)
    run(ctx, (packed, packed_len, bufs, n - 2), stride)


@pytest.mark.parametrize("lone_len", (None, 64))
def test_several_workgroups(ctx, lone_len):
    case = M.random_batch(0x70001, 70001, lone_len)
    assert (len(case[2]) == 70001) if lone_len else (2000 < len(case[2]) < 4000)
    run(ctx, case, 1536)


def test_several_workgroups_dword_path(ctx):
    run(ctx, M.random_batch(0x4099, 4099), 1388)


def test_two_streams_at_once(ctx):
    import torch

    a, b = M.random_batch(51, 4099), M.random_batch(52, 5000, 64)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    devs = [DevUnpack(ctx, *a, 1536, s1), DevUnpack(ctx, *b, 1536, s2), DevUnpack(ctx, *a, 1388, s2),
            DevUnpack(ctx, *b, 64, s1)]
    torch.cuda.synchronize()
    for dev, (case, stride) in zip(devs, ((a, 1536), (b, 1536), (a, 1388), (b, 64))):
        check(dev, *case, stride)


def test_argument_errors_launch_nothing(ctx):
    import torch

    L = _lib.lib()
    case = M.layout([(300, 100, 1), (64, 0, 3)], 12)
    packed, packed_len, bufs, n = case
    dev = DevUnpack(ctx, packed, packed_len, bufs[:0], n, 1536)  # no buffers: nothing launched
    ptr = lambda t: int(t.data_ptr())
    d_bufs = torch.from_numpy(np.concatenate([bufs.view(np.int32).reshape(-1), np.zeros(4, np.int32)])).cuda()
    good = [ctx.handle, ptr(dev.packed), packed_len, ptr(d_bufs), 2, n, ptr(dev.arena), 1536, ptr(dev.lens), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_gro_unpack(*a)

    assert call(a0=None) == _lib.QGCM_E_ARG
    assert call(a5=(1 << 31) + 1) == _lib.QGCM_E_ARG
    assert call(a4=n + 1) == _lib.QGCM_E_ARG  # more buffers than datagrams
    for k in (1, 3, 6, 8):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a1=ptr(dev.packed) + 4) == _lib.QGCM_E_ARG  # the packed area off its 16-B boundary
    assert call(a3=ptr(d_bufs) + 4) == _lib.QGCM_E_ARG      # the table off its 16-B boundary
    assert call(a6=ptr(dev.arena) + 2) == _lib.QGCM_E_ARG
    assert call(a8=ptr(dev.lens) + 2) == _lib.QGCM_E_ARG
    assert call(a7=1538) == _lib.QGCM_E_ARG and call(a7=0) == _lib.QGCM_E_ARG
    assert call(a5=0, a4=0) == 0
    torch.cuda.synchronize()
    arena, lens, _ = dev.read()
    assert np.all(arena == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    check(dev, *case, 1536)


# ---- end to end over loopback ----

def sealed_batch(c, f, n, seed):
    """n TUN packets of 1350 random bytes (they do not compress, so a peer's datagrams share one length and
    travel as trains) to the peers of flags f, sealed by qgcm_route_chain_seal_host at stride 1472."""
    stride, L = 1472, 1350
    dests = (f, f + 8, f + 4)  # same flags; f + 4 has no key
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    for i in range(n):
        slots[i, 20:24] = np.frombuffer(addr(dests[(i // 50) % 3]).to_bytes(4, "little"), np.uint8)
    tun = slots.copy()
    lens, peer, status = np.full(n, L, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    route.route_chain_seal_host(c, slots.ctypes.data, stride, n, lens, nonces.ctypes.data, BOTH, peer, status)
    return tun, slots, lens, peer, status


def over_the_wire(c, f, n, open_stride, seed):
    """Sealed, planned, sent, received coalesced and opened with slots of open_stride bytes -> the number of
    datagrams that crossed."""
    wire = Wire(1)
    try:
        route.udp_gro(wire.rx[0], True)
        tun, slots, lens, peer, status = sealed_batch(c, f, n, seed)
        sendable = np.flatnonzero((status == 1) & (lens != 0))
        assert len(sendable) >= 100
        order, trains = route.send_plan_host(c, lens, peer)
        assert sorted(order.tolist()) == sendable.tolist() and int(trains[:, 1].max()) >= 40
        # inside the first long train: one datagram forged, one from a sender no route knows
        long_train = trains[np.flatnonzero(trains[:, 1] >= 40)[0]]
        forged, stranger = (int(order[int(long_train[0]) + k]) for k in (7, 19))
        slots[forged, 40] ^= 1
        slots[stranger, 0:4] = np.frombuffer(STRANGER.to_bytes(4, "little"), np.uint8)
        port = wire.L.qgcm_udp_port(wire.rx[0])
        addrs = route.peer_addrs([("127.0.0.1", port)] * MAX_KEYS)
        assert route.udp_send_plan(wire.tx, slots.ctypes.data, 1472, n, lens, order, trains, addrs, MAX_KEYS) == len(order)
        m = len(order)
        packed, bufs, out = np.zeros(1 << 20, np.uint8), np.zeros((1024, 4), np.uint32), np.zeros(3, np.uint64)
        assert route.udp_recv_gro(wire.rx[0], packed, bufs, 1024, 1000, out) == m
        bufs, used = bufs[:int(out[0])], int(out[1])
        assert M.table_ok(bufs, m) and int(out[2]) == 0
    finally:
        wire.close()
    where = {int(src): j for j, src in enumerate(order)}  # arrival order is plan order: one sender, one receiver
    if M.host_coalesces():
        inside = [b for b in bufs if M.count(int(b[1]), int(b[2])) > 1 and
                  int(b[3]) <= where[forged] and where[stranger] < int(b[3]) + M.count(int(b[1]), int(b[2]))]
        assert len(inside) == 1, "the forged and the unroutable datagram did not arrive inside one coalesced buffer"

    # the existing pipeline on the arena the host unpack makes of the same input
    ref_arena, ref_lens = np.zeros(m * open_stride, np.uint8), np.zeros(m, np.uint32)
    route.gro_unpack_cpu(packed, used, bufs, m, ref_arena, open_stride, ref_lens)
    dgram = ref_lens.copy()
    assert dgram.tolist() == [int(lens[src]) for src in order]
    ref_peer, ref_status = np.zeros(m, np.uint32), np.full(m, 0xAB, np.uint8)
    t0, l0 = stats(c, route.RX)
    ref_dropped = route.route_chain_open_host(c, ref_arena.ctypes.data, open_stride, m, ref_lens, BOTH, ref_peer, ref_status)
    t1, l1 = stats(c, route.RX)
    # the new one
    arena, got_lens = np.empty(m * open_stride, np.uint8), np.full(m, M.LEN_SENTINEL, np.uint32)
    got_peer, got_status = np.zeros(m, np.uint32), np.full(m, 0xAB, np.uint8)
    dropped = route.route_chain_open_gro_host(c, packed, used, bufs, arena.ctypes.data, open_stride, m, got_lens, BOTH,
                                              got_peer, got_status)
    t2, l2 = stats(c, route.RX)
    assert dropped == ref_dropped
    assert np.array_equal(got_peer, ref_peer) and np.array_equal(got_status, ref_status) and np.array_equal(got_lens, ref_lens)
    assert (t2 - t1).tolist() == (t1 - t0).tolist() and np.array_equal(l2 - l1, l1 - l0)
    arena, ref_arena = arena.reshape(m, open_stride), ref_arena.reshape(m, open_stride)
    for j in range(m):
        end = 4 + int(got_lens[j]) if got_status[j] == 1 else int(dgram[j])
        assert np.array_equal(arena[j, :end], ref_arena[j, :end]), j
    # and the packets are the ones that went in
    assert got_peer[where[stranger]] == NO_PEER and got_status[where[stranger]] == 0 and dropped >= 1
    if f & CM.ENCRYPTION:
        assert got_status[where[forged]] == 0 and dropped == 2
    for j, src in enumerate(order):
        if src in (forged, stranger):
            continue
        assert got_status[j] == 1 and got_peer[j] == 20 and got_lens[j] == 1350, (j, src)
        assert np.array_equal(arena[j, 4:4 + 1350], tun[src, 4:4 + 1350]), (j, src)
    return m


def loop_ctx(f):
    """The round trip's context of tests/test_gpu_chain_route.py: slot 20 stands for this node on the way back
    in, with the key and the flags of the peers sealed to."""
    key = bytes(range(7, 39))
    net = CM.Net({**NET.table, OWN: 20}, NET.net, NET.mask, NET.gateway, OWN)
    return make_ctx(CM.Peers({**FLAGS, 20: f}, {f: key, f + 8: key, 20: key}, MAX_KEYS), net)


@pytest.mark.parametrize("f", (0, 1, 2, 3))
def test_sealed_batch_over_loopback(f):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = loop_ctx(f)
    try:
        over_the_wire(c, f, 150, 1472, 0x6A0 + f)
    finally:
        c.close()


def test_sealed_batch_over_loopback_in_two_chunks():
    """Slots of 1 MiB on the way in: a chunk of the routed host pipelines holds 256 of them, so the 300
    datagrams that cross are opened in two chunks, cut at a buffer boundary."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = loop_ctx(3)
    try:
        assert over_the_wire(c, 3, 450, 1 << 20, 0x2C4) > 256
    finally:
        c.close()
