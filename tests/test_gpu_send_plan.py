"""GPU: qgcm_send_plan (quantum_amd/csrc/plan_kernels.hip) writes exactly the plan of tests/send_plan_model.py
-- counts, order[:m], trains[:t] -- and a planned batch goes over loopback as its peers' sealed datagrams.

The device scan works in tiles of 256 positions, one lane each (kPlanTile; send_plan_model.TILE), so the
boundary shapes of send_plan_model.edge_cases sit at 255, 256 and 257, and the 70 001-packet batch gives the
one-workgroup spine kernel 274 tile summaries to fold."""
import ctypes as C
import os

import numpy as np
import pytest

import send_plan_model as M
from quantum_amd import _lib, batch, route
from send_plan_wire import STRIDE, Wire, expected

pytestmark = pytest.mark.gpu


def small_ctx(max_keys, plan_device_min):
    """A context that skips the per-packet GHASH tables (not used here), with QGCM_PLAN_DEVICE_MIN as given."""
    from quantum_amd.crypto import Context

    env = {"QGCM_FLAT_GHASH_KEYS": "0", "QGCM_PLAN_DEVICE_MIN": str(plan_device_min)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Context(device=0, max_keys=max_keys)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def cx_device():
    """max_keys 1000 (not a power of two); qgcm_send_plan_host always plans on the device."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = small_ctx(1000, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cx_host():
    """max_keys 1000; qgcm_send_plan_host always plans on the host."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = small_ctx(1000, 4294967295)
    yield c
    c.close()


class DevPlan:
    """One qgcm_send_plan call enqueued on `stream`; read() after a synchronize."""

    def __init__(self, ctx, lens, peer, kw, stream=None):
        import torch

        n = len(lens)
        self.n = n
        self.d_lens = torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32).copy()).cuda()
        self.d_peer = torch.from_numpy(np.asarray(peer, np.uint32).view(np.int32).copy()).cuda()
        self.order = torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda")
        self.trains = torch.full((4 * max(1, n),), -1, dtype=torch.int32, device="cuda")
        self.counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        self.work = route.send_plan_work(n)
        torch.cuda.synchronize()  # the inputs are there whatever stream plans
        route.send_plan(ctx, n, self.d_lens, self.d_peer, self.order, self.trains, self.counts, self.work,
                        route.plan_limits(**kw) if kw else None, stream)

    def read(self):
        m, t = self.counts.cpu().numpy().view(np.uint32).tolist()
        assert m <= self.n and t <= m
        order = self.order.cpu().numpy().view(np.uint32)[:m].tolist()
        trains = self.trains.cpu().numpy().view(np.uint32).reshape(-1, 4)[:t]
        return order, [tuple(x) for x in trains.tolist()]


def check_case(ctx, max_keys, name, lens, peer, kw):
    import torch

    dev = DevPlan(ctx, lens, peer, kw)
    torch.cuda.synchronize()
    want_order, want_trains = M.plan(lens, peer, max_keys, M.limits(**kw))
    got_order, got_trains = dev.read()
    assert len(got_order) == len(want_order) and len(got_trains) == len(want_trains), name
    assert got_order == want_order, name
    assert got_trains == want_trains, name


def test_edges_max_keys_2048(ctx):
    for case in M.edge_cases(2048):
        check_case(ctx, 2048, *case)


def test_edges_max_keys_1000(cx_device):
    for case in M.edge_cases(1000):
        check_case(cx_device, 1000, *case)


@pytest.mark.parametrize("peers", (3, 1024))
def test_several_workgroups(ctx, peers):
    check_case(ctx, 2048, f"n70001-p{peers}", *M.random_batch(31 + peers, 70001, peers, 2048), {})


@pytest.mark.parametrize("n,peers", ((300601, 1024), (600001, 3)))
def test_spine_folds_several_tiles_per_lane(ctx, n, peers):
    """Past 262 144 packets a lane of the one-workgroup spine kernel folds more than one tile summary: 1 175
    tiles are two a lane with a ragged last stretch and idle lanes behind it, 2 344 are three a lane.  This is
    the range in which qgcm_send_plan_host takes the device by default."""
    check_case(ctx, 2048, f"n{n}-p{peers}", *M.random_batch(n + peers, n, peers, 2048), {})


def test_two_streams_at_once(ctx):
    import torch

    a = M.random_batch(41, 4099, 3, 2048)
    b = M.random_batch(42, 5000, 1024, 2048, lengths=(100, 1382))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    plans = [DevPlan(ctx, *a, {}, s1), DevPlan(ctx, *b, {"max_segs": 7}, s2),
             DevPlan(ctx, *a, {"max_segs": 2}, s2), DevPlan(ctx, *b, {}, s1)]
    torch.cuda.synchronize()
    for dev, (batch_, kw) in zip(plans, ((a, {}), (b, {"max_segs": 7}), (a, {"max_segs": 2}), (b, {}))):
        want = M.plan(*batch_, 2048, M.limits(**kw))
        assert dev.read() == (want[0], want[1])


def test_argument_errors_leave_the_counts_alone(ctx):
    import torch

    L = _lib.lib()
    lens, peer = M.random_batch(1, 64, 3, 2048)
    dev = DevPlan(ctx, lens, peer, {})
    torch.cuda.synchronize()
    dev.counts.fill_(-1)
    ptr = lambda t: int(t.data_ptr())
    good = [ctx.handle, 64, ptr(dev.d_lens), ptr(dev.d_peer), None, ptr(dev.order), ptr(dev.trains), ptr(dev.counts),
            ptr(dev.work), None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_send_plan(*a)

    assert call(a1=(1 << 31) + 1) == _lib.QGCM_E_ARG
    assert call(a0=None) == _lib.QGCM_E_ARG
    for k in (2, 3, 5, 6, 7, 8):  # each array in turn
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert call(a6=ptr(dev.trains) + 4) == _lib.QGCM_E_ARG  # trains off their 16-B boundary
    assert call(a8=ptr(dev.work) + 16) == _lib.QGCM_E_ARG   # the work area off its 256-B boundary
    for kw in ({"max_segs": 1025}, {"max_bytes": 65508}):
        lim = route.plan_limits(**kw)
        assert call(a4=C.addressof(lim)) == _lib.QGCM_E_ARG, kw
    assert call(a1=0) == 0  # an empty batch launches nothing
    torch.cuda.synchronize()
    assert dev.counts.cpu().tolist() == [-1, -1]
    assert call() == 0
    torch.cuda.synchronize()
    assert dev.read() == tuple(M.plan(lens, peer, 2048))


@pytest.mark.parametrize("n", (65, 4099))
def test_host_call_on_both_paths(cx_device, cx_host, n):
    for kw in ({}, {"max_segs": 7, "max_seg_len": 1000}):
        lens, peer = M.random_batch(50 + n, n, 16, 1000)
        want_order, want_trains = M.plan(lens, peer, 1000, M.limits(**kw))
        for c in (cx_device, cx_host):
            order, trains = route.send_plan_host(c, lens, peer, route.plan_limits(**kw) if kw else None)
            assert order.tolist() == want_order and [tuple(t) for t in trains.tolist()] == want_trains
    nothing = np.zeros(n, np.uint32)
    for c in (cx_device, cx_host):
        order, trains = route.send_plan_host(c, nothing, nothing)
        assert len(order) == 0 and len(trains) == 0
        lim = route.plan_limits(max_segs=2000)
        with pytest.raises(_lib.QgcmError):
            route.send_plan_host(c, lens, peer, lim)


def test_wire():
    """resolve -> chain (encryption only) -> plan on the device, then the planned send over loopback: every
    peer's socket gets that peer's sealed datagrams, byte for byte as the slots hold them, in arena order."""
    import torch

    from quantum_amd.crypto import Context

    peers, n = 3, 96
    addr = lambda p: route.IPtoInt(f"10.99.1.{p}")
    c = Context(device=0, max_keys=4)
    wire = Wire(peers)
    try:
        for p in range(peers):
            c.set_key(p, bytes((p * 29 + k) & 0xFF for k in range(32)))
        route.routes_set(c, {addr(p): p for p in range(peers)}, route.IPtoInt("10.99.0.0"), route.mask_of(16),
                         route.IPtoInt("10.99.7.7"), route.IPtoInt("10.99.0.1"))
        rng = np.random.default_rng(96)
        slots = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
        # TUN packet lengths in stretches, so that a peer's neighbours often share one; every 11th to a stranger
        tun_lens = np.array([(20, 668, 1350, 64)[(i // 9) % 4] for i in range(n)], np.uint32)
        for i in range(n):
            dst = route.IPtoInt("10.99.200.200") if i % 11 == 7 else addr((i * 7) % peers)
            slots[i, 20:24] = np.frombuffer(dst.to_bytes(4, "little"), np.uint8)
        arena = torch.from_numpy(slots.reshape(-1).copy()).cuda()
        d_lens = torch.from_numpy(tun_lens.view(np.int32).copy()).cuda()
        d_peer = torch.zeros(n, dtype=torch.int32, device="cuda")
        descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        nbytes = torch.zeros(n, dtype=torch.int32, device="cuda")
        order = torch.zeros(n, dtype=torch.int32, device="cuda")
        trains = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        route.resolve_outgoing(c, arena, STRIDE, n, d_lens, d_peer, descs)
        route.chain_outgoing(c, arena, STRIDE, n, d_lens, d_peer, descs, route.PLUGIN_ENCRYPTION, batch.GENERATE, status,
                             nbytes, route.chain_work(n))
        route.send_plan(c, n, d_lens, d_peer, order, trains, counts, route.send_plan_work(n))
        torch.cuda.synchronize()
        sealed = arena.cpu().numpy().reshape(n, STRIDE)
        lens = d_lens.cpu().numpy().view(np.uint32)
        peer = d_peer.cpu().numpy().view(np.uint32)
        m, t = counts.cpu().tolist()
        h_order = order.cpu().numpy().view(np.uint32)[:m]
        h_trains = trains.cpu().numpy().view(np.uint32).reshape(-1, 4)[:t]
        want = M.plan(lens, peer, 4)
        assert (h_order.tolist(), [tuple(x) for x in h_trains.tolist()]) == want
        strangers = sum(1 for i in range(n) if i % 11 == 7)
        assert m == n - strangers and t < m  # some trains hold several datagrams
        assert np.array_equal(lens[lens != 0], tun_lens[lens != 0] + 32)
        stats = np.zeros(3, np.uint64)
        assert wire.send(sealed, lens, h_order, h_trains, stats) == m
        got = [wire.drain(p, int(np.sum((peer == p) & (lens != 0)))) for p in range(peers)]
        for p in range(peers):
            assert got[p] == expected(sealed, lens, peer, p), p
        # over all sockets: the packets qgcm_udp_send_slots_to would send
        would = [sealed[i, :lens[i]].tobytes() for i in range(n) if peer[i] != M.NO_PEER and lens[i] != 0]
        assert sorted(b for g in got for b in g) == sorted(would) and len(would) == m
    finally:
        wire.close()
        c.close()
