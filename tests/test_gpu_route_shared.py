"""The state the routed host pipelines share (quantum_amd/csrc/route.cpp: the stream, the device arena, the side
buffer and the ingest staging belong to the context, whatever form the batch arrives in): one context serves the
forms in turn and gives what a fresh context gives.  All comparisons are exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
TWO = 257  # slots of 1 MiB: kRouteChunkBytes holds 256, so every call below runs a chunk of 256 and a chunk of 1


def coalesced_of(dgrams, per=4):
    """The datagrams back to back as qgcm_udp_recv_gro would leave them: runs of up to `per` equal lengths share a
    buffer -> (packed, packed_len, bufs)."""
    bufs, at, i = [], 0, 0
    while i < len(dgrams):
        k = i + 1
        while k < len(dgrams) and k - i < per and len(dgrams[k]) == len(dgrams[i]):
            k += 1
        total = sum(len(d) for d in dgrams[i:k])
        bufs.append((at, total, len(dgrams[i]) if k - i > 1 else 0, i))
        at, i = at + total, k
    packed = np.zeros((at + 15) & ~15, np.uint8)
    packed[:at] = np.concatenate(dgrams)
    return packed, at, np.array(bufs, np.uint32)


def test_one_context_serves_every_pipeline_form_in_turn():
    """One context takes, in this order, the chained super-frame seal, the chained coalesced open, the chained
    frames seal, the coalesced open with coalesced delivery and the plain open from slots -- tables of 32-, 16- and
    8-byte entries, then none; with and without nonces, chain work area and packed outputs -- each in two chunks
    (257 slots of 1 MiB), and each gives what the same call gives on a fresh context of its own: a staging or side
    buffer sized or laid out for the previous form would show."""
    import gso_model as GM
    import test_gpu_gro as G
    from quantum_amd import route
    from test_gpu_chain_route import BOTH, STRANGER, addr, stats
    from test_gpu_frames import finish, same
    from test_gpu_gso import host_segmented

    rng = np.random.default_rng(0x5A4ED)
    dsts = (addr(3), addr(11), addr(7), STRANGER)  # 7 has no key
    items = ([GM.tcp_frame(rng, 44 * 60 + 13, 60, dsts[i % 2]) for i in range(4)] +
             [GM.udp_frame(rng, 10 * 50 + 1, 50, dsts[(i + 1) % 4]) for i in range(7)])
    g_packed, g_len, g_frames, n = GM.layout(items, 21)
    assert n == TWO and len(g_frames) == 11
    f_packed, f_len, f_table = host_segmented(g_packed, g_len, g_frames, n, 160)
    nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)

    helper = G.loop_ctx(3)
    try:
        _, slots, s_lens, _, s_status = G.sealed_batch(helper, 3, 400, 0x5A4EE)
    finally:
        helper.close()
    src = np.flatnonzero((s_status == 1) & (s_lens != 0))[:TWO]
    assert len(src) == TWO
    dgrams = [slots[i, :int(s_lens[i])].copy() for i in src]
    dgrams[7][40] ^= 1                                                      # forged
    dgrams[19][0:4] = np.frombuffer(STRANGER.to_bytes(4, "little"), np.uint8)  # from a sender no route knows
    d_len = np.array([len(d) for d in dgrams], np.uint32)
    packed, used, bufs = coalesced_of(dgrams)
    assert G.M.table_ok(bufs, TWO) and 2 <= len(bufs) < TWO
    arena = np.zeros(TWO * MIB, np.uint8)  # the host arena of the two calls that have one
    heads = arena.reshape(TWO, MIB)[:, :2048]

    def sealed(call, table):
        def run(c):
            lens = np.full(n, GM.LEN_SENTINEL, np.uint32)
            return finish(c, n, lens, 1 << 17, lambda *a: call(c, *table, MIB, n, lens, nonces.ctypes.data, BOTH, *a))
        return run

    def opened(call):
        def run(c):
            lens, peer, status = np.full(TWO, G.M.LEN_SENTINEL, np.uint32), np.full(TWO, 7, np.uint32), np.full(TWO, 0xAB, np.uint8)
            t0, l0 = stats(c, route.RX)
            res = call(c, lens, peer, status)
            t1, l1 = stats(c, route.RX)
            assert 2 <= int((status == 0).sum()) < 8 and set(status.tolist()) == {0, 1}
            return dict(res, lens=lens, peer=peer, status=status, tot=t1 - t0, links=l1 - l0)
        return run

    def delivered(lens, status):
        """The bytes of every slot that the call defines: the packet of a delivered one, the datagram of a dropped."""
        return [heads[j, :4 + int(lens[j]) if status[j] == 1 else int(d_len[j])].copy() for j in range(TWO)]

    def chain_gro(c, lens, peer, status):
        rc = route.route_chain_open_gro_host(c, packed, used, bufs, arena.ctypes.data, MIB, TWO, lens, BOTH, peer, status)
        return dict(rc=rc, slots=delivered(lens, status))

    def gro_coalesced(c, lens, peer, status):
        out_buf = np.full(1 << 19, 0x5A, np.uint8)
        rc, frames, out = route.route_chain_open_gro_coalesced_host(c, packed, used, bufs, MIB, TWO, lens, BOTH, peer, status, out_buf)
        assert out[0] == TWO and np.all(out_buf[int(out[2]):] == 0x5A)
        return dict(rc=rc, frames=frames.copy(), out=out.copy(), buf=out_buf[:int(out[2])].copy())

    def plain(c, lens, peer, status):
        for j, d in enumerate(dgrams):
            heads[j, :len(d)] = d
        lens[:] = d_len
        rc = route.route_open_host(c, arena.ctypes.data, MIB, TWO, lens, peer, status)
        return dict(rc=rc, slots=delivered(lens, status))

    def same_opened(got, want):
        assert got.keys() == want.keys()
        for k in want:
            if k == "slots":
                assert all(np.array_equal(g, w) for g, w in zip(got[k], want[k]))
            else:
                assert np.array_equal(got[k], want[k]), k

    forms = ((sealed(route.route_chain_seal_gso_host, (g_packed, g_len, g_frames)), same),
             (opened(chain_gro), same_opened),
             (sealed(route.route_chain_seal_frames_host, (f_packed, f_len, f_table)), same),
             (opened(gro_coalesced), same_opened),
             (opened(plain), same_opened))
    shared = G.loop_ctx(3)
    try:
        for run, compare in forms:
            got = run(shared)
            own = G.loop_ctx(3)
            try:
                want = run(own)
            finally:
                own.close()
            compare(got, want)
    finally:
        shared.close()
