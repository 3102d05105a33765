"""CPU: tests/gro_resolve_model.py on hand-written tables, every expected length, peer and descriptor written
out, and against qgcm_gro_unpack_cpu followed by tests/chain_model.py's incoming resolve on a seeded batch; and
the new symbol in the header and the export list."""
import os
import re

import numpy as np
import pytest

import chain_model as CM
import gro_model as G
import gro_resolve_model as M
from conftest import ROOT
from quantum_amd import _lib, route
from route_model import NO_PEER

le = route.IPtoInt
HIT, MISS, OUTSIDE, GATEWAY, OWN = le("10.99.1.3"), le("10.99.200.200"), le("8.8.8.8"), le("10.99.7.7"), le("10.99.0.1")
TABLE = {le(f"10.99.1.{p}"): p for p in range(17)}
NETS = {"gateway": M.Net({**TABLE, GATEWAY: 18}, le("10.99.0.0"), route.mask_of(16), GATEWAY, OWN),
        "no-gateway": M.Net(TABLE, le("10.99.0.0"), route.mask_of(16), GATEWAY, OWN)}
STRIDE = 64


def four(a: int):
    return np.frombuffer(a.to_bytes(4, "little"), np.uint8)


def run(net, packed, packed_len, bufs, n, stride=STRIDE, before=None):
    arena, lens, peer, descs = M.fresh(n, stride)
    if before:
        before(arena, lens)
    M.gro_resolve(net, packed, packed_len, np.array(bufs, np.uint32).reshape(-1, 4), n, arena, stride, lens, peer, descs)
    return arena, lens.tolist(), peer.tolist(), [tuple(int(v) for v in d) for d in descs.tolist()]


def test_a_lone_datagram():
    packed = np.arange(48, dtype=np.uint8)
    packed[5:9] = four(HIT)
    arena, lens, peer, descs = run(NETS["gateway"], packed, 45, [(5, 40, 0, 0)], 1)
    assert lens == [40] and peer == [3] and descs == [(0, 36, 3)]
    assert np.array_equal(arena[:40], packed[5:45]) and np.all(arena[40:] == M.SENTINEL)


def test_a_train_with_a_shorter_tail():
    packed = np.arange(64, dtype=np.uint8)
    packed[3:7], packed[23:27], packed[43:47] = four(HIT), four(MISS), four(le("10.99.1.9"))
    arena, lens, peer, descs = run(NETS["gateway"], packed, 50, [(3, 47, 20, 0)], 3)
    assert lens == [20, 20, 7] and peer == [3, NO_PEER, 9]
    assert descs == [(0, 16, 3), (64, 16, NO_PEER), (128, 3, 9)]
    assert np.array_equal(arena[128:135], packed[43:50]) and np.all(arena[135:192] == M.SENTINEL)


def test_lengths_around_four_and_the_stride():
    """L in {0, 3, 4, stride, stride + 1}: 0 and 3 hold no address, stride + 1 keeps its length and misses."""
    specs = [(L, 0, mod) for L, mod in ((0, 1), (3, 2), (4, 3), (STRIDE, 5), (STRIDE + 1, 6))]
    packed, packed_len, bufs, n = G.layout(specs, 1)
    for b in bufs:
        if b[1] >= 4:
            packed[b[0]:b[0] + 4] = four(HIT)
    arena, lens, peer, descs = run(NETS["gateway"], packed, packed_len, bufs, n)
    assert lens == [0, 3, 4, 64, 65]
    assert peer == [NO_PEER, NO_PEER, 3, 3, NO_PEER]
    assert descs == [(0, 0, NO_PEER), (64, 0, NO_PEER), (128, 0, 3), (192, 60, 3), (256, 61, NO_PEER)]
    assert np.all(arena[0:64] == M.SENTINEL) and np.all(arena[64 + 3:128] == M.SENTINEL)
    assert np.array_equal(arena[256:320], packed[bufs[4][0]:bufs[4][0] + 64])  # cut at the stride


def test_a_gap_in_first_and_a_skipped_buffer():
    """Slot 1 is named by nobody, slot 3 by a buffer one byte past packed_len: both keep their length and bytes
    and are resolved from them."""
    packed = np.zeros(64, np.uint8)
    packed[0:4], packed[16:20], packed[40:44] = four(HIT), four(le("10.99.1.5")), four(le("10.99.1.6"))

    def before(arena, lens):
        arena[64:68], lens[1] = four(le("10.99.1.7")), 12
        arena[192:196], lens[3] = four(le("10.99.1.8")), 3
    arena, lens, peer, descs = run(NETS["gateway"], packed, 48, [(0, 8, 0, 0), (16, 8, 0, 2), (40, 9, 0, 3)], 5, before=before)
    assert lens == [8, 12, 8, 3, M.LEN_SENTINEL]
    assert peer == [3, 7, 5, NO_PEER, NO_PEER]
    assert descs == [(0, 4, 3), (64, 8, 7), (128, 4, 5), (192, 0, NO_PEER), (256, M.LEN_SENTINEL - 4, NO_PEER)]
    assert np.all(arena[68:128] == M.SENTINEL) and np.all(arena[196:] == M.SENTINEL)


@pytest.mark.parametrize("name,want", (("gateway", 18), ("no-gateway", NO_PEER)))
def test_the_gateway_mapped_and_unmapped(name, want):
    packed = np.zeros(32, np.uint8)
    packed[1:5] = four(OUTSIDE)
    _, lens, peer, descs = run(NETS[name], packed, 21, [(1, 20, 0, 0)], 1)
    assert lens == [20] and peer == [want] and descs == [(0, 16, want)]


def test_without_a_table_it_is_the_incoming_resolve():
    def before(arena, lens):
        arena[0:4], lens[0] = four(HIT), 64
        arena[64:68], lens[1] = four(HIT), 65
    arena, lens, peer, descs = run(NETS["gateway"], np.zeros(16, np.uint8), 0, [], 2, before=before)
    assert lens == [64, 65] and peer == [3, NO_PEER] and descs == [(0, 60, 3), (64, 61, NO_PEER)]


@pytest.mark.parametrize("stride", (1536, 1388))
def test_seeded_batch_equals_the_host_unpack_then_the_chain_models_resolve(stride):
    net = NETS["gateway"]
    packed, packed_len, bufs, n = G.random_batch(0x6E50, 1500)
    M.plant(packed, bufs, (HIT, MISS, OUTSIDE), 1)
    arena, lens, peer, descs = M.fresh(n, stride)
    M.gro_resolve(net, packed, packed_len, bufs, n, arena, stride, lens, peer, descs)
    ref_arena, ref_lens = G.fresh(n, stride)
    route.gro_unpack_cpu(packed, packed_len, bufs, n, ref_arena, stride, ref_lens)
    assert np.array_equal(arena, ref_arena) and np.array_equal(lens, ref_lens)
    cm = CM.Net(net.table, net.net, net.mask, net.gateway, net.own_ip)
    for i in range(n):
        want = CM.resolve_in(cm, ref_arena[i * stride:(i + 1) * stride], int(ref_lens[i]), stride, 32)
        assert int(peer[i]) == want, i
        assert tuple(int(v) for v in descs[i].tolist()) == (i * stride, max(0, int(ref_lens[i]) - 4), want), i
    assert {3, 18, NO_PEER} <= set(peer.tolist()) and (peer != NO_PEER).sum() > 500


def test_the_edge_case_is_what_the_gpu_test_says_it_is():
    """The figures tests/test_gpu_gro_resolve.py names for gro_model.edge_case."""
    for stride in (1536, 1388):
        packed, packed_len, bufs, n = G.edge_case(stride)
        grams = [d for b in bufs for d in G.datagrams(b)]
        readable = [(src, L) for _, src, L in grams if 4 <= L <= stride]
        assert (n, len(bufs), len(readable)) == (2001, 661, 1425)
        assert {src % 16 for src, _ in readable} == set(range(16))
        assert {src % 16 for src, L in readable if L == 4} >= {13, 14, 15}
        assert sum(L < 4 for _, _, L in grams) == 480 and sum(L > stride for _, _, L in grams) == 96


def test_symbol_in_the_header_and_the_export_list():
    with open(os.path.join(ROOT, "include", "qgcm.h")) as f:
        assert re.search(r"^int qgcm_gro_resolve\(", f.read(), re.M)
    assert "qgcm_gro_resolve" in _lib.EXPORTS
