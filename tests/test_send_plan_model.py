"""CPU: the send plan's contract (tests/send_plan_model.py) has the properties include/qgcm.h states, and the
host planner qgcm_send_plan_cpu (quantum_amd/csrc/send_plan_core.h) equals it byte for byte."""
import numpy as np
import pytest

import send_plan_model as M
from quantum_amd import _lib, route

MAX_KEYS = (2048, 1000)


def batches(max_keys):
    out = M.edge_cases(max_keys)
    for seed, (n, peers) in enumerate(((500, 2), (3000, 16), (3000, 1024), (20000, 50))):
        for kw in ({}, {"max_segs": 5}, {"max_seg_len": 1000}, {"max_bytes": 4000}):
            out.append((f"random-{seed}-{kw}", *M.random_batch(900 + seed, n, peers, max_keys), kw))
    return out


@pytest.mark.parametrize("max_keys", MAX_KEYS)
def test_model_properties(max_keys):
    for name, lens, peer, kw in batches(max_keys):
        lim = M.limits(**kw)
        order, trains = M.plan(lens, peer, max_keys, lim)
        sendable = [i for i in range(len(lens)) if peer[i] < max_keys and lens[i] != 0]
        assert sorted(order) == sendable, name  # each sendable index exactly once, and no other
        pos = 0
        for first, count, p, seg in trains:  # the trains tile [0, m)
            assert first == pos and 1 <= count <= M.cap(seg, lim), name
            assert all(peer[i] == p and lens[i] == seg for i in order[first:first + count]), name
            pos += count
        assert pos == len(order), name
        for a, b in zip(trains, trains[1:]):  # no two neighbours that the limits would have let be one
            if a[2:] == b[2:]:
                assert a[1] == M.cap(a[3], lim), name
        last = {}
        for i in order:  # arena order within a peer
            assert last.get(peer[i], -1) < i, name
            last[peer[i]] = i
        assert [peer[i] for i in order] == sorted(peer[i] for i in order), name


@pytest.mark.parametrize("max_keys", MAX_KEYS)
def test_host_planner_equals_model(max_keys):
    for name, lens, peer, kw in batches(max_keys):
        order, trains = route.send_plan_cpu(lens, peer, max_keys, route.plan_limits(**kw) if kw else None)
        want_order, want_trains = M.plan(lens, peer, max_keys, M.limits(**kw))
        assert order.tolist() == want_order, name
        assert [tuple(t) for t in trains.tolist()] == want_trains, name


def test_host_planner_many_key_slots():
    """More than 65536 key slots: the sort's third 8-bit pass, which ends in the other buffer."""
    max_keys = (1 << 20) - 1
    lens, peer = M.random_batch(5, 5000, 300, max_keys)
    order, trains = route.send_plan_cpu(lens, peer, max_keys)
    want_order, want_trains = M.plan(lens, peer, max_keys)
    assert order.tolist() == want_order and [tuple(t) for t in trains.tolist()] == want_trains


def test_empty_batch_and_limit_errors():
    L = _lib.lib()
    lens, peer = M.random_batch(1, 64, 3, 2048)
    order, trains, counts = np.zeros(64, np.uint32), np.zeros((64, 4), np.uint32), np.full(2, 7, np.uint32)
    args = (lens.ctypes.data, peer.ctypes.data, 2048)
    outs = (order.ctypes.data, trains.ctypes.data, counts.ctypes.data)
    assert L.qgcm_send_plan_cpu(0, None, None, 2048, None, None, None, counts.ctypes.data) == 0
    assert counts.tolist() == [0, 0]
    counts[:] = 7
    for kw in ({"max_segs": 1025}, {"max_bytes": 65508}, {"max_segs": 1 << 31}, {"max_bytes": 0xFFFFFFFF}):
        lim = route.plan_limits(**kw)
        assert L.qgcm_send_plan_cpu(64, *args, route._limits_ptr(lim), *outs) == _lib.QGCM_E_ARG, kw
        assert counts.tolist() == [7, 7]
    for kw in ({"max_segs": 1024}, {"max_bytes": 65507}, {"max_seg_len": 0xFFFFFFFF}):  # the bounds themselves
        lim = route.plan_limits(**kw)
        assert L.qgcm_send_plan_cpu(64, *args, route._limits_ptr(lim), *outs) == 0, kw
    assert L.qgcm_send_plan_cpu(64, None, peer.ctypes.data, 2048, None, *outs) == _lib.QGCM_E_ARG
    assert L.qgcm_send_plan_cpu(64, *args, None, order.ctypes.data, None, counts.ctypes.data) == _lib.QGCM_E_ARG
    assert L.qgcm_send_plan_cpu((1 << 31) + 1, *args, None, *outs) == _lib.QGCM_E_ARG
    assert L.qgcm_send_plan_work((1 << 31) + 1) == 0
