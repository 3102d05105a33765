"""CPU: qgcm_train_pack_cpu writes exactly what tests/train_pack_model.py writes -- the packed area, the table and
the counts, over sentinels -- for hand-made plans and for the plans qgcm_send_plan_cpu makes of seeded batches;
a plan that is not well-formed is refused with nothing written."""
import numpy as np
import pytest

import train_pack_model as M
from quantum_amd import _lib, route


def cpu_pack(arena, stride, n, order, trains, m, t, cap, room):
    packed, ptrains, pcounts = M.fresh(n, room)
    rc = _lib.lib().qgcm_train_pack_cpu(arena.ctypes.data, stride, n, order.ctypes.data, m, trains.ctypes.data, t,
                                        packed.ctypes.data, cap, ptrains.ctypes.data, pcounts.ctypes.data)
    return rc, packed, ptrains, pcounts


def check(arena, stride, n, order, trains, packed_cap=None):
    order, trains = np.ascontiguousarray(order, np.uint32), np.ascontiguousarray(trains, np.uint32).reshape(-1, 4)
    m, t = len(order), len(trains)
    assert M.well_formed(stride, n, order, m, trains, t)
    full = M.need(trains)
    cap = full if packed_cap is None else packed_cap
    want_packed = np.full(cap + 64, M.SENTINEL, np.uint8)
    want, (wt, total) = M.pack(arena, stride, n, order, trains, m, t, want_packed, cap)
    assert (wt, total) == (t, full)
    fast_packed = np.full(cap + 64, M.SENTINEL, np.uint8)  # the vectorised model the GPU tests use for large batches
    fast, fast_counts = M.pack_fast(arena, stride, n, order, trains, m, t, fast_packed, cap)
    assert np.array_equal(fast, want) and fast_counts == (t, total) and np.array_equal(fast_packed, want_packed)
    rc, packed, ptrains, pcounts = cpu_pack(arena, stride, n, order, trains, m, t, cap, cap + 64)
    assert rc == 0 and pcounts.tolist() == [t, full]
    assert np.array_equal(ptrains[:t], want)
    assert np.array_equal(packed, want_packed)  # whole: padding zeroed, the bytes behind untouched
    assert np.all(ptrains[t:] == M.PT_SENTINEL) or t == 0
    got, got_bytes = route.train_pack_cpu(arena, stride, n, order, trains, np.zeros(max(cap, 1), np.uint8)[:cap])
    assert got_bytes == full and np.array_equal(got, want)
    return want, want_packed


def test_hand_made_plan():
    """Three trains over six slots of 32 bytes: 3 x 5 bytes, 1 x 32 bytes, 2 x 17 bytes."""
    stride, n = 32, 6
    arena = np.arange(n * stride, dtype=np.uint32).astype(np.uint8)
    order = np.array([4, 0, 2, 5, 3, 1], np.uint32)
    trains = np.array([(0, 3, 7, 5), (3, 1, 8, 32), (4, 2, 9, 17)], np.uint32)
    ptrains, packed = check(arena, stride, n, order, trains)
    assert ptrains.tolist() == [[0, 3, 7, 5], [16, 1, 8, 32], [48, 2, 9, 17]]
    slot = lambda i, L: arena[i * stride:i * stride + L].tolist()
    assert packed[:16].tolist() == slot(4, 5) + slot(0, 5) + slot(2, 5) + [0]
    assert packed[16:48].tolist() == slot(5, 32)
    assert packed[48:96].tolist() == slot(3, 17) + slot(1, 17) + [0] * 14
    assert np.all(packed[96:] == M.SENTINEL)


@pytest.mark.parametrize("stride", (1536, 1388))
def test_edge_batch(stride):
    arena, lens, peer, max_keys = M.edge_batch(stride)
    order, trains = route.send_plan_cpu(lens, peer, max_keys)
    want_order, want_trains = M.plan_of(lens, peer, max_keys)
    assert np.array_equal(order, want_order) and np.array_equal(trains, want_trains)
    ptrains, _ = check(arena, stride, len(lens), order, trains)
    assert np.all(ptrains[:, 0] % 16 == 0)
    # every destination residue mod 16 occurs
    residues = {(k * int(s)) % 16 for _, c, _, s in ptrains.tolist() for k in range(c)}
    assert residues == set(range(16))


def test_random_plans():
    for seed, n, stride, lim in ((0x7A1, 3000, 1536, {}), (0x7A2, 1000, 64, {}), (0x7A3, 2000, 1388, {"max_segs": 7}),
                                 (0x7A4, 900, 1536, {"max_segs": 1})):
        arena, lens, peer, max_keys = M.random_batch(seed, n, stride)
        limits = route.plan_limits(**lim) if lim else None
        order, trains = route.send_plan_cpu(lens, peer, max_keys, limits)
        assert 0 < len(order) < n
        check(arena, stride, n, order, trains)


def test_packed_cap_cuts():
    arena, lens, peer, max_keys = M.random_batch(0xCA7, 400, 1536)
    order, trains = route.send_plan_cpu(lens, peer, max_keys)
    full, _ = check(arena, 1536, 400, order, trains)
    k = len(full) // 2
    start, size = int(full[k, 0]), M.train_bytes(int(full[k, 1]), int(full[k, 3]))
    assert size > 32
    for cap, fitted in ((start, k), (start + size - 1, k), (start + size - 9, k), (start + size, k + 1), (0, 0)):
        ptrains, _ = check(arena, 1536, 400, order, trains, cap)
        assert np.all(ptrains[:fitted, 0] != M.NO_ROOM) and np.all(ptrains[fitted:, 0] == M.NO_ROOM)  # a suffix
        assert np.array_equal(ptrains[:, 1:], full[:, 1:])


def test_malformed_plans_are_refused_with_nothing_written():
    stride, n = 1536, 300
    arena, lens, peer, max_keys = M.random_batch(0xBAD, n, stride, peers=3)
    order, trains = route.send_plan_cpu(lens, peer, max_keys)
    check(arena, stride, n, order, trains)
    cases = [(name, o, tr, m, t) for name, o, tr, m, t, _ in M.malformed_plans(stride, n, order, trains)]
    m, t = len(order), len(trains)
    swapped = trains.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    gap = trains.copy()
    gap[2, 0] += 1
    cases += [("trains-out-of-order", order, swapped, m, t), ("a-gap", order, gap, m, t),
              ("t-above-m", order[:2].copy(), trains[:3].copy(), 2, 3),
              ("trains-short-of-m", order, trains[:-1].copy(), m, t - 1)]
    for name, o, tr, mm, tt in cases:
        assert not M.well_formed(stride, n, o, mm, tr, tt), name
        rc, packed, ptrains, pcounts = cpu_pack(arena, stride, n, o, tr, mm, tt, 1 << 20, 1 << 20)
        assert rc == _lib.QGCM_E_ARG, name
        assert np.all(packed == M.SENTINEL) and np.all(ptrains == M.PT_SENTINEL) and np.all(pcounts == M.COUNT_SENTINEL), name


def test_bad_arguments_and_the_empty_batch():
    L = _lib.lib()
    stride, n = 1536, 100
    arena, lens, peer, max_keys = M.random_batch(0xA46, n, stride)
    order, trains = route.send_plan_cpu(lens, peer, max_keys)
    packed, ptrains, pcounts = M.fresh(n, 1 << 18)
    args = [arena.ctypes.data, stride, n, order.ctypes.data, len(order), trains.ctypes.data, len(trains),
            packed.ctypes.data, packed.size, ptrains.ctypes.data, pcounts.ctypes.data]

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.qgcm_train_pack_cpu(*a)

    assert call(a1=1538) == _lib.QGCM_E_ARG and call(a1=0) == _lib.QGCM_E_ARG
    assert call(a8=(1 << 32) - 15) == _lib.QGCM_E_ARG
    assert call(a2=(1 << 31) + 1) == _lib.QGCM_E_ARG
    for k in (0, 3, 5, 7, 9, 10):
        assert call(**{f"a{k}": None}) == _lib.QGCM_E_ARG, k
    assert np.all(packed == M.SENTINEL) and np.all(ptrains == M.PT_SENTINEL) and np.all(pcounts == M.COUNT_SENTINEL)
    # n == 0, and a batch with nothing sendable: counts {0, 0}, nothing else
    assert call(a0=None, a2=0, a3=None, a4=0, a5=None, a6=0, a7=None, a9=None) == 0 and pcounts.tolist() == [0, 0]
    pcounts[:] = M.COUNT_SENTINEL
    assert call(a4=0, a6=0) == 0 and pcounts.tolist() == [0, 0]
    assert np.all(packed == M.SENTINEL) and np.all(ptrains == M.PT_SENTINEL)
    assert call() == 0 and pcounts[0] == len(trains)
