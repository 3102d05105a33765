"""CPU: qgcm_gro_unpack_cpu (quantum_amd/csrc/gro_core.h) writes exactly what tests/gro_model.py writes --
the whole arena and all lengths, sentinels included -- and refuses tables whose `first` values are not the
exclusive prefix sums of their counts."""
import numpy as np
import pytest

import gro_model as M
from quantum_amd import _lib, route


def both(packed, packed_len, bufs, n, stride):
    want_arena, want_lens = M.fresh(n, stride)
    M.unpack(packed, packed_len, bufs, n, want_arena, stride, want_lens)
    arena, lens = M.fresh(n, stride)
    route.gro_unpack_cpu(packed, packed_len, bufs, n, arena, stride, lens)
    return (arena, lens), (want_arena, want_lens)


@pytest.mark.parametrize("stride", (1536, 1388))
def test_edges(stride):
    packed, packed_len, bufs, n = M.edge_case(stride)
    assert M.table_ok(bufs, n)
    (arena, lens), (want_arena, want_lens) = both(packed, packed_len, bufs, n, stride)
    assert np.array_equal(lens, want_lens)
    assert np.array_equal(arena, want_arena)
    # the model itself: lengths beyond the stride are kept, and some slot tail kept its sentinel
    assert lens.max() == stride + 1 and np.any(arena.reshape(n, stride)[:, -1] == M.SENTINEL)


@pytest.mark.parametrize("lone_len", (None, 64))
def test_random_batch(lone_len):
    packed, packed_len, bufs, n = M.random_batch(77, 3001, lone_len)
    (arena, lens), (want_arena, want_lens) = both(packed, packed_len, bufs, n, 1472)
    assert np.array_equal(lens, want_lens) and np.array_equal(arena, want_arena)


def test_buffer_past_the_packed_area_is_skipped_whole():
    packed, packed_len, bufs, n = M.layout([(300, 100, 1), (500, 100, 2), (64, 0, 3)], 5)
    short = int(bufs[1][0]) + 499  # the middle buffer reaches one byte past it, the last one lies wholly behind
    (arena, lens), (want_arena, want_lens) = both(packed, short, bufs, n, 128)
    assert np.array_equal(lens, want_lens) and np.array_equal(arena, want_arena)
    assert lens.tolist() == [100] * 3 + [M.LEN_SENTINEL] * 6
    assert np.all(arena[3 * 128:] == M.SENTINEL)


def test_tables_that_are_not_prefix_sums_are_refused():
    packed, packed_len, bufs, n = M.layout([(300, 100, 0), (77, 0, 0), (200, 100, 0)], 6)
    assert n == 6 and M.table_ok(bufs, n)
    arena, lens = M.fresh(n + 2, 128)

    def rc(b, m):
        b = np.ascontiguousarray(b, np.uint32)
        return _lib.lib().qgcm_gro_unpack_cpu(packed.ctypes.data, packed_len, b.ctypes.data, len(b), m, arena.ctypes.data,
                                              128, lens.ctypes.data)

    assert rc(bufs, n) == 0
    arena[:], lens[:] = M.SENTINEL, M.LEN_SENTINEL
    for what, m in (("first", n), ("gap", n), ("swap", n), ("short", n - 1), ("long", n + 1), ("none", n)):
        bad = bufs.copy()
        if what == "first":
            bad[0, 3] = 1
        elif what == "gap":
            bad[2, 3] += 1
        elif what == "swap":
            bad = bad[[1, 0, 2]]
        elif what == "none":
            bad = bad[:0]
        assert not M.table_ok(bad, m)
        assert rc(bad, m) == _lib.QGCM_E_ARG, what
    assert np.all(arena == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL)
    # more buffers than datagrams, a stride that is no multiple of 4, NULL arrays
    L = _lib.lib()
    assert L.qgcm_gro_unpack_cpu(packed.ctypes.data, packed_len, bufs.ctypes.data, 3, 2, arena.ctypes.data, 128,
                                 lens.ctypes.data) == _lib.QGCM_E_ARG
    assert L.qgcm_gro_unpack_cpu(packed.ctypes.data, packed_len, bufs.ctypes.data, 3, n, arena.ctypes.data, 126,
                                 lens.ctypes.data) == _lib.QGCM_E_ARG
    assert L.qgcm_gro_unpack_cpu(None, packed_len, bufs.ctypes.data, 3, n, arena.ctypes.data, 128,
                                 lens.ctypes.data) == _lib.QGCM_E_ARG
    assert L.qgcm_gro_unpack_cpu(None, 0, None, 0, 0, None, 128, None) == 0
