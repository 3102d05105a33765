"""CPU: qgcm_frames_unpack_cpu (quantum_amd/csrc/frames_core.h) against tests/frames_model.py -- arena and lengths
whole, pre-filled with sentinels, so slot tails, Raw[0:4] and the bytes behind a short frame are proven untouched
-- and every class of table it refuses, with nothing written."""
import numpy as np
import pytest

import frames_model as M
from quantum_amd import _lib, route


def run(packed, packed_len, frames, stride):
    n = len(frames)
    arena, lens, _, _ = M.fresh(n, stride)
    want_arena, want_lens, _, _ = M.fresh(n, stride)
    route.frames_unpack_cpu(packed, packed_len, frames, arena, stride, lens)
    M.unpack(packed, packed_len, frames, want_arena, stride, want_lens)
    assert np.array_equal(lens, want_lens)
    if not np.array_equal(arena, want_arena):
        at = np.flatnonzero(arena != want_arena)
        raise AssertionError(f"{at.size} bytes differ, the first in slot {int(at[0]) // stride} at byte {int(at[0]) % stride}")
    return arena, lens


def test_a_hand_table():
    """Three frames, one of them empty, the second behind a gap: slot i is frame i, at Raw[4:]."""
    packed = np.arange(96, dtype=np.uint8)
    frames = np.array([(0, 5), (32, 0), (64, 30)], np.uint32)
    arena, lens = run(packed, 94, frames, 40)
    assert lens.tolist() == [5, 0, 30]
    assert arena[4:9].tolist() == [0, 1, 2, 3, 4] and np.all(arena[9:40] == M.SENTINEL) and np.all(arena[:4] == M.SENTINEL)
    assert np.all(arena[40:80] == M.SENTINEL)
    assert arena[84:114].tolist() == list(range(64, 94)) and np.all(arena[114:] == M.SENTINEL)


def test_a_long_frame_is_clamped_to_the_slot_and_keeps_its_length():
    packed = np.arange(64, dtype=np.uint8)
    arena, lens = run(packed, 64, np.array([(0, 20), (16, 48)], np.uint32), 24)  # frames may overlap here
    assert lens.tolist() == [20, 48]
    assert arena[24 + 4:48].tolist() == list(range(16, 36))


@pytest.mark.parametrize("stride", (1536, 1388, 64))
def test_edge_lengths(stride):
    packed, packed_len, frames = M.layout(M.edge_packets(stride, (None,)), stride)
    run(packed, packed_len, frames, stride)


@pytest.mark.parametrize("seed", range(4))
def test_seeded_tables(seed):
    packets = M.random_packets(0x5EED + seed, 300 + seed, (None,), lens=(0, 1, 19, 64, 333, 1350, 1433, 3000))
    packed, packed_len, frames = M.layout(packets, seed, gaps=True)
    run(packed, packed_len, frames, (1472, 1388, 64, 1536)[seed])


def test_every_invalid_class_is_refused_with_nothing_written():
    L = _lib.lib()
    packets = M.random_packets(7, 9, (None,), lens=(64, 100))
    packed, packed_len, frames = M.layout(packets)
    assert M.table_ok(frames, packed_len)
    bad = {
        "off-not-on-16": (4, (int(frames[4, 0]) + 4, 8)),
        "one-past-the-end": (8, (int(frames[8, 0]), int(frames[8, 1]) + 1)),
        "off-past-the-end": (2, ((packed_len + 15) & ~15, 1)),
        "wraps-32-bits": (5, (0xFFFFFFF0, 0x20)),
        "len-all-ones": (0, (0, 0xFFFFFFFF)),
    }
    for name, (i, f) in bad.items():
        t = frames.copy()
        t[i] = f
        assert not M.table_ok(t, packed_len), name
        arena, lens, _, _ = M.fresh(len(t), 256)
        rc = L.qgcm_frames_unpack_cpu(packed.ctypes.data, packed_len, t.ctypes.data, len(t), arena.ctypes.data, 256,
                                      lens.ctypes.data)
        assert rc == _lib.QGCM_E_ARG, name
        assert np.all(arena == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL), name
    # a frame that ends exactly at packed_len is valid
    assert int(frames[-1, 0]) + int(frames[-1, 1]) == packed_len
    run(packed, packed_len, frames, 256)


def test_argument_errors():
    L = _lib.lib()
    packed, packed_len, frames = M.layout(M.random_packets(8, 3, (None,), lens=(64,)))
    arena, lens, _, _ = M.fresh(3, 128)
    good = [packed.ctypes.data, packed_len, frames.ctypes.data, 3, arena.ctypes.data, 128, lens.ctypes.data]
    for k in (0, 2, 4, 6):
        a = list(good)
        a[k] = None
        assert L.qgcm_frames_unpack_cpu(*a) == _lib.QGCM_E_ARG, k
    for stride in (0, 4, 130):
        a = list(good)
        a[5] = stride
        assert L.qgcm_frames_unpack_cpu(*a) == _lib.QGCM_E_ARG, stride
    a = list(good)
    a[3] = (1 << 31) + 1
    assert L.qgcm_frames_unpack_cpu(*a) == _lib.QGCM_E_ARG
    assert np.all(arena == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL)
    assert L.qgcm_frames_unpack_cpu(None, 0, None, 0, None, 128, None) == 0
    assert L.qgcm_frames_unpack_cpu(*good) == 0


def test_binding():
    assert {"qgcm_tun_read_packed", "qgcm_frames_resolve", "qgcm_frames_unpack_cpu",
            "qgcm_route_chain_seal_frames_host"} <= set(_lib.EXPORTS)
    import ctypes as C

    assert C.sizeof(_lib.Frame) == 8 and _lib.Frame.off.offset == 0 and _lib.Frame.len.offset == 4
