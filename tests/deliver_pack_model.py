"""The delivered-packet pack of include/qgcm.h ("delivered packets packed on routed batches") restated in
numpy: which packet is delivered, its record, the table, the counts and the cut at packed_cap; and the inputs
the CPU and GPU tests share."""
import numpy as np

SENTINEL = 0x5A              # packed bytes before a pack
REC_SENTINEL = 0xC0FFEE11    # recs words before a pack
COUNT_SENTINEL = 0x0123456789ABCDEF
NO_ROOM = 0xFFFFFFFF         # `off` of a record that did not fit


def delivered(status, length: int, stride: int) -> bool:
    return status == 1 and 4 + length <= stride


def rec_bytes(length: int) -> int:
    return (4 + length + 15) & ~15


def pack(arena, stride: int, n: int, lens, peer, status, packed, packed_cap: int):
    """In place into `packed` (a flat uint8 array, at least min(packed_cap, need) long) -> (recs (m, 4) uint32 of
    off, len, slot, peer; counts (m, bytes))."""
    recs, at = [], 0
    for i in range(n):
        L = int(lens[i])
        if not delivered(1 if status is None else int(status[i]), L, stride):
            continue
        R = rec_bytes(L)
        fits = at + R <= packed_cap
        recs.append((at if fits else NO_ROOM, L, i, int(peer[i])))
        if fits:
            packed[at:at + 4 + L] = arena[i * stride:i * stride + 4 + L]
            packed[at + 4 + L:at + R] = 0
        at += R
    return np.array(recs, np.uint32).reshape(-1, 4), (len(recs), at)


def pack_fast(arena, stride: int, n: int, lens, peer, status, packed, packed_cap: int):
    """pack() for the large batches, vectorised: the records of one size R are gathered and scattered together.
    tests/test_deliver_pack_model.py holds it equal to pack()."""
    L = lens[:n].astype(np.int64)
    ok = 4 + L <= stride
    if status is not None:
        ok &= status[:n] == 1
    slot = np.flatnonzero(ok)
    L = L[slot]
    R = (4 + L + 15) & ~15
    end = np.cumsum(R)
    off = end - R
    fits = end <= packed_cap
    recs = np.stack([np.where(fits, off, NO_ROOM), L, slot, peer[:n][slot].astype(np.int64)], axis=1).astype(np.uint32)
    for size in np.unique(R[fits]):
        sel = np.flatnonzero(fits & (R == size))
        cols = np.arange(size)
        # the padding may lie past the slot (a stride that is no multiple of 16): read inside it, then zero
        rows = arena[(slot[sel] * stride)[:, None] + np.minimum(cols, stride - 1)[None, :]]
        rows[cols[None, :] >= (4 + L[sel])[:, None]] = 0
        packed[off[sel][:, None] + cols[None, :]] = rows
    return recs.reshape(-1, 4), (len(slot), int(end[-1]) if len(slot) else 0)


def fresh(n: int, packed_bytes: int):
    """A packed area, a table and counts full of sentinels: whatever a pack does not name must keep them."""
    return (np.full(packed_bytes, SENTINEL, np.uint8), np.full((max(1, n), 4), REC_SENTINEL, np.uint32),
            np.full(2, COUNT_SENTINEL, np.uint64))


def need(lens, status, stride: int) -> int:
    """bytes of the whole pack."""
    L = np.asarray(lens).astype(np.int64)
    ok = 4 + L <= stride
    if status is not None:
        ok &= np.asarray(status) == 1
    return int(np.sum((4 + L[ok] + 15) & ~15))


def arena_of(seed: int, n: int, stride: int):
    return np.random.default_rng(seed).integers(0, 256, n * stride, dtype=np.uint8)


def edge_case(stride: int):
    """About 40 packets: every length around the 4- and 16-byte pieces and the slot's end, the ways a packet is
    left out (status 0 with a garbage length, status 2, a status-1 length one past the slot, one whose 4 + L
    wraps 32 bits), the first and the last packet dropped.  -> (arena, lens, peer, status)."""
    rows = [(0, 0xDEAD0000)]                      # the first packet dropped, its length garbage
    for L in (0, 1, 11, 12, 13, 27, 28, 29, 1382, stride - 5, stride - 4):
        rows.append((1, L))
    rows += [(1, stride - 3),                     # 4 + L == stride + 1: left out
             (1, 0xFFFFFFFF), (1, 0xFFFFFFFC),    # 4 + L wraps: left out
             (2, 100), (0, 64), (255, 7)]
    for L in (12, 0, 1382, 1, stride - 4, 13, 11, 0):   # neighbours of every size on both sides
        rows += [(1, L), (0, stride * 3)]
    rows += [(1, 500), (1, 28), (0, 0)]           # the last packet dropped
    n = len(rows)
    status = np.array([r[0] for r in rows], np.uint8)
    lens = np.array([r[1] for r in rows], np.uint32)
    peer = ((np.arange(n, dtype=np.uint64) * 2654435761) & 0xFFFFFFFF).astype(np.uint32)
    assert 36 <= n <= 48 and status[0] != 1 and status[-1] != 1
    return arena_of(0xDE1 + stride, n, stride), lens, peer, status


def random_batch(seed: int, n: int, stride: int = 1536, max_len: int = 1500, drop: float = 0.1, with_status=True):
    """n packets of seeded random lengths in 0..max_len, a fraction `drop` of them dropped (status 0, or 2 now and
    then).  -> (arena, lens, peer, status or None)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n).astype(np.uint32)
    peer = rng.integers(0, 1 << 20, n).astype(np.uint32)
    status = None
    if with_status:
        status = np.ones(n, np.uint8)
        dropped = rng.random(n) < drop
        status[dropped] = np.where(rng.random(int(dropped.sum())) < 0.2, 2, 0)
    return arena_of(seed + 1, n, stride), lens, peer, status
