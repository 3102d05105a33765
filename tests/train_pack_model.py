"""The train pack of include/qgcm.h ("planned trains packed on routed batches") restated in numpy: which train is
void, a train's bytes, the table, the counts, the cut at packed_cap and the rules for a malformed plan; and the
inputs the CPU and GPU tests share.  It never calls the library."""
import numpy as np

import send_plan_model as P

SENTINEL = 0x5A              # packed bytes before a pack
PT_SENTINEL = 0xC0FFEE22     # ptrains words before a pack
COUNT_SENTINEL = 0x0123456789ABCDEF
NO_ROOM = 0xFFFFFFFF         # `off` of a train that did not fit, or is void
MAX_COUNT = 1024


def void(first: int, count: int, seg_len: int, m: int, stride: int) -> bool:
    return not 1 <= count <= MAX_COUNT or not 1 <= seg_len <= stride or first + count > m


def train_bytes(count: int, seg_len: int) -> int:
    return (count * seg_len + 15) & ~15


def well_formed(stride: int, n: int, order, m: int, trains, t: int) -> bool:
    """What qgcm_train_pack_cpu asks of a plan before it writes anything."""
    if m > n or t > m:
        return False
    at = 0
    for first, count, _, seg_len in np.asarray(trains, np.int64).reshape(-1, 4)[:t].tolist():
        if first != at or void(first, count, seg_len, m, stride):
            return False
        at += count
    return at == m and all(int(x) < n for x in order[:m])


def pack(arena, stride: int, n: int, order, trains, m: int, t: int, packed, packed_cap: int):
    """The device's rules, which are the host's on a well-formed plan.  In place into `packed` (a flat uint8 array)
    -> (ptrains (t, 4) uint32 of off, count, peer, seg_len; pcounts (t, bytes)).  m and t are clamped to n; a void
    train has size 0 and off NO_ROOM; a member with order[p] >= n is seg_len zero bytes."""
    m, t = min(m, n), min(t, n)
    out, at = [], 0
    for first, count, peer, seg_len in np.asarray(trains, np.int64).reshape(-1, 4)[:t].tolist():
        if void(first, count, seg_len, m, stride):
            out.append((NO_ROOM, count, peer, seg_len))
            continue
        R = train_bytes(count, seg_len)
        fits = at + R <= packed_cap
        out.append((at if fits else NO_ROOM, count, peer, seg_len))
        if fits:
            for k in range(count):
                slot = int(order[first + k])
                d = at + k * seg_len
                packed[d:d + seg_len] = arena[slot * stride:slot * stride + seg_len] if slot < n else 0
            packed[at + count * seg_len:at + R] = 0
        at += R
    return np.array(out, np.uint32).reshape(-1, 4), (t, at)


def pack_fast(arena, stride: int, n: int, order, trains, m: int, t: int, packed, packed_cap: int):
    """pack() for the large batches, vectorised, for well-formed plans only: the datagrams of one seg_len are
    gathered and scattered together.  tests/test_train_pack_model.py holds it equal to pack()."""
    tr = np.asarray(trains, np.int64).reshape(-1, 4)[:t]
    first, count, seg = tr[:, 0], tr[:, 1], tr[:, 3]
    R = (count * seg + 15) & ~15
    end = np.cumsum(R)
    off = end - R
    fits = end <= packed_cap
    ptrains = np.stack([np.where(fits, off, NO_ROOM), count, tr[:, 2], seg], axis=1).astype(np.uint32)
    which = np.repeat(np.arange(t), count)              # the train of every position
    k = np.arange(int(count.sum())) - first[which]
    dst = off[which] + k * seg[which]
    slot = np.asarray(order[:m]).astype(np.int64)
    live = fits[which]
    for size in np.unique(seg[fits]):
        sel = np.flatnonzero(live & (seg[which] == size))
        for lo in range(0, len(sel), 1 << 16):
            s = sel[lo:lo + (1 << 16)]
            cols = np.arange(size)
            packed[dst[s][:, None] + cols[None, :]] = arena[(slot[s] * stride)[:, None] + cols[None, :]]
    for j in np.flatnonzero(fits & (count * seg != R)):  # the zero padding
        packed[off[j] + count[j] * seg[j]:end[j]] = 0
    return ptrains.reshape(-1, 4), (t, int(end[-1]) if t else 0)


def fresh(n: int, packed_bytes: int):
    """A packed area, a table and counts full of sentinels: whatever a pack does not name must keep them."""
    return (np.full(packed_bytes, SENTINEL, np.uint8), np.full((max(1, n), 4), PT_SENTINEL, np.uint32),
            np.full(2, COUNT_SENTINEL, np.uint64))


def need(trains) -> int:
    """bytes of the whole pack of a well-formed plan."""
    tr = np.asarray(trains, np.int64).reshape(-1, 4)
    return int(np.sum((tr[:, 1] * tr[:, 3] + 15) & ~15))


def arena_of(seed: int, n: int, stride: int):
    return np.random.default_rng(seed).integers(0, 256, n * stride, dtype=np.uint8)


def plan_of(lens, peer, max_keys: int, **lim):
    """The plan of tests/send_plan_model.py as arrays -> (order (m) uint32, trains (t, 4) uint32)."""
    order, trains = P.plan(lens, peer, max_keys, P.limits(**lim))
    return np.array(order, np.uint32), np.array(trains, np.uint32).reshape(-1, 4)


# ---- batches shared by the CPU and the GPU tests ----
EDGE_SEGS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 256, 257, 1381, 1382, 1383, 1472)
EDGE_COUNTS = (1, 2, 3, 16, 17, 64)


def edge_batch(stride: int, seed: int = 0xED6E):
    """Every seg_len of EDGE_SEGS that a slot of `stride` bytes holds (and `stride` itself) times every count of
    EDGE_COUNTS: one peer per pair, its `count` datagrams of seg_len bytes scattered over the batch by a seeded
    shuffle, so that peers interleave and a train's sources lie far apart.  Every train starts on a 16-B boundary
    and datagram k at k * seg_len behind it, so with 16 and more datagrams of an odd length every destination
    residue mod 16 occurs; with seg_len <= 5 three and more datagrams share one granule.  A run longer than
    cap(seg_len) is cut into several trains by the plan.  -> (arena, lens, peer, max_keys)."""
    segs = sorted({s for s in EDGE_SEGS if s <= stride} | {stride})
    lens, peer = [], []
    for c, (seg, count) in enumerate((s, k) for s in segs for k in EDGE_COUNTS):
        lens += [seg] * count
        peer += [c] * count
    rng = np.random.default_rng(seed + stride)
    shuffle = rng.permutation(len(lens))
    lens, peer = np.array(lens, np.uint32)[shuffle], np.array(peer, np.uint32)[shuffle]
    return arena_of(seed + stride + 1, len(lens), stride), lens, peer, len(segs) * len(EDGE_COUNTS)


def random_batch(seed: int, n: int, stride: int = 1536, peers: int = 7, lengths=(36, 60, 700, 1382, 1383), junk=0.1):
    """n packets of `peers` peers with lengths drawn from `lengths`, a share of them unsendable.
    -> (arena, lens, peer, max_keys)."""
    max_keys = max(peers, 16)
    lens, peer = P.random_batch(seed, n, peers, max_keys, tuple(x for x in lengths if x <= stride), junk)
    return arena_of(seed + 1, n, stride), lens, peer, max_keys


def malformed_plans(stride: int, n: int, order, trains):
    """(name, order, trains, m, t, tiles) for every class of plan that is not well-formed, made from a well-formed
    one of at least four trains whose third has more than one datagram.  With `tiles` the `first` values still
    ascend and the valid trains keep their positions, so the device's packed bytes are determined; without it only
    the table, the counts and the bounds are."""
    order, trains = np.array(order, np.uint32), np.array(trains, np.uint32).reshape(-1, 4)
    m, t = len(order), len(trains)
    assert t >= 4 and trains[2, 1] > 1 and m < n
    out = []

    def add(name, o=order, tr=trains, mm=m, tiles=True):
        out.append((name, o.copy(), tr.copy(), mm, t, tiles))

    o = order.copy()
    o[int(trains[2, 0]) + 1] = n
    add("order-at-n", o)
    o[int(trains[2, 0])] = 0xFFFFFFFF
    add("order-wraps", o)
    for name, field, value in (("count-0", 1, 0), ("count-1025", 1, 1025), ("seg-len-0", 3, 0),
                               ("seg-len-past-stride", 3, stride + 4)):
        tr = trains.copy()
        tr[2, field] = value
        add(name, tr=tr)
    tr = trains.copy()
    tr[-1, 1] += 1
    add("last-train-past-m", tr=tr)
    tr = trains.copy()
    tr[1, 0] = 0xFFFFFFFF  # first + count wraps 32 bits
    add("first-wraps", tr=tr, tiles=False)
    add("m-above-n", mm=n + 5)
    return out
