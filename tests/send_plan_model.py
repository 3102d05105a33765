"""The send plan's contract (include/qgcm.h "send plan on routed batches") in plain Python: a sort by
(peer, index), itertools.groupby over (peer, length), and the chop into trains.  The only expected-value
source of the send-plan tests; it never calls the library."""
from itertools import groupby

DEFAULTS = (64, 65507, 65507)  # max_segs, max_seg_len, max_bytes


def limits(max_segs=0, max_seg_len=0, max_bytes=0):
    """A zero field takes its default."""
    return tuple(v or d for v, d in zip((max_segs, max_seg_len, max_bytes), DEFAULTS))


def cap(length, lim):
    max_segs, max_seg_len, max_bytes = lim
    return 1 if length > max_seg_len else max(1, min(max_segs, max_bytes // length))


def plan(lens, peer, max_keys, lim=DEFAULTS):
    """-> (order, trains): order a list of indices, trains a list of (first, count, peer, seg_len)."""
    order = sorted((i for i in range(len(lens)) if peer[i] < max_keys and lens[i] != 0), key=lambda i: (peer[i], i))
    trains, pos = [], 0
    for (p, length), run in groupby(order, key=lambda i: (int(peer[i]), int(lens[i]))):
        r, c = len(list(run)), cap(length, lim)
        for first in range(pos, pos + r, c):
            trains.append((first, min(c, pos + r - first), p, length))
        pos += r
    return [int(i) for i in order], trains


# ---- batches shared by the CPU and the GPU tests ----
NO_PEER = 0xFFFFFFFF
TILE = 256  # positions per workgroup of the device scan (plan_kernels.hip kPlanTile): the edges sit around it


def random_batch(seed, n, peers, max_keys, lengths=(36, 700, 1382), junk=0.1):
    """n packets on `peers` key slots spread over [0, max_keys) (max_keys - 1 among them), lengths drawn from
    `lengths`; a share `junk` of them unsendable: length 0, peer NO_PEER, peer >= max_keys."""
    import numpy as np

    rng = np.random.default_rng(seed)
    slots = np.unique(np.concatenate([[max_keys - 1], rng.integers(0, max_keys, max(0, peers - 1))])).astype(np.uint32)
    peer = slots[rng.integers(0, len(slots), n)]
    lens = np.asarray(lengths, np.uint32)[rng.integers(0, len(lengths), n)]
    bad = rng.random(n) < junk
    kind = rng.integers(0, 3, n)
    lens = np.where(bad & (kind == 0), 0, lens).astype(np.uint32)
    peer = np.where(bad & (kind == 1), NO_PEER, peer).astype(np.uint32)
    peer = np.where(bad & (kind == 2), max_keys + rng.integers(0, 5, n), peer).astype(np.uint32)
    return lens, peer


def edge_cases(max_keys):
    """(name, lens, peer, limits keywords): the shapes at which a tiled scan of 256 positions can go wrong."""
    import numpy as np

    u32 = lambda v: np.asarray(v, np.uint32)
    full = lambda n, v: np.full(n, v, np.uint32)
    out = []
    for n in (1, 63, 64, 65, 257, 4099):
        for peers in (1, 3, 1024):
            out.append((f"random-n{n}-p{peers}", *random_batch(1000 * n + peers, n, peers, max_keys), {}))
    n = 4099
    out.append(("one-peer-1382-cap47", full(n, 1382), full(n, 5), {}))
    out.append(("one-peer-max-segs-7", full(n, 1382), full(n, 5), {"max_segs": 7}))
    out.append(("one-peer-100-cap64", full(n, 100), full(n, max_keys - 1), {"max_segs": 64}))
    for head in (TILE, TILE - 1):  # a run head exactly at the tile edge and just before it
        lens = np.concatenate([full(head, 700), full(600 - head, 36)])
        out.append((f"run-head-at-{head}", lens, full(600, 2), {}))
        peer = np.concatenate([full(head, 1), full(600 - head, 2)])
        out.append((f"peer-head-at-{head}", full(600, 700), peer, {}))
    # one run, and with max_segs 1024 at 20 bytes one train, across three tiles
    out.append(("one-train-three-tiles", full(700, 20), full(700, 9), {"max_segs": 1024}))
    out.append(("one-run-three-tiles", full(700, 1382), full(700, 9), {}))
    out.append(("nothing-sendable", u32([0, 100, 0, 7] * 80), u32([1, NO_PEER, 2, max_keys] * 80), {}))
    out.append(("only-last-sendable", u32([0] * 299 + [64]), u32([3] * 300), {}))
    out.append(("only-first-sendable", u32([64] + [0] * 299), u32([3] * 300), {}))
    lens, peer = random_batch(77, 1000, 3, max_keys, junk=0.5)
    out.append(("half-unsendable", lens, peer, {}))
    lens = u32([1400, 1200, 1400, 1200, 900, 900, 900] * 60)
    out.append(("above-max-seg-len", lens, full(len(lens), 4), {"max_seg_len": 1300}))
    out.append(("above-max-bytes", lens, full(len(lens), 4), {"max_bytes": 1000}))
    out.append(("max-segs-1", *random_batch(78, 777, 3, max_keys), {"max_segs": 1}))
    return out
