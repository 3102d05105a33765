"""Plain models of the route table and the link metrics (include/qgcm.h "routes resolved on the GPU"), shared
by tests/test_route_model.py and tests/test_gpu_route_edges.py.

route_sums is the yardstick of the accounting tests: the header's counter table in numpy, exact in uint64, fast
enough for a million packets.  py_route_hash / build_table / probe_path restate how the library places and
finds an address; the GPU tests use them only to CHOOSE inputs (addresses that collide, tables that wrap past
the last slot) and to assert that the chosen inputs still do what they were chosen for -- never to compute an
expected peer, which always comes from a dict.
"""
from __future__ import annotations

import numpy as np

NO_PEER = 0xFFFFFFFF
TX, RX = 0, 1
OVERHEAD = 28  # tag and nonce


def route_sums(direction, peer, lens, status, max_keys):
    """(totals, links): the uint64 rows [Packets, Bytes, DroppedPackets, DroppedBytes] one qgcm_route_account
    call adds -- `totals` of shape (4,), `links` of shape (max_keys, 4).  `peer` / `lens` are the d_peer values
    and the descriptor lengths (uint32), `status` the status bytes or None (every resolved packet delivered)."""
    peer = np.asarray(peer, np.uint32)
    lens = np.asarray(lens, np.uint32).astype(np.uint64)
    n = len(peer)
    resolved = peer < np.uint32(max_keys)  # QGCM_NO_PEER and every other value at or above max_keys: unresolved
    ok = resolved.copy() if status is None else resolved & (np.asarray(status, np.uint8) == 1)
    if direction == RX:
        ok &= lens >= OVERHEAD  # shorter than tag and nonce: dropped whatever its status
    drop = resolved & ~ok
    four, oh, zero = np.uint64(4), np.uint64(OVERHEAD), np.uint64(0)
    if direction == TX:
        by = np.where(ok, four + lens + oh, zero)
    else:
        by = np.where(ok, four + np.where(ok, lens, oh) - oh, zero)  # never below zero: ok has len >= 28
    db = np.where(drop, four + lens, zero)
    cols = np.stack([ok.astype(np.uint64), by, drop.astype(np.uint64), db], axis=1)
    links = np.zeros((max_keys, 4), np.uint64)
    np.add.at(links, peer[resolved].astype(np.int64), cols[resolved])
    totals = cols.sum(axis=0, dtype=np.uint64)
    totals[2] += np.uint64(n - int(resolved.sum()))  # unresolved: one dropped packet, bytes 0, no link
    return totals, links


# ---- where the library puts an address (input selection only) ----

def py_route_hash(ip: int) -> int:
    h = (ip * 0x9E3779B1) & 0xFFFFFFFF
    return h ^ (h >> 15)


def capacity(count: int) -> int:
    cap = 2
    while cap < 2 * count:
        cap <<= 1
    return cap


def build_table(pairs):
    """(slots, wrapped): the open-addressing table of `pairs` ((ip, peer) in insertion order; a repeated ip
    overwrites) as a list of (ip, peer) or None, and whether an insertion stepped from the last slot to slot 0."""
    cap = capacity(len(pairs))
    slots, wrapped = [None] * cap, False
    for ip, peer in pairs:
        h = py_route_hash(ip) & (cap - 1)
        while slots[h] is not None and slots[h][0] != ip:
            wrapped |= h == cap - 1
            h = (h + 1) & (cap - 1)
        slots[h] = (ip, peer)
    return slots, wrapped


def probe_path(slots, ip):
    """The slots a lookup of `ip` reads, in order, up to its hit or the first empty entry."""
    cap, path = len(slots), []
    h = py_route_hash(ip) & (cap - 1)
    for _ in range(cap):
        path.append(h)
        if slots[h] is None or slots[h][0] == ip:
            break
        h = (h + 1) & (cap - 1)
    return path


def crosses_seam(path) -> bool:
    return any(b < a for a, b in zip(path, path[1:]))


SWEEP_TABLES = 64


def sweep_case(k: int):
    """Table k of the random-address sweep: (dict of 1 ... 8 routes on random 32-bit addresses, the 256
    addresses of its batch -- mapped ones at even places, random misses at odd ones --, an unmapped gateway)."""
    import random

    rng = random.Random(0x5EE9 + k)
    count = 1 + k % 8
    t = {}
    while len(t) < count:
        t[rng.getrandbits(32)] = rng.randrange(2048)
    keys = list(t)
    addrs = []
    for i in range(256):
        a = rng.choice(keys)
        while i % 2 and a in t:
            a = rng.getrandbits(32)
        addrs.append(a)
    return t, addrs, rng.getrandbits(32)


def sweep_wraps(k: int) -> bool:
    """Whether building table k, or looking one of its batch's addresses up, steps from the last slot to slot 0."""
    t, addrs, _ = sweep_case(k)
    slots, wrapped = build_table(list(t.items()))
    return wrapped or any(crosses_seam(probe_path(slots, a)) for a in addrs)
