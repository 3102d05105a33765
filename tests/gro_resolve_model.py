"""The contract of qgcm_gro_resolve (include/qgcm.h "coalesced receive on routed batches") restated in numpy:
the unpack of tests/gro_model.py, then the incoming resolve as the header documents it, the peer always from a
dict.  A slot no unskipped buffer names keeps its length and bytes and is resolved from them; without a table the
call is the incoming resolve alone.  Shared by tests/test_gro_resolve_model.py, tests/test_gpu_gro_resolve.py and
tools/gro_resolve_bench.py.
"""
from __future__ import annotations

import numpy as np

import gro_model as G
from frames_model import DESC, LEN_SENTINEL, PEER_SENTINEL, SENTINEL, Net, fresh  # noqa: F401 (fresh: re-exported)
from route_model import NO_PEER


def lookup(net: Net, addr: int) -> int:
    key = addr if (addr & net.mask) == (net.net & net.mask) else net.gateway  # router/router.go:25-30
    return net.table.get(key, NO_PEER)


def resolve_incoming(net: Net, arena, stride: int, n: int, lens, peer, descs) -> None:
    """qgcm_resolve_incoming: readable when 4 <= L <= stride, the sender in Raw[0:4]."""
    for i in range(n):
        L = int(lens[i])
        p = NO_PEER
        if 4 <= L <= stride:
            p = lookup(net, int.from_bytes(arena[i * stride:i * stride + 4].tobytes(), "little"))
        peer[i] = p
        descs[i] = (i * stride, L - 4 if L >= 4 else 0, p)


def gro_resolve(net: Net, packed, packed_len: int, bufs, n: int, arena, stride: int, lens, peer, descs) -> None:
    """In place, over whatever arena, lens, peer and descs held before."""
    G.unpack(packed, packed_len, bufs, n, arena, stride, lens)
    resolve_incoming(net, arena, stride, n, lens, peer, descs)


def plant(packed, bufs, srcs, seed: int = 0):
    """A sender address into the first four bytes of every datagram of `bufs` with L >= 4 that lies inside
    `packed`, cycling through `srcs` (a hit, an in-net miss, an out-of-net address) from `seed` on.  In place;
    returns packed."""
    at = seed
    for b in bufs:
        for _, src, L in G.datagrams(b):
            if L >= 4 and src + 4 <= packed.size:
                packed[src:src + 4] = np.frombuffer(int(srcs[at % len(srcs)]).to_bytes(4, "little"), np.uint8)
                at += 1
    return packed
