"""The contract of include/qgcm.h "outgoing frames packed on routed batches" restated in numpy: the frame table,
the unpack with its clamp and its void frames, and -- composed with the outgoing resolve as the header documents
it, the peer always from a dict -- what qgcm_frames_resolve leaves.  Shared by tests/test_frames_model.py (the
host unpack), tests/test_gpu_frames.py (the kernel and the pipeline) and tools/frames_bench.py.
"""
from __future__ import annotations

import numpy as np

from route_model import NO_PEER, OVERHEAD

SENTINEL = 0xA5
LEN_SENTINEL = 0xDEADBEEF
PEER_SENTINEL = 0x0BADF00D
DESC = np.dtype([("off", "<u8"), ("len", "<u4"), ("key", "<u4")])


class Net:
    """table: dict IPtoInt address -> peer; the values router/router.go:21-31 resolves with."""

    def __init__(self, table, net, mask, gateway, own_ip):
        self.table, self.net, self.mask, self.gateway, self.own_ip = dict(table), net, mask, gateway, own_ip


def valid(off: int, length: int, packed_len: int) -> bool:
    return off % 16 == 0 and off + length <= packed_len


def table_ok(frames, packed_len: int) -> bool:
    return all(valid(int(o), int(l), packed_len) for o, l in frames)


def ascends(frames, packed_len: int) -> bool:
    end = 0
    for o, l in frames:
        if not valid(int(o), int(l), packed_len) or int(o) < end:
            return False
        end = int(o) + int(l)
    return True


def fresh(n: int, stride: int):
    """(arena, lens, peer, descs) at their sentinels."""
    descs = np.zeros(max(1, n), DESC)
    descs.view(np.uint8)[:] = SENTINEL
    return (np.full(max(1, n) * stride, SENTINEL, np.uint8), np.full(max(1, n), LEN_SENTINEL, np.uint32),
            np.full(max(1, n), PEER_SENTINEL, np.uint32), descs)


def unpack(packed, packed_len: int, frames, arena, stride: int, lens) -> None:
    """The unpack half as the device does it: a void frame is a packet of length 0 whose slot is untouched."""
    for i, (off, length) in enumerate(np.asarray(frames, np.uint32).reshape(-1, 2).tolist()):
        if not valid(off, length, packed_len):
            lens[i] = 0
            continue
        lens[i] = length
        b = min(length, stride - 4)
        arena[i * stride + 4:i * stride + 4 + b] = packed[off:off + b]


def resolve_outgoing(net: Net, arena, stride: int, lens, peer, descs) -> None:
    """qgcm_resolve_outgoing as include/qgcm.h documents it, divergences included."""
    own = np.frombuffer(net.own_ip.to_bytes(4, "little"), np.uint8)
    for i, length in enumerate(lens.tolist()):
        p = NO_PEER
        if length >= 20 and 4 + length + OVERHEAD <= stride:
            dst = int.from_bytes(arena[i * stride + 20:i * stride + 24].tobytes(), "little")
            key = dst if (dst & net.mask) == (net.net & net.mask) else net.gateway
            p = net.table.get(key, NO_PEER)
            if p != NO_PEER:
                arena[i * stride:i * stride + 4] = own
        peer[i] = p
        descs[i] = (i * stride, length, p)


def frames_resolve(net: Net, packed, packed_len: int, frames, arena, stride: int, lens, peer, descs) -> None:
    """qgcm_frames_resolve: the unpack, then the outgoing resolve (a void frame resolves as the packet of length 0
    it became: QGCM_NO_PEER, descriptor {i * stride, 0, QGCM_NO_PEER})."""
    n = len(frames)
    unpack(packed, packed_len, frames, arena, stride, lens)
    resolve_outgoing(net, arena, stride, lens[:n], peer, descs)


def layout(packets, seed: int = 0, gaps=False):
    """(packed, packed_len, frames): the packets (byte arrays) back to back, each on the next 16-byte boundary
    (`gaps`: now and then one further on), the area filled with seeded junk in between and rounded up to 16 B;
    packed_len = the end of the last frame."""
    rng = np.random.default_rng(0xF4A3E5 + seed)
    frames = np.zeros((len(packets), 2), np.uint32)
    at = end = 0
    for i, p in enumerate(packets):
        if gaps and i % 5 == 3:
            at += 16 * (1 + i % 3)
        frames[i] = (at, len(p))
        end = at + len(p)
        at = (end + 15) & ~15
    packed = rng.integers(0, 256, max(16, at), dtype=np.uint8)
    for (off, length), p in zip(frames.tolist(), packets):
        packed[off:off + length] = p
    return packed, end, frames


def packet(rng, length: int, dst: int | None):
    p = rng.integers(0, 256, length, dtype=np.uint8)
    if dst is not None and length >= 20:
        p[16:20] = np.frombuffer(dst.to_bytes(4, "little"), np.uint8)
    return p


EDGE_LENS = (0, 1, 3, 4, 11, 12, 13, 15, 16, 19, 20, 21, 27, 28, 29, 31, 32, 33, 255, 256, 257, 1350)


def edge_lens(stride: int):
    """... and the longest that seals, one more, the longest a slot holds, one more, and two slots' worth."""
    return EDGE_LENS + (stride - 32, stride - 31, stride - 4, stride - 3, 2 * stride)


def edge_packets(stride: int, dsts, seed: int = 1):
    """Every edge length once per destination of `dsts`, interleaved."""
    rng = np.random.default_rng(0xED6E + seed + stride)
    return [packet(rng, L, d) for L in edge_lens(stride) for d in dsts]


def random_packets(seed: int, n: int, dsts, lens=(20, 21, 64, 700, 1350, 1433)):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(lens), n)
    which = rng.integers(0, len(dsts), n)
    return [packet(rng, lens[pick[i]], dsts[which[i]]) for i in range(n)]
