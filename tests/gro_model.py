"""The coalesced receive of include/qgcm.h ("coalesced receive on routed batches") restated in numpy: the
count of a buffer, the skip rule, the unpack and the table check of the host entry points; and the inputs the
CPU and GPU tests share."""
import socket
import struct

import numpy as np

UDP_SEGMENT, UDP_GRO = 103, 104  # linux/udp.h

SENTINEL = 0xA5          # arena bytes before an unpack
LEN_SENTINEL = 0xDEADBEEF  # lens before an unpack


def count(length: int, seg_len: int) -> int:
    if seg_len == 0 or seg_len >= length:
        return 1
    return -(-length // seg_len)


def datagrams(buf):
    """(slot, source offset, L) of every datagram of one table entry (off, len, seg_len, first)."""
    off, length, seg_len, first = (int(v) for v in buf)
    c = count(length, seg_len)
    if c == 1:
        return [(first, off, length)]
    return [(first + k, off + k * seg_len, min(seg_len, length - k * seg_len)) for k in range(c)]


def skipped(buf, packed_len: int, n: int) -> bool:
    off, length, seg_len, first = (int(v) for v in buf)
    return off + length > packed_len or first + count(length, seg_len) > n


def table_ok(bufs, n: int) -> bool:
    at = 0
    for b in bufs:
        if int(b[3]) != at:
            return False
        at += count(int(b[1]), int(b[2]))
    return at == n


def unpack(packed, packed_len: int, bufs, n: int, arena, stride: int, lens) -> None:
    """In place: `arena` a flat uint8 array of n * stride bytes, `lens` uint32 (n)."""
    for b in bufs:
        if skipped(b, packed_len, n):
            continue
        for slot, src, L in datagrams(b):
            lens[slot] = L
            m = min(L, stride)
            arena[slot * stride:slot * stride + m] = packed[src:src + m]


def fresh(n: int, stride: int):
    """An arena and lengths full of sentinels: whatever an unpack does not name must keep them."""
    return np.full(n * stride, SENTINEL, np.uint8), np.full(n, LEN_SENTINEL, np.uint32)


def layout(specs, seed: int):
    """A packed area for specs of (len, seg_len, off % 16): each buffer at the next offset of that residue,
    random bytes everywhere (the gaps too), packed_len the end of the last buffer, the allocation rounded up
    to 16 B.  -> (packed, packed_len, bufs (n_bufs, 4) uint32, n)."""
    bufs, at, first = [], 0, 0
    for length, seg_len, mod in specs:
        off = at + (mod - at) % 16
        bufs.append((off, length, seg_len, first))
        first += count(length, seg_len)
        at = off + length
    rng = np.random.default_rng(seed)
    packed = rng.integers(0, 256, max(16, (at + 15) & ~15), dtype=np.uint8)
    return packed, at, np.array(bufs, np.uint32).reshape(-1, 4), first


def edge_specs(stride: int):
    """Every datagram length around the 4- and 16-byte pieces and around the stride, as lone buffers (seg_len 0
    and seg_len > len in turn) and as segments of coalesced buffers, at every source residue of 16; odd and even
    segment sizes; a shorter last segment, a one-byte last segment, exactly 64 segments; the last buffer ends
    off a 16-byte boundary."""
    lengths = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 1382, stride - 1, stride, stride + 1)
    specs = []
    for j, L in enumerate(lengths):
        for mod in range(16):
            specs.append((L, 0 if (j + mod) % 2 == 0 else L + 1 + mod, mod))
    for mod in range(16):
        for seg in (1, 3, 4, 15, 16, 17, 63, 64, 65, 77, 1382, stride - 1, stride, stride + 1):
            specs.append((3 * seg + max(1, seg - 10 if seg > 10 else seg), seg, mod))  # a shorter (or full) last one
            if seg > 1:
                specs.append((2 * seg + 1, seg, (mod + 5) % 16))                      # a one-byte last one
    for mod, seg in ((0, 101), (7, 1000), (12, 16), (15, 1)):
        specs.append((64 * seg, seg, mod))                                            # exactly 64 segments
    specs.append((1382, 0, 3))  # ends at 3 + 1382 = 9 mod 16
    return specs


def edge_case(stride: int):
    packed, packed_len, bufs, n = layout(edge_specs(stride), 0x6A0 + stride)
    assert packed_len % 16 != 0 and int(bufs[-1][0]) + int(bufs[-1][1]) == packed_len
    assert {int(b[0]) % 16 for b in bufs} == set(range(16))
    return packed, packed_len, bufs, n


def random_batch(seed: int, n: int, lone_len=None):
    """n datagrams: buffers of 1..64 segments of a seeded random size in 1..1472 with a random shorter tail, or
    (lone_len) n lone buffers of that many bytes."""
    rng = np.random.default_rng(seed)
    specs, total = [], 0
    while total < n:
        if lone_len is not None:
            specs.append((lone_len, 0, int(rng.integers(0, 16))))
            total += 1
            continue
        c = int(min(rng.integers(1, 65), n - total))
        seg = int(rng.integers(1, min(1472, 65535 // c) + 1))  # a buffer holds at most 65535 bytes
        last = int(rng.integers(1, seg + 1))
        length = (c - 1) * seg + last
        specs.append((length, seg if c > 1 or rng.integers(0, 2) else 0, int(rng.integers(0, 16))))
        total += count(length, specs[-1][1])
    packed, packed_len, bufs, total = layout(specs, seed + 1)
    assert total == n
    return packed, packed_len, bufs, n


def host_coalesces() -> bool:
    """Whether this kernel's loopback hands a UDP_SEGMENT train back as one UDP_GRO buffer: plain sockets, the
    option numbers of linux/udp.h, nothing of the library."""
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        rx.bind(("127.0.0.1", 0))
        rx.settimeout(1.0)
        rx.setsockopt(socket.IPPROTO_UDP, UDP_GRO, 1)
        tx.sendmsg([b"a" * 10, b"b" * 10, b"c" * 10], [(socket.IPPROTO_UDP, UDP_SEGMENT, struct.pack("H", 10))], 0,
                   rx.getsockname())
        data, anc, _, _ = rx.recvmsg(65536, socket.CMSG_SPACE(4))
        return len(data) == 30 and any(lvl == socket.IPPROTO_UDP and typ == UDP_GRO and
                                       int.from_bytes(val[:2], "little") == 10 for lvl, typ, val in anc)
    except OSError:
        return False
    finally:
        rx.close()
        tx.close()
