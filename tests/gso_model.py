"""The contract of include/qgcm.h "TUN super-frames segmented on routed batches" restated in numpy, from the
header's text and independently of quantum_amd/csrc/gso_core.h: when an entry is valid, the segments of a TCP4 /
UDP4 super-frame with their patched headers and checksums, the completed checksum of a CSUM packet, the clamp, the
void entries, and -- composed with the outgoing resolve, the peer always from a dict -- what qgcm_gso_resolve
leaves.  Also a builder of super-frames as a TUN queue with IFF_VNET_HDR hands them over.  Shared by
tests/test_gso_model.py (the host segmentation), tests/test_gpu_gso.py (the kernel and the pipeline) and
tools/tun_gso_bench.py.  A frame's segments are made with array operations over all of them at once, so a table
of half a million slots takes seconds.
"""
from __future__ import annotations

import numpy as np

from frames_model import DESC, LEN_SENTINEL, PEER_SENTINEL, SENTINEL, Net, fresh  # noqa: F401  (re-exported)
from route_model import NO_PEER, OVERHEAD

PLAIN, CSUM, TCP4, UDP4 = 0, 1, 2, 3
SEGS = 2048
FRAME = np.dtype([("off", "<u4"), ("len", "<u4"), ("first", "<u4"), ("count", "<u4"), ("gso_size", "<u2"), ("hdr_len", "<u2"),
                  ("l4_off", "<u2"), ("csum_off", "<u2"), ("kind", "<u4"), ("reserved", "<u4")])
assert FRAME.itemsize == 32
FIN, PSH, ACK = 0x01, 0x08, 0x10


def entry(off=0, len=0, first=0, count=1, gso_size=0, hdr_len=0, l4_off=0, csum_off=0, kind=PLAIN):
    e = np.zeros((), FRAME)
    e["off"], e["len"], e["first"], e["count"] = off, len, first, count
    e["gso_size"], e["hdr_len"], e["l4_off"], e["csum_off"], e["kind"] = gso_size, hdr_len, l4_off, csum_off, kind
    return e


def valid(f, packed_len: int, n: int) -> bool:
    off, length, first, count, kind = int(f["off"]), int(f["len"]), int(f["first"]), int(f["count"]), int(f["kind"])
    gso, hdr, l4, co = int(f["gso_size"]), int(f["hdr_len"]), int(f["l4_off"]), int(f["csum_off"])
    if off % 16 or off + length > packed_len or first + count > n or kind > 3:
        return False
    if kind == PLAIN:
        return count == 1
    if kind == CSUM:
        return count == 1 and l4 % 2 == 0 and co % 2 == 0 and l4 + co + 2 <= length
    if not (20 <= l4 <= 60 and l4 % 4 == 0):
        return False
    if kind == UDP4 and hdr != l4 + 8:
        return False
    if kind == TCP4 and not (20 <= hdr - l4 <= 60 and (hdr - l4) % 4 == 0):
        return False
    if hdr >= length or gso < 1:
        return False
    return count == -(-(length - hdr) // gso) and count <= SEGS


def table_ok(frames, n: int, packed_len: int) -> bool:
    """What the host calls ask: every entry valid, `first` the prefix sum of the counts, n slots in all."""
    at = 0
    for f in frames:
        if int(f["first"]) != at or not valid(f, packed_len, n):
            return False
        at += int(f["count"])
    return at == n


def _words(a):
    """Big-endian 16-bit words of the rows of a uint8 array of even width, as uint64."""
    return (a[:, 0::2].astype(np.uint64) << np.uint64(8)) | a[:, 1::2].astype(np.uint64)


def _fold_not(s):
    s = s.astype(np.uint64)
    for _ in range(4):
        s = (s & np.uint64(0xFFFF)) + (s >> np.uint64(16))
    return (~s) & np.uint64(0xFFFF)


def _put16(rows, at, v):
    rows[:, at] = (v >> 8) & 0xFF
    rows[:, at + 1] = v & 0xFF


def segments(packed, f):
    """The packets of a valid entry: (rows, L) -- rows a (count, width) uint8 array, packet k in rows[k, :L[k]],
    zeros behind it."""
    off, length, kind = int(f["off"]), int(f["len"]), int(f["kind"])
    frame = np.asarray(packed[off:off + length], np.uint8)
    if kind in (PLAIN, CSUM):
        rows = np.zeros((1, length + (length & 1)), np.uint8)
        rows[0, :length] = frame
        if kind == CSUM:
            l4, at = int(f["l4_off"]), int(f["l4_off"]) + int(f["csum_off"])
            c = int(_fold_not(_words(rows[:, l4:]).sum(axis=1))[0]) or 0xFFFF
            rows[0, at], rows[0, at + 1] = c >> 8, c & 0xFF
        return rows, np.array([length], np.int64)
    gso, hdr, l4, count = int(f["gso_size"]), int(f["hdr_len"]), int(f["l4_off"]), int(f["count"])
    width = hdr + gso + ((hdr + gso) & 1)
    body = np.zeros(count * gso, np.uint8)
    body[:length - hdr] = frame[hdr:]
    rows = np.zeros((count, width), np.uint8)
    rows[:, :hdr] = frame[:hdr]
    rows[:, hdr:hdr + gso] = body.reshape(count, gso)
    k = np.arange(count, dtype=np.int64)
    P = np.minimum(gso, length - hdr - k * gso)
    L = hdr + P
    _put16(rows, 2, L & 0xFFFF)
    id0 = int(frame[4]) << 8 | int(frame[5])
    _put16(rows, 4, (id0 + k) & 0xFFFF)
    _put16(rows, 10, np.zeros(count, np.int64))
    _put16(rows, 10, _fold_not(_words(rows[:, :l4]).sum(axis=1)).astype(np.int64))
    l4_len = (L - l4) & 0xFFFF
    if kind == TCP4:
        seq = (int.from_bytes(frame[l4 + 4:l4 + 8].tobytes(), "big") + k * gso) & 0xFFFFFFFF
        _put16(rows, l4 + 4, seq >> 16)
        _put16(rows, l4 + 6, seq & 0xFFFF)
        rows[:-1, l4 + 13] &= 0xFF ^ (FIN | PSH)
        at, proto = l4 + 16, 6
    else:
        _put16(rows, l4 + 4, l4_len)
        at, proto = l4 + 6, 17
    _put16(rows, at, np.zeros(count, np.int64))
    s = _words(rows[:, 12:20]).sum(axis=1) + np.uint64(proto) + l4_len.astype(np.uint64) + _words(rows[:, l4:]).sum(axis=1)
    c = _fold_not(s).astype(np.int64)
    if kind == UDP4:
        c[c == 0] = 0xFFFF
    _put16(rows, at, c)
    return rows, L


def gso_resolve(net, packed, packed_len: int, frames, n: int, arena, stride: int, lens, peer, descs, resolve=True) -> None:
    """qgcm_gso_resolve over the entries in table order (a table whose `first` ascends): the slots of every valid
    entry, the void-frame result for slot `first` of a void one with count >= 1 and first < n, nothing for any
    other slot.  resolve=False: the segmentation alone (lens and the arena, as qgcm_gso_unpack_cpu)."""
    a2 = arena[:n * stride].reshape(n, stride)
    own = np.frombuffer(net.own_ip.to_bytes(4, "little"), np.uint8) if resolve else None
    for f in frames:
        first, count = int(f["first"]), int(f["count"])
        if not valid(f, packed_len, n):
            if count >= 1 and first < n and resolve:
                lens[first], peer[first] = 0, NO_PEER
                descs[first] = (first * stride, 0, NO_PEER)
            continue
        rows, L = segments(packed, f)
        sl = slice(first, first + count)
        lens[sl] = L
        room = stride - 4
        full = int(min(int(L[0]), room))  # every segment but the last has L[0] bytes
        a2[first:first + count - 1, 4:4 + full] = rows[:-1, :full]
        last = int(min(int(L[-1]), room))
        a2[first + count - 1, 4:4 + last] = rows[-1, :last]
        if not resolve:
            continue
        p = NO_PEER
        if int(f["len"]) >= 20:
            dst = int.from_bytes(np.asarray(packed[int(f["off"]) + 16:int(f["off"]) + 20], np.uint8).tobytes(), "little")
            key = dst if (dst & net.mask) == (net.net & net.mask) else net.gateway
            p = net.table.get(key, NO_PEER)
        ok = (L >= 20) & (4 + L + OVERHEAD <= stride) & (p != NO_PEER)
        peer[sl] = np.where(ok, p, NO_PEER)
        a2[first:first + count][ok, 0:4] = own
        d = descs[sl]
        d["off"] = np.arange(first, first + count, dtype=np.uint64) * np.uint64(stride)
        d["len"] = L
        d["key"] = peer[sl]


def packets(packed, packed_len: int, frames, n: int):
    """The whole packets of a well-formed table, in slot order."""
    assert table_ok(frames, n, packed_len)
    out = []
    for f in frames:
        rows, L = segments(packed, f)
        out += [rows[k, :int(L[k])].copy() for k in range(len(L))]
    return out


# ---- the builder: super-frames as the kernel hands them over ----

def _csum_partial(b: bytes) -> int:
    """The ones'-complement sum, folded but not complemented: what the stack leaves for the device to finish."""
    if len(b) % 2:
        b += b"\0"
    s = sum(int.from_bytes(b[i:i + 2], "big") for i in range(0, len(b), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def ip_header(ihl: int, total: int, ident: int, proto: int, src: bytes, dst: bytes, rng) -> bytearray:
    h = bytearray(ihl)
    h[0], h[1] = 0x40 | ihl // 4, 0
    h[2:4] = (total & 0xFFFF).to_bytes(2, "big")
    h[4:6] = (ident & 0xFFFF).to_bytes(2, "big")
    h[6:8] = b"\x40\x00"
    h[8], h[9] = 64, proto
    h[12:16], h[16:20] = src, dst
    h[20:] = bytes(rng.integers(0, 256, ihl - 20, dtype=np.uint8))  # options: any bytes
    h[10:12] = (0xFFFF ^ _csum_partial(bytes(h))).to_bytes(2, "big")
    return h


def le_ip(v: int) -> bytes:
    return int(v).to_bytes(4, "little")  # common.IPtoInt is little-endian over the address bytes


def tcp_frame(rng, payload_len: int, gso: int, dst: int, ihl=20, tcp_hl=20, ident=0x1234, seq=0x01020304,
              flags=ACK | PSH | FIN, payload=None, src=0x0100630A):
    """(frame bytes, fields of its entry): a TCP super-frame with the pseudo-header's partial sum in the checksum
    field, as a TUN queue with TUN_F_CSUM hands it over."""
    pay = bytes(rng.integers(0, 256, payload_len, dtype=np.uint8)) if payload is None else bytes(payload)
    hdr_len = ihl + tcp_hl
    ip = ip_header(ihl, hdr_len + len(pay), ident, 6, le_ip(src), le_ip(dst), rng)
    t = bytearray(tcp_hl)
    t[0:4] = bytes(rng.integers(0, 256, 4, dtype=np.uint8))
    t[4:8] = (seq & 0xFFFFFFFF).to_bytes(4, "big")
    t[8:12] = bytes(rng.integers(0, 256, 4, dtype=np.uint8))
    t[12], t[13] = (tcp_hl // 4) << 4, flags
    t[14:16] = b"\xff\xff"
    t[20:] = bytes(rng.integers(0, 256, tcp_hl - 20, dtype=np.uint8))
    pseudo = bytes(ip[12:20]) + bytes([0, 6]) + ((tcp_hl + len(pay)) & 0xFFFF).to_bytes(2, "big")
    t[16:18] = _csum_partial(pseudo).to_bytes(2, "big")
    frame = np.frombuffer(bytes(ip) + bytes(t) + pay, np.uint8)
    return frame, dict(kind=TCP4, gso_size=gso, hdr_len=hdr_len, l4_off=ihl, count=-(-len(pay) // gso))


def udp_frame(rng, payload_len: int, gso: int, dst: int, ihl=20, ident=0xFFFE, payload=None, src=0x0100630A):
    pay = bytes(rng.integers(0, 256, payload_len, dtype=np.uint8)) if payload is None else bytes(payload)
    ip = ip_header(ihl, ihl + 8 + len(pay), ident, 17, le_ip(src), le_ip(dst), rng)
    u = bytearray(8)
    u[0:4] = bytes(rng.integers(0, 256, 4, dtype=np.uint8))
    u[4:6] = ((8 + len(pay)) & 0xFFFF).to_bytes(2, "big")
    pseudo = bytes(ip[12:20]) + bytes([0, 17]) + bytes(u[4:6])
    u[6:8] = _csum_partial(pseudo).to_bytes(2, "big")
    frame = np.frombuffer(bytes(ip) + bytes(u) + pay, np.uint8)
    return frame, dict(kind=UDP4, gso_size=gso, hdr_len=ihl + 8, l4_off=ihl, count=-(-len(pay) // gso))


def csum_packet(rng, payload_len: int, dst: int, tcp: bool, ihl=20):
    """A single packet whose L4 checksum the stack left partial (virtio's NEEDS_CSUM): csum_start = ihl, csum_offset
    16 (TCP) or 6 (UDP)."""
    if tcp:
        frame, f = tcp_frame(rng, payload_len, max(1, payload_len), dst, ihl=ihl)
        return frame, dict(kind=CSUM, l4_off=ihl, csum_off=16, count=1)
    frame, f = udp_frame(rng, payload_len, max(1, payload_len), dst, ihl=ihl)
    return frame, dict(kind=CSUM, l4_off=ihl, csum_off=6, count=1)


def plain_packet(rng, length: int, dst):
    p = rng.integers(0, 256, length, dtype=np.uint8)
    if dst is not None and length >= 20:
        p[16:20] = np.frombuffer(le_ip(dst), np.uint8)
    return p, dict(kind=PLAIN, count=1)


def vnet_header(fields, frame_len: int, whole_hdr_len=False) -> bytes:
    """The 10-byte virtio_net_hdr the kernel would put in front: hdr_len is the linear part of its buffer --
    `whole_hdr_len`: the whole frame, as it is at times."""
    import struct

    kind = fields["kind"]
    gso_type = {PLAIN: 0, CSUM: 0, TCP4: 1, UDP4: 5}[kind]
    flags = 0 if kind == PLAIN else 1
    off = {PLAIN: 0, CSUM: fields.get("csum_off", 0), TCP4: 16, UDP4: 6}[kind]
    hdr_len = frame_len if whole_hdr_len else fields.get("hdr_len", 0)
    return struct.pack("<BBHHHH", flags, gso_type, hdr_len & 0xFFFF, fields.get("gso_size", 0), fields.get("l4_off", 0), off)


def layout(items, seed: int = 0, slot_gaps=False):
    """(packed, packed_len, frames, n): the frames of `items` ((bytes, fields) pairs) each on a 16-byte boundary
    with ten bytes free before it, as qgcm_tun_read_gso lays them (the first at 16), seeded junk in between, the
    area rounded up to 16 B; `first` the prefix sum of the counts (`slot_gaps`: now and then a slot left out, which
    no entry names); packed_len = the end of the last frame."""
    rng = np.random.default_rng(0x650A + seed)
    frames = np.zeros(len(items), FRAME)
    at, end, slot = 16, 0, 0
    for i, (b, f) in enumerate(items):
        if slot_gaps and i % 4 == 2:
            slot += 1 + i % 3
        frames[i] = entry(off=at, len=len(b), first=slot, **f)
        slot += int(frames[i]["count"])
        end = at + len(b)
        at = (end + 10 + 15) & ~15
    packed = rng.integers(0, 256, max(16, (end + 15) & ~15), dtype=np.uint8)
    for fr, (b, _) in zip(frames, items):
        packed[int(fr["off"]):int(fr["off"]) + len(b)] = b
    return packed, end, frames, slot


def rfc1071(b: bytes) -> int:
    """The Internet checksum of RFC 1071 over b, plainly: 0 for a packet whose checksum field is right."""
    if len(b) % 2:
        b += b"\0"
    s = 0
    for i in range(0, len(b), 2):
        s += b[i] << 8 | b[i + 1]
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def verify(pkt: bytes):
    """(IPv4 header checksum right, L4 checksum right) of a whole TCP or UDP packet over IPv4."""
    ihl = (pkt[0] & 15) * 4
    total = int.from_bytes(pkt[2:4], "big")
    l4 = pkt[ihl:]
    pseudo = pkt[12:20] + bytes([0, pkt[9]]) + len(l4).to_bytes(2, "big")
    return rfc1071(pkt[:ihl]) == 0 and total == len(pkt), rfc1071(pseudo + l4) == 0
