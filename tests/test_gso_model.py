"""CPU: qgcm_gso_unpack_cpu (quantum_amd/csrc/gso_core.h) equals tests/gso_model.py byte for byte -- arenas, lengths
and sentinels -- and, independently of both, what it makes are packets: every segment's IPv4 and L4 checksum
verifies with a plain RFC 1071 routine, the payloads in sequence order give the frame's payload back, sequence
numbers and ids are consecutive, FIN and PSH appear on the last segment only.  Every table the header calls not
well-formed is refused with nothing written."""
import numpy as np
import pytest

import gso_model as M
from quantum_amd import _lib, route

DST = int.from_bytes(bytes([10, 99, 0, 3]), "little")


def unpack_cpu(packed, packed_len, frames, n, stride):
    arena, lens = np.full(max(1, n) * stride, M.SENTINEL, np.uint8), np.full(max(1, n), M.LEN_SENTINEL, np.uint32)
    route.gso_unpack_cpu(packed, packed_len, frames, n, arena, stride, lens)
    return arena, lens


def model(packed, packed_len, frames, n, stride):
    arena, lens, peer, descs = M.fresh(n, stride)
    M.gso_resolve(None, packed, packed_len, frames, n, arena, stride, lens, peer, descs, resolve=False)
    return arena, lens


def mixed_items(seed):
    rng = np.random.default_rng(seed)
    items = []
    for gso in (1, 3, 4, 15, 16, 17, 1347, 1348, 1448):
        for tail in (1, 2, 3, gso - 1, gso):
            if tail < 1:
                continue
            items.append(M.tcp_frame(rng, 2 * gso + tail, gso, DST, ident=0xFFFE, seq=0xFFFFFFFF - gso))
    for ihl, tcp_hl in ((20, 20), (24, 20), (20, 32), (40, 60), (60, 60)):
        items.append(M.tcp_frame(rng, 5000, 1348, DST, ihl=ihl, tcp_hl=tcp_hl))
    for count in (1, 2, 63, 64, 65):
        items.append(M.tcp_frame(rng, 24 * count - 5, 24, DST))
        items.append(M.udp_frame(rng, 31 * count - 30, 31, DST, ihl=24))
    items.append(M.udp_frame(rng, 3 * 1472, 1472, DST))
    items.append(M.tcp_frame(rng, M.SEGS * 7, 7, DST))
    for tcp in (True, False):
        for L in (0, 1, 2, 3, 100, 1349):
            items.append(M.csum_packet(rng, L, DST, tcp))
    for L in (0, 1, 19, 20, 64, 1350, 3000):
        items.append(M.plain_packet(rng, L, DST))
    return items


@pytest.fixture(scope="module")
def mixed():
    return M.layout(mixed_items(0x6501), 1)


@pytest.mark.parametrize("stride", (1536, 1388, 64, 8))
def test_unpack_cpu_equals_the_model(mixed, stride):
    packed, packed_len, frames, n = mixed
    assert M.table_ok(frames, n, packed_len)
    got, want = unpack_cpu(packed, packed_len, frames, n, stride), model(packed, packed_len, frames, n, stride)
    assert np.array_equal(got[1], want[1])
    if not np.array_equal(got[0], want[0]):
        at = np.flatnonzero(got[0] != want[0])
        raise AssertionError(f"{at.size} bytes differ, the first in slot {int(at[0]) // stride} at byte {int(at[0]) % stride}")
    assert (got[0] == M.SENTINEL).sum() > n  # the tails kept their bytes


def test_segments_are_packets(mixed):
    """From the library's arena alone, with a plain RFC 1071 routine."""
    packed, packed_len, frames, n = mixed
    stride = 3104
    arena, lens = unpack_cpu(packed, packed_len, frames, n, stride)
    a2 = arena.reshape(n, stride)
    for f in frames:
        first, count, kind = int(f["first"]), int(f["count"]), int(f["kind"])
        if kind == M.PLAIN:
            assert a2[first, 4:4 + int(f["len"])].tobytes() == packed[int(f["off"]):int(f["off"]) + int(f["len"])].tobytes()
            continue
        pkts = [a2[first + k, 4:4 + int(lens[first + k])].tobytes() for k in range(count)]
        for p in pkts:
            assert M.verify(p) == (True, True)
        if kind == M.CSUM:
            continue
        hdr, l4, gso = int(f["hdr_len"]), int(f["l4_off"]), int(f["gso_size"])
        frame = packed[int(f["off"]):int(f["off"]) + int(f["len"])].tobytes()
        assert b"".join(p[hdr:] for p in pkts) == frame[hdr:]
        assert all(len(p) == hdr + gso for p in pkts[:-1]) and 1 <= len(pkts[-1]) - hdr <= gso
        id0 = int.from_bytes(frame[4:6], "big")
        assert [int.from_bytes(p[4:6], "big") for p in pkts] == [(id0 + k) & 0xFFFF for k in range(count)]
        if kind == M.TCP4:
            seq0 = int.from_bytes(frame[l4 + 4:l4 + 8], "big")
            assert [int.from_bytes(p[l4 + 4:l4 + 8], "big") for p in pkts] == [(seq0 + k * gso) & 0xFFFFFFFF for k in range(count)]
            assert all(p[l4 + 13] & (M.FIN | M.PSH) == 0 and p[l4 + 13] & M.ACK for p in pkts[:-1])
            assert pkts[-1][l4 + 13] == frame[l4 + 13] and frame[l4 + 13] & (M.FIN | M.PSH) == M.FIN | M.PSH
        else:
            assert all(int.from_bytes(p[l4 + 4:l4 + 6], "big") == len(p) - l4 for p in pkts)
        for p in pkts:  # nothing else of the header moved
            keep = bytearray(p[:hdr])
            ref = bytearray(frame[:hdr])
            for at, w in ((2, 4), (10, 2)) + (((l4 + 4, 4), (l4 + 13, 1), (l4 + 16, 2)) if kind == M.TCP4 else ((l4 + 4, 4),)):
                keep[at:at + w] = ref[at:at + w] = bytes(w)
            assert keep == ref


def udp_zero_checksum_item(seed=0x0C5):
    """A UDP super-frame whose first segment's checksum comes to 0, which goes out as 0xffff."""
    rng = np.random.default_rng(seed)
    pay = bytearray(rng.integers(0, 256, 200, dtype=np.uint8))
    pay[0:2] = b"\0\0"
    frame, f = M.udp_frame(np.random.default_rng(seed + 1), 200, 100, DST, payload=pay)  # (the ports are drawn)
    rows, L = M.segments(frame, M.entry(off=0, len=len(frame), **f))
    seg = bytearray(rows[0, :int(L[0])].tobytes())
    seg[26:28] = b"\0\0"
    c = M.rfc1071(bytes(seg[12:20]) + bytes([0, 17]) + (len(seg) - 20).to_bytes(2, "big") + bytes(seg[20:]))
    pay[0:2] = c.to_bytes(2, "big")  # the word that brings the sum to 0xffff
    return M.udp_frame(np.random.default_rng(seed + 1), 200, 100, DST, payload=pay)


def test_udp_checksum_of_zero_goes_out_as_ffff():
    item = udp_zero_checksum_item()
    packed, packed_len, frames, n = M.layout([item])
    arena, lens = unpack_cpu(packed, packed_len, frames, n, 1536)
    seg = arena[4:4 + int(lens[0])].tobytes()
    assert seg[26:28] == b"\xff\xff" and M.verify(seg) == (True, True)
    arena2, _ = model(packed, packed_len, frames, n, 1536)
    assert np.array_equal(arena, arena2)


def bad_tables(packed_len, frames, n):
    """(name, table, n_frames-or-None, n) for every rule of the header."""
    def changed(i, **kw):
        t = frames.copy()
        for k, v in kw.items():
            t[i][k] = v
        return t

    kinds = frames["kind"].tolist()
    tcp, udp, cs, pl = kinds.index(M.TCP4), kinds.index(M.UDP4), kinds.index(M.CSUM), kinds.index(M.PLAIN)
    T, U, C = frames[tcp], frames[udp], frames[cs]
    yield "off not on a 16-byte boundary", changed(tcp, off=int(T["off"]) + 4), n
    yield "past the packed area", changed(len(frames) - 1, len=packed_len - int(frames[-1]["off"]) + 1), n
    yield "off + len wraps 32 bits", changed(pl, off=0xFFFFFFF0, len=0x20), n
    yield "kind 4", changed(pl, kind=4), n
    yield "a plain entry of two slots", changed(pl, count=2), n
    yield "a csum entry of no slot", changed(cs, count=0), n
    yield "csum: l4_off odd", changed(cs, l4_off=int(C["l4_off"]) + 1), n
    yield "csum: csum_off odd", changed(cs, csum_off=int(C["csum_off"]) + 1), n
    yield "csum: the field past the packet", changed(cs, csum_off=(int(C["len"]) - int(C["l4_off"]) + 1) & ~1), n
    yield "l4_off 16", changed(tcp, l4_off=16), n
    yield "l4_off 64", changed(tcp, l4_off=64), n
    yield "l4_off 22", changed(tcp, l4_off=22), n
    yield "udp: hdr_len not l4_off + 8", changed(udp, hdr_len=int(U["hdr_len"]) + 4), n
    yield "tcp: header of 16", changed(tcp, hdr_len=int(T["l4_off"]) + 16), n
    yield "tcp: header of 64", changed(tcp, hdr_len=int(T["l4_off"]) + 64), n
    yield "tcp: header of 22", changed(tcp, hdr_len=int(T["l4_off"]) + 22), n
    yield "hdr_len == len", changed(tcp, len=int(T["hdr_len"])), n
    yield "gso_size 0", changed(tcp, gso_size=0), n
    yield "count one short", changed(tcp, count=int(T["count"]) - 1), n
    yield "count one over", changed(udp, count=int(U["count"]) + 1), n
    yield "first + count past n", frames, n - 1
    yield "the counts do not total n", frames, n + 1
    swapped = frames.copy()
    swapped[[tcp, tcp + 1]] = swapped[[tcp + 1, tcp]]
    yield "first does not ascend", swapped, n
    gap = frames.copy()
    gap["first"][tcp + 1:] += 1
    yield "a gap in first", gap, n + 1


def test_tables_that_are_not_well_formed_are_refused(mixed):
    packed, packed_len, frames, n = mixed
    L = _lib.lib()
    seen = 0
    for name, table, m in bad_tables(packed_len, frames, n):
        assert not M.table_ok(table, m, packed_len), name
        arena, lens = np.full(max(n, m) * 256, M.SENTINEL, np.uint8), np.full(max(n, m), M.LEN_SENTINEL, np.uint32)
        rc = L.qgcm_gso_unpack_cpu(packed.ctypes.data, packed_len, table.ctypes.data, len(table), m, arena.ctypes.data, 256,
                                   lens.ctypes.data)
        assert rc == _lib.QGCM_E_ARG, name
        assert np.all(arena == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL), name
        seen += 1
    assert seen == 24
    # more than 2048 segments: a frame of 2049 payload bytes cut every byte
    rng = np.random.default_rng(5)
    frame, f = M.tcp_frame(rng, M.SEGS + 1, 1, DST)
    p2, l2, t2, n2 = M.layout([(frame, f)])
    assert n2 == M.SEGS + 1 and not M.table_ok(t2, n2, l2)
    arena, lens = np.full(n2 * 64, M.SENTINEL, np.uint8), np.full(n2, M.LEN_SENTINEL, np.uint32)
    assert L.qgcm_gso_unpack_cpu(p2.ctypes.data, l2, t2.ctypes.data, 1, n2, arena.ctypes.data, 64, lens.ctypes.data) == _lib.QGCM_E_ARG
    assert np.all(arena == M.SENTINEL)


def test_argument_errors(mixed):
    packed, packed_len, frames, n = mixed
    L = _lib.lib()
    arena, lens = np.full(n * 64, M.SENTINEL, np.uint8), np.full(n, M.LEN_SENTINEL, np.uint32)
    good = [packed.ctypes.data, packed_len, frames.ctypes.data, len(frames), n, arena.ctypes.data, 64, lens.ctypes.data]
    for k, v in ((0, None), (2, None), (5, None), (7, None), (6, 0), (6, 4), (6, 66), (4, (1 << 31) + 1), (3, n + 1)):
        a = list(good)
        a[k] = v
        assert L.qgcm_gso_unpack_cpu(*a) == _lib.QGCM_E_ARG, (k, v)
    assert np.all(arena == M.SENTINEL) and np.all(lens == M.LEN_SENTINEL)
    assert L.qgcm_gso_unpack_cpu(None, 0, None, 0, 0, None, 64, None) == 0
    assert L.qgcm_gso_unpack_cpu(*good) == 0 and not np.all(arena == M.SENTINEL)


def test_the_builder_makes_frames_the_kernel_would():
    """The checksum field holds the pseudo-header's partial sum, so completing it as NEEDS_CSUM says gives a packet
    that verifies; the vnet header's hdr_len may be the whole frame."""
    rng = np.random.default_rng(9)
    for tcp in (True, False):
        frame, f = M.csum_packet(rng, 333, DST, tcp)
        rows, L = M.segments(frame, M.entry(off=0, len=len(frame), **f))
        assert M.verify(rows[0, :int(L[0])].tobytes()) == (True, True)
        assert M.verify(frame.tobytes()) == (True, False)
    frame, f = M.tcp_frame(rng, 4000, 1348, DST)
    import struct
    assert struct.unpack("<BBHHHH", M.vnet_header(f, len(frame), True)) == (1, 1, len(frame), 1348, 20, 16)
    assert struct.unpack("<BBHHHH", M.vnet_header(f, len(frame)))[2] == 40
