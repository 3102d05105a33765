"""CPU: qgcm_deliver_coalesce_cpu (quantum_amd/csrc/coalesce_core.h) equals tests/coalesce_model.py in packed bytes,
table and counts, with sentinels behind every array -- and, resting on parent code instead of the model: the
produced table and area go through qgcm_gso_unpack_cpu and give the delivered packets back byte for byte; packets
qgcm_gso_unpack_cpu cuts from a super-frame coalesce back to that frame; a plain RFC 1071 loop finds every coalesced
frame's IPv4 checksum right and its TCP field completing to a valid checksum.  Every link rule broken, one at a
time, splits a run there and only there."""
import numpy as np
import pytest

import coalesce_cases as K
import coalesce_model as M
from quantum_amd import _lib, route

S = K.SENTINEL


def run_cpu(arena, stride, n, lens, peer, status, cap=None):
    """-> (packed with `cap` bytes in front of a sentinel margin, frames[:entries], counts, the whole table)"""
    cap = n * (((stride + 15) & ~15) + 16) if cap is None else cap
    packed = np.full(cap + 64, S, np.uint8)
    frames = np.zeros(n + 2, M.GSO_FRAME)
    frames.view(np.uint8)[:] = S
    a, l, p = arena.copy(), lens.copy(), peer.copy()
    got, counts = route.deliver_coalesce_cpu(a, stride, n, l, p, status, packed[:cap], frames[:max(n, 1)])
    assert np.array_equal(a, arena) and np.array_equal(l, lens) and np.array_equal(p, peer)
    assert (packed[cap:] == S).all() and (frames[n:].view(np.uint8) == S).all()
    return packed[:cap], got.copy(), counts, frames


def check_equal(arena, stride, n, lens, peer, status, cap=None):
    packed, frames, counts, _ = run_cpu(arena, stride, n, lens, peer, status, cap)
    want, wframes, wcounts = M.coalesce(arena, stride, n, lens, peer, status, np.full(len(packed), S, np.uint8))
    assert np.array_equal(counts, wcounts)
    assert np.array_equal(frames, wframes)
    assert np.array_equal(packed, want)
    return packed, frames, counts


def rfc1071(data):
    s = 0
    for k in range(0, len(data) - 1, 2):
        s += data[k] << 8 | data[k + 1]
    if len(data) & 1:
        s += data[-1] << 8
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def check_anchors(arena, stride, n, lens, status, packed, frames, counts):
    """the round trip through qgcm_gso_unpack_cpu and the checksums of the coalesced frames"""
    delivered = np.flatnonzero((np.ones(n, bool) if status is None else status == 1) & (4 + lens.astype(np.int64) <= stride))
    assert int(counts[3]) == len(delivered) == int(frames["count"].sum())
    t = frames.copy()
    assert np.array_equal(np.concatenate([np.arange(f, f + c) for f, c in zip(t["first"], t["count"])]), delivered)
    t["first"] = np.cumsum(t["count"]) - t["count"]
    t["reserved"] = 0
    m = len(delivered)
    back, blens = np.zeros(max(1, m) * stride, np.uint8), np.zeros(max(1, m), np.uint32)
    route.gso_unpack_cpu(packed, int(counts[1]), t, m, back, stride, blens)
    assert np.array_equal(blens[:m], lens[delivered])
    rows, brows = arena.reshape(-1, stride), back.reshape(-1, stride)
    col = np.arange(stride - 4)[None, :]
    live = col < lens[delivered][:, None]
    assert np.array_equal(np.where(live, brows[:m, 4:], 0), np.where(live, rows[delivered, 4:], 0))
    for f in frames[frames["kind"] == M.TCP4]:
        pkt = packed[f["off"]:f["off"] + f["len"]].tolist()
        assert rfc1071(pkt[:f["l4_off"]]) == 0xFFFF
        # NEEDS_CSUM: the sum over [l4_off, len), the field's partial value included, complemented into the field
        # must give a segment that verifies against its real pseudo-header
        l4, c = pkt[f["l4_off"]:], 0xFFFF ^ rfc1071(pkt[f["l4_off"]:])
        l4[16], l4[17] = c >> 8, c & 255
        assert rfc1071(pkt[12:20] + [0, 6, len(l4) >> 8, len(l4) & 255] + l4) == 0xFFFF
        lead = packed[f["off"] - 16:f["off"]]
        assert not lead[:6].any() and lead[6] == 1 and lead[7] == 1
        assert lead[8:].view("<u2").tolist() == [f["hdr_len"], f["gso_size"], f["l4_off"], 16]
    for f in frames[frames["kind"] == M.PLAIN]:
        assert not packed[f["off"] - 16:f["off"]].any()


@pytest.fixture(scope="module", params=(1536, 1388, 128))
def mixed(request):
    return (request.param,) + K.mixed(request.param)


def test_cpu_equals_the_model_on_the_mixed_batch(mixed):
    stride, arena, lens, peer, status = mixed
    n = len(lens)
    packed, frames, counts = check_equal(arena, stride, n, lens, peer, status)
    assert counts[2] > 50 and (frames["count"] == 64).any()
    check_anchors(arena, stride, n, lens, status, packed, frames, counts)
    if stride >= 1388:
        assert (frames["count"] == 59).sum() == 2  # the cut at 65535 bytes: 130 segments of 1100
    # NULL status: every packet counts as status 1
    packed, frames, counts = check_equal(arena, stride, n, lens, peer, None)
    check_anchors(arena, stride, n, lens, None, packed, frames, counts)


@pytest.mark.parametrize("case", K.split_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_one_broken_rule_splits_there_and_only_there(case):
    stride = 128
    b = K.Batch(stride)
    lo = K.add_split(b, case)
    assert lo == 0
    arena, lens, peer, status = b.done()
    packed, frames, counts = check_equal(arena, stride, 6, lens, peer, status)
    assert tuple(frames["first"]) == case[2]
    check_anchors(arena, stride, 6, lens, status, packed, frames, counts)
    # ... and without the edit the six are one entry
    b = K.Batch(stride)
    K.add_split(b, ("none", lambda b, lo: None, (0,)))
    arena, lens, peer, status = b.done()
    _, frames, counts = check_equal(arena, stride, 6, lens, peer, status)
    assert tuple(frames["first"]) == (0,) and frames["count"][0] == 6 and tuple(counts) == (1, 16 + 208, 1, 6)


def sizes(stride, P, **kw):
    b = K.Batch(stride)
    b.run(len(P), P, **kw)
    arena, lens, peer, status = b.done()
    packed, frames, counts = check_equal(arena, stride, len(P), lens, peer, status)
    check_anchors(arena, stride, len(P), lens, status, packed, frames, counts)
    return frames


def test_cut_at_64_members_and_at_65535_bytes():
    assert sizes(128, [20] * 130)["count"].tolist() == [64, 64, 2]
    f = sizes(1536, [1100] * 130)  # (65535 - 40) / 1100 = 59
    assert f["count"].tolist() == [59, 59, 12] and f["len"][0] == 40 + 59 * 1100 <= 65535
    assert sizes(1536, [1023] * 65)["count"].tolist() == [64, 1]  # 40 + 64 * 1023 = 65512 still fits


def test_tail_rules():
    assert sizes(128, [40, 40, 40, 9])["count"].tolist() == [4]
    assert sizes(128, [40, 9])["count"].tolist() == [2]
    assert sizes(128, [20] * 64 + [7])["count"].tolist() == [64, 1]         # a full frame takes no tail
    assert sizes(128, [20] * 65 + [7])["count"].tolist() == [64, 2]
    assert sizes(128, [40, 39, 38])["count"].tolist() == [2, 1]             # three falling sizes
    assert sizes(128, [40, 39, 38, 37])["count"].tolist() == [2, 1, 1]
    assert sizes(128, [40, 35, 35, 35])["count"].tolist() == [1, 3]         # a tail followed by an eq pair is none
    assert sizes(128, [40, 40, 35, 35])["count"].tolist() == [2, 2]
    assert sizes(128, [40, 40, 41])["count"].tolist() == [2, 1]             # a longer one never joins
    assert sizes(128, [40, 40, 9, 40, 40])["count"].tolist() == [3, 2]
    f = sizes(128, [40, 40, 9])
    assert f["gso_size"][0] == 40 and f["len"][0] == 40 + 89


def test_seq_and_id_wrap():
    assert sizes(128, [30] * 8, seq0=0xFFFFFFFF - 100, id0=0xFFFC)["count"].tolist() == [8]


def test_psh_comes_from_the_last_member():
    b = K.Batch(128)
    b.run(4, 30)
    b.parts[-1]["flags"][3] = M.ACK | M.PSH
    arena, lens, peer, status = b.done()
    packed, frames, counts = check_equal(arena, 128, 4, lens, peer, status)
    assert frames["count"].tolist() == [4] and packed[16 + 20 + 13] == M.ACK | M.PSH


def test_recomputed_zero_against_a_field_of_ffff_is_no_candidate():
    # a payload chosen so that the TCP checksum comes out 0x0000; 0xffff sums right too but is not what is recomputed
    b = K.Batch(128)
    b.run(3, 30)
    arena, lens, peer, status = b.done()
    at = 1 * 128 + 4
    field = int(arena[at + 36]) << 8 | int(arena[at + 37])
    word = int(arena[at + 40]) << 8 | int(arena[at + 41])
    # adding `field` to a payload word (ones' complement) makes the recomputed checksum zero
    s = word + field
    s = (s & 0xFFFF) + (s >> 16)
    arena[at + 40], arena[at + 41], arena[at + 36], arena[at + 37] = s >> 8, s & 255, 0, 0
    assert rfc1071(arena[at + 20:at + 70].tolist() + arena[at + 12:at + 20].tolist() + [0, 6, 0, 50]) == 0xFFFF
    _, frames, _ = check_equal(arena, 128, 3, lens, peer, status)
    assert frames["count"].tolist() == [3]  # the field 0x0000 is what is recomputed: a candidate
    arena[at + 36] = arena[at + 37] = 0xFF
    assert rfc1071(arena[at + 20:at + 70].tolist() + arena[at + 12:at + 20].tolist() + [0, 6, 0, 50]) == 0xFFFF
    _, frames, _ = check_equal(arena, 128, 3, lens, peer, status)
    assert frames["count"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("short", (1, 16, 17, 200, 208, 224, 225, 400))
def test_packed_cap_too_small(short):
    b = K.Batch(128)
    b.run(6, 28, flow=1)   # one entry of 40 + 168 = 208 bytes: region [0, 224)
    b.run(1, 11, flow=2)   # region [224, 224 + 16 + 64)
    b.run(2, 60, flow=3)
    arena, lens, peer, status = b.done()
    full = check_equal(arena, 128, 9, lens, peer, status)
    packed, frames, counts = check_equal(arena, 128, 9, lens, peer, status, cap=short)
    assert counts[1] == full[2][1] and np.array_equal(frames["len"], full[1]["len"])
    lost = frames["off"] == M.NO_ROOM
    assert lost.any() and (np.diff(lost.astype(int)) >= 0).all() and lost[0] == (short < 224)


def test_refusals_and_the_empty_batch():
    L = _lib.lib()
    z = np.zeros(64, np.uint8)
    u = np.zeros(4, np.uint32)
    fr = np.zeros(4, M.GSO_FRAME)
    c = np.full(4, 9, np.uint64)
    args = lambda **k: [k.get("arena", z.ctypes.data), k.get("stride", 16), k.get("n", 1), k.get("lens", u.ctypes.data),
                        k.get("peer", u.ctypes.data), None, k.get("packed", z.ctypes.data), k.get("cap", 64),
                        k.get("frames", fr.ctypes.data), k.get("counts", c.ctypes.data)]
    assert L.qgcm_deliver_coalesce_cpu(*args(n=0, arena=None, lens=None, peer=None, packed=None, frames=None)) == 0
    assert c.tolist() == [0, 0, 0, 0]
    for bad in (dict(stride=18), dict(stride=0), dict(n=(1 << 31) + 1), dict(cap=(1 << 32) - 15), dict(counts=None),
                dict(arena=None), dict(lens=None), dict(peer=None), dict(packed=None), dict(frames=None)):
        assert L.qgcm_deliver_coalesce_cpu(*args(**bad)) == _lib.QGCM_E_ARG, bad


def test_segments_cut_by_gso_unpack_coalesce_back_to_their_frame():
    """the inverse: a TCP4 super-frame of at most m segments -> qgcm_gso_unpack_cpu -> one entry with its payload"""
    rng = np.random.default_rng(11)
    for ihl, doff, gso, paylen, stride in ((20, 20, 1348, 12 * 1024, 1536), (24, 32, 100, 6400, 256), (20, 20, 7, 64 * 7 - 3, 128),
                                           (60, 60, 3, 61, 128)):
        hdr = ihl + doff
        f = M.fields(1)
        f["ihl"][:], f["doff"][:], f["P"][:], f["flags"][:] = ihl, doff, gso, M.ACK | M.PSH
        f["seq"][:], f["id"][:] = 0xFFFFFF00, 0xFFF0
        one, _ = M.build(f, 4 + hdr + gso, rng)
        payload = rng.integers(0, 256, paylen, dtype=np.uint8)
        sup = np.zeros(16 + ((hdr + paylen + 15) & ~15), np.uint8)
        sup[16:16 + hdr] = one[4:4 + hdr]
        sup[16 + hdr:16 + hdr + paylen] = payload
        count = -(-paylen // gso)
        t = np.zeros(1, M.GSO_FRAME)
        t[0] = (16, hdr + paylen, 0, count, gso, hdr, ihl, 0, M.TCP4, 0)
        arena, lens = np.zeros(count * stride, np.uint8), np.zeros(count, np.uint32)
        route.gso_unpack_cpu(sup, len(sup), t, count, arena, stride, lens)
        peer = np.full(count, 5, np.uint32)
        packed, frames, counts = check_equal(arena, stride, count, lens, peer, None)
        assert len(frames) == 1 and tuple(counts) == (1, len(sup), 1, count)
        g = frames[0]
        assert (g["kind"], g["count"], g["gso_size"], g["hdr_len"], g["l4_off"], g["len"]) == (M.TCP4, count, gso, hdr, ihl, hdr + paylen)
        assert np.array_equal(packed[16 + hdr:16 + hdr + paylen], payload)
        assert packed[16 + ihl + 13] == M.ACK | M.PSH


def test_write_gso_checks_the_table_first():
    import os
    r, w = os.pipe()
    try:
        packed = np.zeros(256, np.uint8)
        good = np.zeros(1, M.GSO_FRAME)
        good[0] = (16, 100, 0, 1, 0, 0, 0, 0, M.PLAIN, 0)
        out = np.zeros(3, np.uint64)
        assert route.tun_write_gso(w, packed, 256, good, out) == 1 and out.tolist() == [1, 1, 0]
        assert len(os.read(r, 4096)) == 110
        for bad in ((0, 100, 0, 1, 0, 0, 0, 0, M.PLAIN, 0), (24, 100, 0, 1, 0, 0, 0, 0, M.PLAIN, 0), (16, 241, 0, 1, 0, 0, 0, 0, M.PLAIN, 0),
                    (M.NO_ROOM, 100, 0, 1, 0, 0, 0, 0, M.PLAIN, 0), (16, 100, 0, 1, 0, 0, 20, 16, 1, 0), (16, 100, 0, 1, 0, 0, 0, 0, 3, 0),
                    (16, 100, 0, 3, 30, 40, 20, 16, M.TCP4, 0), (16, 100, 0, 2, 0, 40, 20, 16, M.TCP4, 0), (16, 100, 0, 2, 30, 38, 20, 16, M.TCP4, 0)):
            t = np.concatenate([good, good])
            t[1] = bad
            assert route.tun_write_gso(w, packed, 256, t, out) == -1 and out.tolist() == [0, 0, 0]
        os.set_blocking(r, False)
        with pytest.raises(BlockingIOError):
            os.read(r, 1)  # nothing was written
    finally:
        os.close(r)
        os.close(w)


def test_the_mixed_batch_holds_the_zero_checksum_and_the_ip_option_cases():
    """what the GPU test relies on: in the mixed batch the 0x0000 field merges its three, the 0xffff field splits them,
    and an IP option byte that differs splits a run of six in the middle"""
    for stride in (1536, 128):
        arena, lens, peer, status = K.mixed(stride)
        _, frames, _ = check_equal(arena, stride, len(lens), lens, peer, status)
        by_first = {int(f["first"]): int(f["count"]) for f in frames}
        lo = int(np.flatnonzero((lens == 70) & (arena.reshape(-1, stride)[:, 4 + 20 + 1] == (40015 & 255)))[0])
        assert [by_first.get(lo + k) for k in range(6)] == [3, None, None, 1, 1, 1]
        assert by_first[lo + 6] == 3 and by_first[lo + 9] == 3


def test_an_ip_option_byte_that_differs_splits_the_run():
    b = K.Batch(128)
    K.ip_option_differs(b, b.run(6, 19, ihl=28), 6, 3)
    arena, lens, peer, status = b.done()
    packed, frames, counts = check_equal(arena, 128, 6, lens, peer, status)
    assert frames["first"].tolist() == [0, 3] and frames["l4_off"].tolist() == [28, 28]
    check_anchors(arena, 128, 6, lens, status, packed, frames, counts)
