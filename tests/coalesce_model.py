"""The contract of include/qgcm.h "delivered TCP segments coalesced on routed batches" restated in numpy, from the
header's text: which delivered packet is a candidate, when neighbours link, stretches, the cut, the tail, and the
packed area with its table.  Vectorised, so that half a million slots take seconds.  Also the batch builder of
the coalescing tests: TCP segments with valid checksums from per-slot field arrays."""
import numpy as np

GSO_FRAME = [("off", "<u4"), ("len", "<u4"), ("first", "<u4"), ("count", "<u4"), ("gso_size", "<u2"), ("hdr_len", "<u2"),
             ("l4_off", "<u2"), ("csum_off", "<u2"), ("kind", "<u4"), ("reserved", "<u4")]
PLAIN, TCP4 = 0, 2
SEGS = 64
NO_ROOM = 0xFFFFFFFF
ACK, PSH, FIN, SYN, RST, URG, ECE = 0x10, 0x08, 0x01, 0x02, 0x04, 0x20, 0x40


def fold(s):
    s = np.asarray(s, np.uint64).copy()
    while (s >> np.uint64(16)).any():
        s = (s & np.uint64(0xFFFF)) + (s >> np.uint64(16))
    return s


def _be16(rows, at):
    """the 16-bit big-endian word at byte `at` (an array, one per row) of each row"""
    i = np.arange(len(rows))
    return rows[i, at].astype(np.int64) << 8 | rows[i, at + 1]


def _word_sums(pk, lo, hi):
    """per row the sum of the big-endian 16-bit words of bytes [lo, hi) (lo even; an odd end padded with zero)"""
    w = pk.shape[1] & ~1
    col = np.arange(w)
    b = np.ascontiguousarray(pk[:, :w])
    b = b * ((col >= lo[:, None]) & (col < hi[:, None]))
    return b.view(">u2").sum(axis=1, dtype=np.uint64)


def classify(arena, stride, n, lens, status):
    """per slot: delivered, candidate, ihl, hdr, P, psh (the last four meaningful for candidates)"""
    rows = np.ascontiguousarray(arena[:n * stride]).reshape(n, stride)
    pk = rows[:, 4:]
    L = lens.astype(np.int64)
    delivered = (np.ones(n, bool) if status is None else status == 1) & (4 + L <= stride)
    ok = delivered & (L >= 40) & (L <= 0xFFFF)
    Lc = np.where(ok, L, 40)
    ok &= pk[:, 0] >> 4 == 4
    ihl = 4 * (pk[:, 0] & 15).astype(np.int64)
    ok &= (ihl >= 20) & (ihl <= 60) & (ihl + 20 <= Lc)
    ihl = np.where(ok, ihl, 20)
    zero = np.zeros(n, np.int64)
    ok &= (_be16(pk, zero + 2) == Lc) & (pk[:, 9] == 6) & (_be16(pk, zero + 6) & 0xBFFF == 0)
    i = np.arange(n)
    doff = 4 * (pk[i, ihl + 12] >> 4).astype(np.int64)
    ok &= (doff >= 20) & (doff <= 60) & (pk[i, ihl + 12] & 15 == 0) & (pk[i, ihl + 13] & 0xF7 == 0x10)
    hdr = ihl + doff
    ok &= Lc - hdr >= 1
    hdr = np.where(ok, hdr, 40)
    # both checksums recomputed with their fields taken as zero
    sel = np.flatnonzero(ok)
    cand = np.zeros(n, bool)
    if len(sel):
        p, ih, ln = pk[sel], ihl[sel], Lc[sel]
        ip_field, tcp_field = _be16(p, ih * 0 + 10), _be16(p, ih + 16)
        ip = _word_sums(p, ih * 0, ih) - ip_field.astype(np.uint64)
        tcp = _word_sums(p, ih, ln) - tcp_field.astype(np.uint64)
        tcp += _word_sums(p, ih * 0 + 12, ih * 0 + 20) + np.uint64(6) + (ln - ih).astype(np.uint64)
        cand[sel] = ((fold(ip) ^ np.uint64(0xFFFF)) == ip_field) & ((fold(tcp) ^ np.uint64(0xFFFF)) == tcp_field)
    return dict(delivered=delivered, cand=cand, ihl=ihl, hdr=hdr, P=np.where(ok, Lc - hdr, 0), psh=pk[i, ihl + 13] & 8 != 0)


def links(arena, stride, n, peer, c):
    """link(i) for every slot, False at 0"""
    pk = np.ascontiguousarray(arena[:n * stride]).reshape(n, stride)[:, 4:]
    link = np.zeros(n, bool)
    if n < 2:
        return link
    both = c["cand"][1:] & c["cand"][:-1] & (peer[1:] == peer[:-1]) & (c["hdr"][1:] == c["hdr"][:-1]) & (c["ihl"][1:] == c["ihl"][:-1])
    sel = np.flatnonzero(both) + 1
    if not len(sel):
        return link
    a, b, ihl, hdr = pk[sel - 1, :120], pk[sel, :120], c["ihl"][sel][:, None], c["hdr"][sel][:, None]
    col = np.arange(a.shape[1])[None, :]
    free = (col >= hdr) | ((col >= 2) & (col < 6)) | (col == 10) | (col == 11) | ((col >= ihl + 4) & (col < ihl + 8)) | \
        (col == ihl + 16) | (col == ihl + 17)
    diff = a ^ b
    diff[col == ihl + 13] &= 0xF7
    same = ((diff == 0) | free).all(axis=1)
    ih = c["ihl"][sel]

    def seq(p):
        return _be16(p, ih + 4) << 16 | _be16(p, ih + 6)

    same &= seq(b) == (seq(a) + c["P"][sel - 1]) & 0xFFFFFFFF
    same &= _be16(b, ih * 0 + 4) == (_be16(a, ih * 0 + 4) + 1) & 0xFFFF
    same &= ~c["psh"][sel - 1]
    link[sel] = same
    return link


def plan(c, link):
    """per slot `joined` (in the frame of slot i - 1), from eq, lt, the cut and the tail rule"""
    n = len(link)
    P = c["P"]
    eq, lt = link.copy(), link.copy()
    eq[1:] &= P[1:] == P[:-1]
    lt[1:] &= P[1:] < P[:-1]
    idx = np.arange(n)
    head = np.maximum.accumulate(np.where(eq, 0, idx))
    j = idx - head
    m = np.minimum(SEGS, (65535 - c["hdr"]) // np.maximum(P, 1))
    m = np.maximum(m, 1)
    eq_next = np.append(eq[1:], False)
    lt_prev = np.insert(lt[:-1], 0, False)
    members_prev = np.insert((j % m + 1)[:-1], 0, 0)  # of the frame that ends at t - 1 (no tail itself: !lt(t - 1))
    m_prev = np.insert(m[:-1], 0, 1)
    tail = lt & ~eq_next & ~lt_prev & (members_prev < m_prev)
    return (eq & (j % m != 0)) | tail, tail


def coalesce(arena, stride, n, lens, peer, status, packed, cap=None):
    """-> (packed as the call leaves it, from the caller's `packed`; frames; counts)"""
    out = packed.copy()
    cap = len(out) if cap is None else cap
    if n == 0:
        return out, np.zeros(0, GSO_FRAME), np.zeros(4, np.uint64)
    c = classify(arena, stride, n, lens, status)
    link = links(arena, stride, n, peer, c)
    joined, _ = plan(c, link)
    dl = np.flatnonzero(c["delivered"])
    starts = dl[~joined[dl]]
    fid = np.cumsum(~joined[dl]) - 1
    k = len(starts)
    count = np.bincount(fid, minlength=k)
    merged = count > 1
    P, hdr, L = c["P"][dl], c["hdr"][dl], lens[dl].astype(np.int64)
    paysum = np.bincount(fid, weights=P, minlength=k).astype(np.int64)
    flen = np.where(merged, c["hdr"][starts] + paysum, lens[starts].astype(np.int64))
    region = 16 + ((flen + 15) & ~15)
    end = np.cumsum(region)
    off = end - region + 16
    fits = end <= cap
    frames = np.zeros(k, GSO_FRAME)
    frames["off"] = np.where(fits, off, NO_ROOM)
    frames["len"], frames["first"], frames["count"] = flen, starts, count
    frames["gso_size"] = np.where(merged, c["P"][starts], 0)
    frames["hdr_len"] = np.where(merged, c["hdr"][starts], 0)
    frames["l4_off"] = np.where(merged, c["ihl"][starts], 0)
    frames["csum_off"] = np.where(merged, 16, 0)
    frames["kind"] = np.where(merged, TCP4, PLAIN)
    frames["reserved"] = peer[starts]
    counts = np.array([k, end[-1] if k else 0, merged.sum(), len(dl)], np.uint64)
    if not fits.any():
        return out, frames, counts
    out[:end[fits][-1]] = 0
    # every member's bytes: the first member its whole packet, a later one its payload behind the ones before
    first = ~joined[dl]
    nb = np.where(first, L, P)
    before = np.cumsum(np.where(first, 0, P))  # payload of later members so far ...
    before -= np.maximum.accumulate(np.where(first, before, 0))  # ... within the frame, this member included
    dst = off[fid] + np.where(first, 0, c["hdr"][starts][fid] + c["P"][starts][fid] + before - P)
    src = dl * stride + 4 + np.where(first, 0, hdr)
    keep = fits[fid] & (nb > 0)
    nb, dst, src = nb[keep], dst[keep], src[keep]
    within = np.arange(nb.sum()) - np.repeat(np.cumsum(nb) - nb, nb)
    out[np.repeat(dst, nb) + within] = arena[np.repeat(src, nb) + within]
    # the merged frames' headers and leads
    mf = np.flatnonzero(merged & fits)
    if len(mf):
        o, ln, ih = off[mf], flen[mf], c["ihl"][starts[mf]]
        last = starts[mf] + count[mf] - 1
        out[o + 2], out[o + 3] = ln >> 8, ln & 255
        out[o + ih + 13] = (out[o + ih + 13] & 0xF7) | np.where(c["psh"][last], 8, 0)
        out[o + 10] = out[o + 11] = 0
        hd = out[np.minimum(o[:, None] + np.arange(60)[None, :], len(out) - 1)]
        ip = fold(_word_sums(hd, ih * 0, ih)) ^ np.uint64(0xFFFF)
        out[o + 10], out[o + 11] = ip >> np.uint64(8), ip & np.uint64(255)
        ps = fold(_word_sums(hd, ih * 0 + 12, ih * 0 + 20) + np.uint64(6) + (ln - ih).astype(np.uint64))
        out[o + ih + 16], out[o + ih + 17] = ps >> np.uint64(8), ps & np.uint64(255)
        vnet = np.zeros((len(mf), 5), "<u2")
        vnet[:, 0] = 0x0101  # flags NEEDS_CSUM, gso_type TCPV4
        vnet[:, 1], vnet[:, 2], vnet[:, 3], vnet[:, 4] = c["hdr"][starts[mf]], c["P"][starts[mf]], ih, 16
        out[(o - 10)[:, None] + np.arange(10)[None, :]] = vnet.view(np.uint8).reshape(len(mf), 10)
    return out, frames, counts


def coalesce_chunks(arena, stride, n, lens, peer, status, chunk):
    """the pipelines' result: coalesce chunk by chunk, the areas one behind the other, `off` and `first` rebased"""
    areas, tables, total = [], [], np.zeros(4, np.uint64)
    for c0 in range(0, n, chunk):
        cn = min(chunk, n - c0)
        st = None if status is None else status[c0:c0 + cn]
        area = np.zeros(cn * (((stride + 15) & ~15) + 16), np.uint8)
        area, fr, counts = coalesce(arena[c0 * stride:(c0 + cn) * stride], stride, cn, lens[c0:c0 + cn], peer[c0:c0 + cn], st, area)
        fr["off"] += np.uint32(total[1])
        fr["first"] += np.uint32(c0)
        areas.append(area[:int(counts[1])])
        tables.append(fr)
        total += counts
    return (np.concatenate(areas) if areas else np.zeros(0, np.uint8)), (np.concatenate(tables) if tables else np.zeros(0, GSO_FRAME)), total


# ---- the batch builder ----

def fields(n, rng=None):
    """per-slot field arrays of n TCP segments of one default flow, to be edited before build()"""
    z = np.zeros(n, np.int64)
    return dict(src=z + 0x0A000002, dst=z + 0x0A000001, sport=z + 40000, dport=z + 5001, seq=z.copy(), ack=z + 1, win=z + 512,
                urg=z.copy(), id=z.copy(), ttl=z + 64, tos=z.copy(), frag=z + 0x4000, flags=z + ACK, ihl=z + 20, doff=z + 20,
                P=z + 100, opt=z.copy(), proto=z + 6)


def run(f, lo, count, P, seq0=1000, id0=1, flow=0, **over):
    """slots [lo, lo + count) of `f` become consecutive segments of flow `flow` (P a number or a sequence)"""
    s = slice(lo, lo + count)
    P = np.broadcast_to(np.asarray(P, np.int64), (count,))
    f["P"][s] = P
    f["seq"][s] = (seq0 + np.cumsum(P) - P) & 0xFFFFFFFF
    f["id"][s] = (id0 + np.arange(count)) & 0xFFFF
    f["sport"][s] = 40000 + flow
    f["opt"][s] = flow
    for k, v in over.items():
        f[k][s] = v


def build(f, stride, rng, fix=True):
    """-> (arena uint8 (n * stride), lens uint32): the packets at Raw[4:], checksums valid, Raw[0:4] and the slot
    tails random"""
    n = len(f["P"])
    rows = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    pk = rows[:, 4:]
    ihl, doff = f["ihl"], f["doff"]
    L = ihl + doff + f["P"]
    assert (4 + L <= stride).all()
    i = np.arange(n)

    def put16(at, v):
        pk[i, at], pk[i, at + 1] = (v >> 8) & 255, v & 255

    # options: bytes that depend on the flow and the place only
    col = np.arange(min(120, stride - 4))[None, :]
    pk[:, :120] = np.where(col < (ihl + doff)[:, None], (f["opt"][:, None] * 37 + col * 11 + 1) & 255, pk[:, :120])
    z = i * 0
    pk[:, 0], pk[:, 1] = 0x40 | ihl >> 2, f["tos"]
    put16(z + 2, L)
    put16(z + 4, f["id"])
    put16(z + 6, f["frag"])
    pk[:, 8], pk[:, 9] = f["ttl"], f["proto"]
    put16(z + 10, z)
    for k, at in (("src", 12), ("dst", 16)):
        put16(z + at, f[k] >> 16)
        put16(z + at + 2, f[k] & 0xFFFF)
    put16(ihl, f["sport"])
    put16(ihl + 2, f["dport"])
    for k, at in (("seq", 4), ("ack", 8)):
        put16(ihl + at, f[k] >> 16)
        put16(ihl + at + 2, f[k] & 0xFFFF)
    pk[i, ihl + 12], pk[i, ihl + 13] = doff >> 2 << 4, f["flags"]
    put16(ihl + 14, f["win"])
    put16(ihl + 16, z)
    put16(ihl + 18, f["urg"])
    arena, lens = rows.reshape(-1), L.astype(np.uint32)
    if fix:
        fix_checksums(arena, stride, i, lens)
    return arena, lens


def fix_checksums(arena, stride, slots, lens):
    """recompute both checksums of the TCP packets in `slots` (ihl and total length taken from the packets)"""
    slots = np.atleast_1d(np.asarray(slots))
    rows = arena.reshape(-1, stride)
    pk = rows[slots, 4:]
    ihl = 4 * (pk[:, 0] & 15).astype(np.int64)
    L = lens[slots].astype(np.int64)
    i = np.arange(len(slots))
    pk[:, 10] = pk[:, 11] = 0
    pk[i, ihl + 16] = pk[i, ihl + 17] = 0
    ip = fold(_word_sums(pk, ihl * 0, ihl)) ^ np.uint64(0xFFFF)
    tcp = _word_sums(pk, ihl, L) + _word_sums(pk, ihl * 0 + 12, ihl * 0 + 20) + np.uint64(6) + (L - ihl).astype(np.uint64)
    tcp = fold(tcp) ^ np.uint64(0xFFFF)
    pk[:, 10], pk[:, 11] = ip >> np.uint64(8), ip & np.uint64(255)
    pk[i, ihl + 16], pk[i, ihl + 17] = tcp >> np.uint64(8), tcp & np.uint64(255)
    rows[slots, 4:] = pk
