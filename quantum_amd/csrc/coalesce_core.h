// coalesce_core.h -- the coalescing of delivered TCP segments of include/qgcm.h ("delivered TCP segments coalesced
// on routed batches") as plain C++: which packet is a candidate, when two neighbours link, the frame arithmetic
// (stretch, cut, tail), the table entry of a frame, the table check of qgcm_tun_write_gso and the host coalescing.
// No HIP, no allocation: qgcm_deliver_coalesce_cpu runs it on work arrays of the caller, coalesce_kernels.hip shares
// the header rules, the class word and the frame arithmetic with it, tun_batch.cpp checks the tables it writes
// with it, and tests/cpp_coalesce builds it under the host sanitizers.
//
// Header words are the packet's dwords as a little-endian load gives them (w0 = p[0:4], ...), which is what the
// device's lanes hold; the host loads them with memcpy.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgcm.h"
#include "gso_core.h"
#include "pack_core.h"

#if defined(__HIPCC__)
#define QGCM_CO_HD __host__ __device__
#else
#define QGCM_CO_HD
#endif

namespace qgcm {

constexpr uint32_t kCoNoRoom = 0xffffffffu;  // `off` of an entry that did not fit
constexpr uint32_t kCoLead = 16;             // bytes in front of every packet: six zeros and the vnet header

// The class word of a slot: P | hdr / 4 << 16 | ihl / 4 << 21 | flags.  P, hdr, ihl and PSH are those of a packet
// that passed the header rules (kCoHeader), zero otherwise.
constexpr uint32_t kCoDelivered = 1u << 25;  // status 1 and 4 + L <= stride
constexpr uint32_t kCoCand = 1u << 26;       // a candidate: the header rules and both checksums
constexpr uint32_t kCoHdrLink = 1u << 27;    // the header part of link(i): everything but "both are candidates"
constexpr uint32_t kCoPsh = 1u << 28;
constexpr uint32_t kCoHeader = 1u << 29;     // the header rules hold (checksums not looked at)

QGCM_CO_HD inline uint32_t co_P(uint32_t c) { return c & 0xffffu; }
QGCM_CO_HD inline uint32_t co_hdr(uint32_t c) { return ((c >> 16) & 31u) << 2; }
QGCM_CO_HD inline uint32_t co_ihl(uint32_t c) { return ((c >> 21) & 15u) << 2; }
QGCM_CO_HD inline uint32_t co_swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }
QGCM_CO_HD inline uint32_t co_round16(uint32_t v) { return (v + 15u) & ~15u; }

// The IPv4 part of the candidate rule from the packet's first three dwords.  True: ihl is set and the TCP
// header's first 20 bytes lie inside the packet.
QGCM_CO_HD inline bool co_ip_ok(uint32_t L, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t &ihl) {
    if (L < 40 || L > 65535 || (w0 & 0xf0u) != 0x40u) return false;
    ihl = 4 * (w0 & 15u);
    if (ihl < 20 || ihl > 60 || ihl + 20 > L) return false;
    if (co_swap16(w0 >> 16) != L || ((w2 >> 8) & 0xffu) != 6) return false;
    return (co_swap16(w1 >> 16) & 0xbfffu) == 0;  // no fragment, the reserved bit clear, DF either way
}

// The TCP part from the dword at p[ihl + 12]: data offset, reserved nibble, flags.  True: a class word with P,
// hdr, ihl, PSH and kCoHeader.
QGCM_CO_HD inline bool co_tcp_ok(uint32_t L, uint32_t ihl, uint32_t t3, uint32_t &cls) {
    const uint32_t doff = 4 * ((t3 >> 4) & 15u), flags = (t3 >> 8) & 0xffu;
    if (doff < 20 || doff > 60 || ihl + doff >= L || (t3 & 0x0fu) || (flags & 0xf7u) != 0x10u) return false;
    const uint32_t hdr = ihl + doff;
    cls = (L - hdr) | (hdr >> 2) << 16 | (ihl >> 2) << 21 | (flags & 8u ? kCoPsh : 0u) | kCoHeader;
    return true;
}

// The bits of header dword j (j0 = ihl / 4) that two linked neighbours share: everything but total length, id,
// IPv4 checksum, sequence number, PSH and TCP checksum.
QGCM_CO_HD inline uint32_t co_cmp_mask(uint32_t j, uint32_t j0) {
    if (j == 0) return 0x0000ffffu;
    if (j == 1) return 0xffff0000u;
    if (j == 2) return 0x0000ffffu;
    if (j == j0 + 1) return 0u;
    if (j == j0 + 3) return ~0x00000800u;
    if (j == j0 + 4) return 0xffff0000u;
    return ~0u;
}

// What is left of link(i) once the headers' shared bits are equal: the peer, seq, id and PSH.  w1 / s: the dword
// with the id and the sequence number's dword of each; P_prev the neighbour's payload.
QGCM_CO_HD inline bool co_follows(uint32_t w1_prev, uint32_t s_prev, uint32_t t3_prev, uint32_t P_prev, uint32_t w1, uint32_t s) {
    const uint32_t id_prev = co_swap16(w1_prev), id = co_swap16(w1);
    return __builtin_bswap32(s) == __builtin_bswap32(s_prev) + P_prev && id == ((id_prev + 1) & 0xffffu) && !(t3_prev & 0x0800u);
}

QGCM_CO_HD inline bool co_link(uint32_t prev, uint32_t cur) { return (prev & kCoCand) && (cur & kCoCand) && (cur & kCoHdrLink); }
QGCM_CO_HD inline bool co_eq(uint32_t prev, uint32_t cur) { return co_link(prev, cur) && co_P(cur) == co_P(prev); }
QGCM_CO_HD inline bool co_lt(uint32_t prev, uint32_t cur) { return co_link(prev, cur) && co_P(cur) < co_P(prev); }

// The cut limit of a candidate's stretch: at least 1, because hdr + P <= 65535
QGCM_CO_HD inline uint32_t co_m(uint32_t c) {
    const uint32_t by_len = (65535u - co_hdr(c)) / co_P(c);
    return by_len < QGCM_COALESCE_SEGS ? by_len : QGCM_COALESCE_SEGS;
}

// What a delivered slot is in its frame.
struct CoRole {
    bool end;            // the frame's last member: the one that names the entry
    uint32_t count;      // members up to and including this one
    uint32_t payload;    // their payload bytes (a candidate's)
    uint32_t rel;        // where this member's payload goes in the frame (the head: hdr)
};

// cls(x): the class word of slot x, 0 for x outside [0, n); head(x): the head of x's stretch (the last slot at or
// below x with !eq), asked for candidates only.
template <class Cls, class Head>
QGCM_CO_HD inline bool co_is_tail(const Cls &cls, const Head &head, int64_t t) {
    const uint32_t prev = cls(t - 1), cur = cls(t);
    if (!co_lt(prev, cur) || co_eq(cur, cls(t + 1)) || co_lt(cls(t - 2), prev)) return false;
    const uint32_t m = co_m(prev);
    return (uint32_t)(t - 1 - head(t - 1)) % m + 1 < m;
}

template <class Cls, class Head>
QGCM_CO_HD inline CoRole co_role(const Cls &cls, const Head &head, int64_t i) {
    const uint32_t c = cls(i);
    if (!(c & kCoCand)) return CoRole{true, 1, 0, 0};
    if (co_is_tail(cls, head, i)) {
        const uint32_t prev = cls(i - 1);
        const uint32_t before = (uint32_t)(i - 1 - head(i - 1)) % co_m(prev) + 1;
        return CoRole{true, before + 1, before * co_P(prev) + co_P(c), co_hdr(c) + before * co_P(prev)};
    }
    const uint32_t m = co_m(c), r = (uint32_t)(i - head(i)) % m;
    const bool last = !co_eq(c, cls(i + 1)) || r + 1 == m;
    return CoRole{last && !co_is_tail(cls, head, i + 1), r + 1, (r + 1) * co_P(c), co_hdr(c) + r * co_P(c)};
}

// The entry of the frame that ends at slot e (class word c, length L, role r), its region starting at byte
// `start` of the packed area.
QGCM_CO_HD inline qgcm_gso_frame co_entry(uint32_t c, uint32_t L, const CoRole &r, uint32_t e, uint64_t start, uint64_t cap, uint32_t peer) {
    qgcm_gso_frame f;
    f.len = r.count == 1 ? L : co_hdr(c) + r.payload;
    f.off = start + kCoLead + co_round16(f.len) <= cap ? (uint32_t)(start + kCoLead) : kCoNoRoom;
    f.first = e - (r.count - 1);
    f.count = r.count;
    const bool tcp = r.count > 1;
    // gso_size is the head's P: the last member's own payload is the tail's when it is shorter
    f.gso_size = tcp ? (uint16_t)((r.payload - co_P(c)) / (r.count - 1)) : 0;
    f.hdr_len = tcp ? (uint16_t)co_hdr(c) : 0;
    f.l4_off = tcp ? (uint16_t)co_ihl(c) : 0;
    f.csum_off = tcp ? 16 : 0;
    f.kind = tcp ? QGCM_GSO_TCP4 : QGCM_GSO_PLAIN;
    f.reserved = peer;
    return f;
}

// The bytes an entry takes in the packed area: the lead and the packet, padded to 16
QGCM_CO_HD inline uint64_t co_region(uint32_t len) { return (uint64_t)kCoLead + co_round16(len); }

// What qgcm_tun_write_gso asks of a table: every entry behind its lead and inside the packed area, PLAIN or TCP4,
// a TCP4 entry valid by gso_core.h's rule apart from `first`.
inline bool co_table_ok(const qgcm_gso_frame *frames, uint32_t m, uint64_t packed_len) {
    for (uint32_t k = 0; k < m; ++k) {
        qgcm_gso_frame f = frames[k];
        if (f.off < kCoLead || (f.off & 15u) || (uint64_t)f.off + f.len > packed_len) return false;
        if (f.kind != QGCM_GSO_PLAIN && f.kind != QGCM_GSO_TCP4) return false;
        f.first = 0;
        if (f.kind == QGCM_GSO_TCP4 && !gso_valid(f, packed_len, QGCM_GSO_SEGS)) return false;
    }
    return true;
}

// qgcm_tun_write_gso's way out for a queue that refuses a super-frame (tun_batch.cpp): a valid TCP4 entry cut on
// the host and written packet by packet behind zero vnet headers; the packets written.
int tun_write_gso_cut(int fd, const uint8_t *packed, const qgcm_gso_frame &f);

// ---- the host coalescing: bytes in network order (gso_core.h's sums) ----

inline uint32_t co_load32(const uint8_t *p) {
    uint32_t w;
    memcpy(&w, p, 4);
    return w;
}

// The class word of slot i without kCoHdrLink.
inline uint32_t co_classify_cpu(const uint8_t *arena, uint64_t stride, uint32_t i, const uint32_t *lens, const uint8_t *status) {
    const uint32_t L = lens[i];
    if (!pack_delivered(status ? status[i] : 1u, L, stride)) return 0;
    const uint8_t *p = arena + (uint64_t)i * stride + kGsoPacketStart;
    uint32_t ihl, cls = 0;
    if (L < 40 || !co_ip_ok(L, co_load32(p), co_load32(p + 4), co_load32(p + 8), ihl)) return kCoDelivered;
    if (!co_tcp_ok(L, ihl, co_load32(p + ihl + 12), cls)) return kCoDelivered;
    cls |= kCoDelivered;
    if (gso_get16(p + 10) != gso_fold_not(gso_sum_be(p, 10) + gso_sum_be(p + 12, ihl - 12))) return cls;
    const uint64_t pseudo = gso_sum_be(p + 12, 8) + 6u + (L - ihl);
    const uint64_t sum = gso_sum_be(p + ihl + 18, (uint64_t)L - ihl - 18, gso_sum_be(p + ihl, 16, pseudo));
    if (gso_get16(p + ihl + 16) != gso_fold_not(sum)) return cls;
    return cls | kCoCand;
}

// kCoHdrLink of slot i >= 1, whose class word c has kCoHeader: its neighbour is delivered, holds as many header
// bytes, and follows.
inline bool co_hdr_link_cpu(const uint8_t *arena, uint64_t stride, uint32_t i, const uint32_t *lens, const uint32_t *peer,
                            uint32_t c, uint32_t c_prev) {
    const uint32_t hdr = co_hdr(c), j0 = co_ihl(c) >> 2, L_prev = lens[i - 1];
    if (!(c_prev & kCoDelivered) || L_prev < hdr || peer[i] != peer[i - 1]) return false;
    const uint8_t *p = arena + (uint64_t)i * stride + kGsoPacketStart, *q = p - stride;
    for (uint32_t j = 0; j < hdr >> 2; ++j)
        if ((co_load32(p + 4 * j) ^ co_load32(q + 4 * j)) & co_cmp_mask(j, j0)) return false;
    return co_follows(co_load32(q + 4), co_load32(q + 4 * j0 + 4), co_load32(q + 4 * j0 + 12), L_prev - hdr, co_load32(p + 4),
                      co_load32(p + 4 * j0 + 4));
}

// The lead of an entry: six zero bytes and the vnet header, in host byte order
inline void co_put_lead(uint8_t *at, const qgcm_gso_frame &f) {
    memset(at, 0, kCoLead);
    if (f.kind != QGCM_GSO_TCP4) return;
    const uint16_t v[4] = {f.hdr_len, f.gso_size, f.l4_off, f.csum_off};
    at[6] = 1;  // VIRTIO_NET_HDR_F_NEEDS_CSUM
    at[7] = 1;  // VIRTIO_NET_HDR_GSO_TCPV4
    memcpy(at + 8, v, 8);
}

// The coalescing by the host.  cls and head: n words each, the caller's.
inline void deliver_coalesce_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                                 const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_gso_frame *frames,
                                 uint64_t counts[4], uint32_t *cls, uint32_t *head) {
    for (uint32_t i = 0; i < n; ++i) cls[i] = co_classify_cpu(arena, stride, i, lens, status);
    for (uint32_t i = 0; i < n; ++i) {
        if (i && (cls[i] & kCoHeader) && co_hdr_link_cpu(arena, stride, i, lens, peer, cls[i], cls[i - 1])) cls[i] |= kCoHdrLink;
        head[i] = i && co_eq(cls[i - 1], cls[i]) ? head[i - 1] : i;
    }
    const auto cls_at = [&](int64_t x) { return x < 0 || x >= (int64_t)n ? 0u : cls[x]; };
    const auto head_at = [&](int64_t x) { return (int64_t)head[x]; };
    uint64_t entries = 0, bytes = 0, coalesced = 0, delivered = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(cls[i] & kCoDelivered)) continue;
        ++delivered;
        const CoRole r = co_role(cls_at, head_at, i);
        if (!r.end) continue;
        const qgcm_gso_frame f = co_entry(cls[i], lens[i], r, i, bytes, packed_cap, peer[i - (r.count - 1)]);
        frames[entries++] = f;
        bytes += co_region(f.len);
        coalesced += f.count > 1;
        if (f.off == kCoNoRoom) continue;
        uint8_t *pkt = packed + f.off;
        const uint8_t *src = arena + (uint64_t)f.first * stride + kGsoPacketStart;
        co_put_lead(pkt - kCoLead, f);
        if (f.count == 1) {
            memcpy(pkt, src, f.len);
        } else {
            memcpy(pkt, src, f.hdr_len);
            uint32_t at = f.hdr_len;
            for (uint32_t k = 0; k < f.count; ++k) {
                const uint32_t P = co_P(cls[f.first + k]);
                memcpy(pkt + at, src + (uint64_t)k * stride + f.hdr_len, P);
                at += P;
            }
            gso_put16(pkt + 2, f.len);
            gso_put16(pkt + 10, 0);
            gso_put16(pkt + 10, gso_fold_not(gso_sum_be(pkt, f.l4_off)));
            uint8_t *tcp = pkt + f.l4_off;
            tcp[13] = (uint8_t)((tcp[13] & ~8u) | (cls[i] & kCoPsh ? 8u : 0u));
            gso_put16(tcp + 16, (uint16_t)~gso_fold_not(gso_sum_be(pkt + 12, 8) + 6u + (f.len - f.l4_off)));
        }
        memset(pkt + f.len, 0, co_round16(f.len) - f.len);
    }
    counts[0] = entries;
    counts[1] = bytes;
    counts[2] = coalesced;
    counts[3] = delivered;
}

}  // namespace qgcm
