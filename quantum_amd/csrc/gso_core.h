// gso_core.h -- the super-frame table of include/qgcm.h ("TUN super-frames segmented on routed batches") as plain
// C++: when an entry is valid, the payload of a segment, the search of a slot's entry, the table check of the host
// entry points and the host segmentation.  No HIP, no allocation: qgcm_gso_unpack_cpu runs it, gso_kernels.hip
// shares the validity rule, the segment lengths and the search with it, route.cpp checks its tables with it,
// tun_batch.cpp checks the entries it writes with it, and tests/cpp_gso builds it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_GSO_HD __host__ __device__
#else
#define QGCM_GSO_HD
#endif

namespace qgcm {

constexpr uint64_t kGsoPacketStart = 4;     // common.PacketStart: a packet lands at Raw[4:]
constexpr uint64_t kGsoVnetHdr = 10;        // struct virtio_net_hdr, what TUNSETVNETHDRSZ is set to
constexpr uint64_t kGsoRoom = 65536 + 16;   // qgcm_tun_read_gso reads only with this much room: no frame is cut
constexpr uint32_t kGsoMaxHdr = 120;        // IPv4 and TCP headers at their longest: 60 + 60

// ceil((len - hdr_len) / gso_size) for hdr_len < len and gso_size >= 1
QGCM_GSO_HD inline uint32_t gso_seg_count(uint32_t len, uint32_t hdr_len, uint32_t gso_size) {
    return (len - hdr_len - 1) / gso_size + 1;  // (32 bits: the device has no 64-bit divide)
}

// The validity rule of include/qgcm.h, from the entry alone.
QGCM_GSO_HD inline bool gso_valid(const qgcm_gso_frame &f, uint64_t packed_len, uint32_t n) {
    if ((f.off & 15u) || (uint64_t)f.off + f.len > packed_len || (uint64_t)f.first + f.count > n || f.kind > QGCM_GSO_UDP4)
        return false;
    if (f.kind == QGCM_GSO_PLAIN) return f.count == 1;
    if (f.kind == QGCM_GSO_CSUM)
        return f.count == 1 && !(f.l4_off & 1u) && !(f.csum_off & 1u) && (uint32_t)f.l4_off + f.csum_off + 2u <= f.len;
    if (f.l4_off < 20 || f.l4_off > 60 || (f.l4_off & 3u) || f.hdr_len <= f.l4_off) return false;
    const uint32_t l4 = (uint32_t)f.hdr_len - f.l4_off;
    if (f.kind == QGCM_GSO_UDP4 ? l4 != 8 : (l4 < 20 || l4 > 60 || (l4 & 3u))) return false;
    if (f.hdr_len >= f.len || f.gso_size == 0) return false;
    return f.count <= QGCM_GSO_SEGS && f.count == gso_seg_count(f.len, f.hdr_len, f.gso_size);
}

// Payload bytes of segment k (k < count) of a valid TCP4 / UDP4 entry.
QGCM_GSO_HD inline uint32_t gso_seg_payload(const qgcm_gso_frame &f, uint32_t k) {
    const uint32_t left = f.len - f.hdr_len - k * (uint32_t)f.gso_size;
    return left < f.gso_size ? left : f.gso_size;
}

// The entry of slot i (i < n, n_frames >= 1): the index of the last entry whose first is at or below i (0 when
// none is) in a table whose `first` values ascend; on any other table some index below n_frames.  Every read of
// the table lies below n_frames.  gro_find (gro_core.h) over this table: the guess of equal counts, the bracket
// grown in doubling steps, then halved.
QGCM_GSO_HD inline uint32_t gso_find(const qgcm_gso_frame *t, uint32_t n_frames, uint32_t n, uint64_t i) {
    uint32_t lo = 0, hi = n_frames;
    const uint32_t guess = (uint32_t)(i * n_frames / n);
    if (t[guess].first <= i) {
        lo = guess;
        uint32_t step = 1;
        while (hi - lo > step && t[lo + step].first <= i) {
            lo += step;
            step <<= 1;
        }
        if (hi - lo > step) hi = lo + step;
    } else {
        hi = guess;
        uint32_t step = 1;
        while (step <= hi && t[hi - step].first > i) {
            hi -= step;
            step <<= 1;
        }
        lo = step <= hi ? hi - step : 0;
    }
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t[mid].first <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// What the host entry points ask of a table: every entry valid, each `first` the sum of the counts before it,
// n slots in all.
inline bool gso_table_ok(const qgcm_gso_frame *frames, uint32_t n_frames, uint32_t n, uint64_t packed_len) {
    uint64_t at = 0;
    for (uint32_t e = 0; e < n_frames; ++e) {
        if (frames[e].first != at || !gso_valid(frames[e], packed_len, n)) return false;
        at += frames[e].count;
    }
    return at == n;
}

// ---- the host segmentation: bytes in network order, one 16-bit word at a time ----

inline uint64_t gso_sum_be(const uint8_t *p, uint64_t bytes, uint64_t sum = 0) {
    uint64_t i = 0;
    for (; i + 1 < bytes; i += 2) sum += (uint32_t)p[i] << 8 | p[i + 1];
    if (i < bytes) sum += (uint32_t)p[i] << 8;  // an odd byte is padded with a zero
    return sum;
}

inline uint16_t gso_fold_not(uint64_t sum) {
    while (sum >> 16) sum = (sum & 0xffff) + (sum >> 16);
    return (uint16_t)~sum;
}

inline void gso_put16(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}

inline uint32_t gso_get16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }

// the first min(bytes, room) bytes
inline void gso_copy_clamped(uint8_t *dst, const uint8_t *src, uint64_t bytes, uint64_t room) {
    if (bytes > room) bytes = room;
    if (bytes) memcpy(dst, src, (size_t)bytes);
}

// One valid entry into its slots: lens[i] and Raw[4 : 4 + min(L, stride - 4)) of each.
inline void gso_unpack_entry_cpu(const uint8_t *packed, const qgcm_gso_frame &f, uint8_t *arena, uint64_t stride, uint32_t *lens) {
    const uint8_t *pkt = packed + f.off;
    const uint64_t room = stride - kGsoPacketStart;
    if (f.kind == QGCM_GSO_PLAIN || f.kind == QGCM_GSO_CSUM) {
        uint8_t *dst = arena + (uint64_t)f.first * stride + kGsoPacketStart;
        lens[f.first] = f.len;
        gso_copy_clamped(dst, pkt, f.len, room);
        if (f.kind == QGCM_GSO_CSUM) {
            uint16_t c = gso_fold_not(gso_sum_be(pkt + f.l4_off, (uint64_t)f.len - f.l4_off));
            if (c == 0) c = 0xffff;
            uint8_t field[2];
            gso_put16(field, c);
            const uint64_t at = (uint64_t)f.l4_off + f.csum_off;
            if (at < room) gso_copy_clamped(dst + at, field, 2, room - at);
        }
        return;
    }
    const bool tcp = f.kind == QGCM_GSO_TCP4;
    const uint32_t id0 = gso_get16(pkt + 4);
    const uint32_t seq0 = (uint32_t)gso_get16(pkt + f.l4_off + 4) << 16 | gso_get16(pkt + f.l4_off + 6);
    for (uint32_t k = 0; k < f.count; ++k) {
        const uint32_t P = gso_seg_payload(f, k), L = f.hdr_len + P;
        const uint8_t *payload = pkt + f.hdr_len + (uint64_t)k * f.gso_size;
        uint8_t h[kGsoMaxHdr];
        memcpy(h, pkt, f.hdr_len);
        gso_put16(h + 2, L & 0xffff);
        gso_put16(h + 4, (id0 + k) & 0xffff);
        gso_put16(h + 10, 0);
        gso_put16(h + 10, gso_fold_not(gso_sum_be(h, f.l4_off)));
        uint8_t *l4 = h + f.l4_off;
        const uint32_t l4_len = (L - f.l4_off) & 0xffff;
        uint32_t at;  // of the checksum in the L4 header
        if (tcp) {
            const uint32_t seq = seq0 + k * (uint32_t)f.gso_size;
            gso_put16(l4 + 4, seq >> 16);
            gso_put16(l4 + 6, seq & 0xffff);
            if (k + 1 != f.count) l4[13] &= (uint8_t)~0x09u;  // FIN, PSH
            at = 16;
        } else {
            gso_put16(l4 + 4, l4_len);
            at = 6;
        }
        gso_put16(l4 + at, 0);
        uint64_t sum = gso_sum_be(h + 12, 8) + (tcp ? 6u : 17u) + l4_len;  // the pseudo-header
        sum = gso_sum_be(l4, (uint64_t)f.hdr_len - f.l4_off, sum);
        uint16_t c = gso_fold_not(gso_sum_be(payload, P, sum));
        if (!tcp && c == 0) c = 0xffff;
        gso_put16(l4 + at, c);
        const uint64_t i = (uint64_t)f.first + k;
        uint8_t *dst = arena + i * stride + kGsoPacketStart;
        lens[i] = L;
        gso_copy_clamped(dst, h, f.hdr_len, room);
        if (room > f.hdr_len) gso_copy_clamped(dst + f.hdr_len, payload, P, room - f.hdr_len);
    }
}

// qgcm_gso_unpack_cpu whole: the arguments, the table, then the segmentation.
inline int gso_unpack_checked(const uint8_t *packed, uint64_t packed_len, const qgcm_gso_frame *frames, uint32_t n_frames,
                              uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens) {
    if (n > QGCM_MAX_BATCH || n_frames > n || (stride & 3) || stride < 8) return QGCM_E_ARG;
    if (n && (!packed || !frames || !arena || !lens)) return QGCM_E_ARG;
    if (!gso_table_ok(frames, n_frames, n, packed_len)) return QGCM_E_ARG;
    for (uint32_t e = 0; e < n_frames; ++e) gso_unpack_entry_cpu(packed, frames[e], arena, stride, lens);
    return QGCM_OK;
}

}  // namespace qgcm
