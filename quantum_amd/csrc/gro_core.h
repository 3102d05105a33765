// gro_core.h -- the coalesced receive of include/qgcm.h ("coalesced receive on routed batches") as plain
// C++: the datagram count of a buffer, the skip rule, the search of a slot's buffer, the table check of the host
// entry points and the host unpack.  No HIP, no allocation: qgcm_gro_unpack_cpu runs it, gro_kernels.hip and
// gro_resolve_kernels.hip share the count, the skip rule and the search with it, route.cpp checks its tables
// with it, and tests/cpp_gro and tests/cpp_gro_resolve build it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_GRO_HD __host__ __device__
#else
#define QGCM_GRO_HD
#endif

namespace qgcm {

// Datagrams in a buffer of `len` bytes cut every `seg_len`: 1 for a lone datagram (no control message, or one
// segment that is not full), else ceil(len / seg_len).  64-bit: len is whatever the table says.
QGCM_GRO_HD inline uint64_t gro_count(uint32_t len, uint32_t seg_len) {
    if (seg_len == 0 || seg_len >= len) return 1;
    return ((uint64_t)len + seg_len - 1) / seg_len;
}

// Length of datagram k (k < gro_count) of such a buffer.
QGCM_GRO_HD inline uint32_t gro_seg_bytes(uint32_t len, uint32_t seg_len, uint64_t count, uint64_t k) {
    if (count == 1) return len;
    const uint64_t left = len - k * seg_len;
    return left < seg_len ? (uint32_t)left : seg_len;
}

// A buffer that reaches past the packed area or past slot n is skipped whole.
QGCM_GRO_HD inline bool gro_buf_skipped(const qgcm_gro_buf &b, uint64_t count, uint64_t packed_len, uint32_t n) {
    return (uint64_t)b.off + b.len > packed_len || (uint64_t)b.first + count > n;
}

// The buffer of slot i (i < n, n_bufs >= 1): the index of the last buffer whose first is at or below i (0 when
// none is) in a table whose `first` values ascend; on any other table some index below n_bufs.  Every read of
// the table lies below n_bufs.  The search of gro_unpack_kernel and gro_resolve_kernel, and tests/cpp_gro_resolve
// runs it on the host.
QGCM_GRO_HD inline uint32_t gro_find(const qgcm_gro_buf *bufs, uint32_t n_bufs, uint32_t n, uint64_t i) {
    // the last buffer whose first is at or below i, kept in [lo, hi): bufs[lo].first <= i unless lo is 0,
    // bufs[hi].first > i unless hi is n_bufs.  Buffers of equal counts would put slot i into buffer
    // i * n_bufs / n; the bracket is grown from there in doubling steps, then halved.
    uint32_t lo = 0, hi = n_bufs;
    const uint32_t guess = (uint32_t)(i * n_bufs / n);
    if (bufs[guess].first <= i) {
        lo = guess;
        uint32_t step = 1;
        while (hi - lo > step && bufs[lo + step].first <= i) {
            lo += step;
            step <<= 1;
        }
        if (hi - lo > step) hi = lo + step;
    } else {
        hi = guess;
        uint32_t step = 1;
        while (step <= hi && bufs[hi - step].first > i) {
            hi -= step;
            step <<= 1;
        }
        lo = step <= hi ? hi - step : 0;
    }
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bufs[mid].first <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// What the host entry points ask of a table: each `first` the exclusive prefix sum of the counts before it,
// and n datagrams in all.
inline bool gro_table_ok(const qgcm_gro_buf *bufs, uint32_t n_bufs, uint32_t n) {
    uint64_t at = 0;
    for (uint32_t b = 0; b < n_bufs; ++b) {
        if (bufs[b].first != at) return false;
        at += gro_count(bufs[b].len, bufs[b].seg_len);
        if (at > n) return false;
    }
    return at == n;
}

// The unpack by the host: lens[i] and bytes [0, min(L, stride)) of slot i for every datagram of every buffer
// that is not skipped; nothing else is written.
inline void gro_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_gro_buf *bufs, uint32_t n_bufs,
                           uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens) {
    for (uint32_t b = 0; b < n_bufs; ++b) {
        const qgcm_gro_buf &g = bufs[b];
        const uint64_t count = gro_count(g.len, g.seg_len);
        if (gro_buf_skipped(g, count, packed_len, n)) continue;
        for (uint64_t k = 0; k < count; ++k) {
            const uint32_t L = gro_seg_bytes(g.len, g.seg_len, count, k);
            const uint64_t i = g.first + k;
            lens[i] = L;
            if (L) memcpy(arena + i * stride, packed + g.off + k * g.seg_len, (size_t)(L < stride ? L : stride));
        }
    }
}

}  // namespace qgcm
