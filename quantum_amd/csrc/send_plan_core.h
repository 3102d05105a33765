// send_plan_core.h -- the send plan of include/qgcm.h ("send plan on routed batches") as plain C++: the
// limits' defaults and bounds, cap(L), and the host planner.  No HIP, no allocation: qgcm_send_plan_cpu and
// the small-batch path of qgcm_send_plan_host run it, plan_kernels.hip shares the limits and cap(L) with it,
// and tests/cpp_plan builds it under the host sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_PLAN_HD __host__ __device__
#else
#define QGCM_PLAN_HD
#endif

namespace qgcm {

constexpr uint32_t kPlanMaxSegs = 64;       // UDP_MAX_SEGMENTS of the oldest kernels with UDP_SEGMENT
constexpr uint32_t kPlanMaxBytes = 65507;   // the largest UDP payload over IPv4
constexpr uint32_t kPlanSegsBound = 1024;   // UIO_MAXIOV: a train is one iovec per datagram

// A zero field takes its default; false when a field is out of bounds (QGCM_E_ARG).
inline bool plan_limits_resolve(const qgcm_plan_limits *in, qgcm_plan_limits *out) {
    qgcm_plan_limits l = in ? *in : qgcm_plan_limits{0, 0, 0};
    if (l.max_segs == 0) l.max_segs = kPlanMaxSegs;
    if (l.max_seg_len == 0) l.max_seg_len = kPlanMaxBytes;
    if (l.max_bytes == 0) l.max_bytes = kPlanMaxBytes;
    if (l.max_segs > kPlanSegsBound || l.max_bytes > kPlanMaxBytes) return false;
    *out = l;
    return true;
}

// Packets of length len (nonzero) that one train may hold.
QGCM_PLAN_HD inline uint32_t plan_cap(uint32_t len, uint32_t max_segs, uint32_t max_seg_len, uint32_t max_bytes) {
    if (len > max_seg_len) return 1u;
    const uint32_t by_bytes = max_bytes / len;
    const uint32_t c = by_bytes < max_segs ? by_bytes : max_segs;
    return c ? c : 1u;
}

// The host planner.  `lim` is resolved (plan_limits_resolve).  order: n entries, trains: n entries; the
// trains' storage doubles as the sort's second buffer, so nothing is allocated.  The sendable indices are
// sorted by peer with one stable counting sort per 8-bit digit of the peer (1 pass up to 256 key slots, 2 up
// to 65536, 3 beyond), least significant digit first, so arena order survives within a peer; one pass over
// the result cuts the trains.
inline void send_plan_cpu(uint32_t n, const uint32_t *lens, const uint32_t *peer, uint32_t max_keys,
                          const qgcm_plan_limits &lim, uint32_t *order, qgcm_train *trains, uint32_t counts[2]) {
    uint32_t passes = 1;
    while (passes < 4 && ((uint64_t)1 << (8 * passes)) < max_keys) ++passes;
    uint32_t *tmp = reinterpret_cast<uint32_t *>(trains);
    // the last pass must land in `order`
    uint32_t *dst = (passes & 1) ? order : tmp, *src = nullptr;
    uint32_t m = 0;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t shift = 8 * pass;
        uint32_t start[256] = {};
        if (pass == 0) {
            for (uint32_t i = 0; i < n; ++i)
                if (peer[i] < max_keys && lens[i] != 0) ++start[peer[i] & 255u];
        } else {
            for (uint32_t j = 0; j < m; ++j) ++start[(peer[src[j]] >> shift) & 255u];
        }
        uint32_t run = 0;
        for (uint32_t d = 0; d < 256; ++d) {
            const uint32_t c = start[d];
            start[d] = run;
            run += c;
        }
        if (pass == 0) {
            m = run;
            for (uint32_t i = 0; i < n; ++i)
                if (peer[i] < max_keys && lens[i] != 0) dst[start[peer[i] & 255u]++] = i;
        } else {
            for (uint32_t j = 0; j < m; ++j) dst[start[(peer[src[j]] >> shift) & 255u]++] = src[j];
        }
        src = dst;
        dst = dst == order ? tmp : order;
    }
    // trains: a run of equal (peer, length) is cut from its front every cap(length) packets
    uint32_t t = 0;
    for (uint32_t p = 0; p < m;) {
        const uint32_t pr = peer[order[p]], len = lens[order[p]];
        const uint32_t cap = plan_cap(len, lim.max_segs, lim.max_seg_len, lim.max_bytes);
        uint32_t q = p + 1;
        while (q < m && q - p < cap && peer[order[q]] == pr && lens[order[q]] == len) ++q;
        trains[t++] = qgcm_train{p, q - p, pr, len};
        p = q;
    }
    counts[0] = m;
    counts[1] = t;
}

}  // namespace qgcm
