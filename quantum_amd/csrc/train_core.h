// train_core.h -- the train pack of include/qgcm.h ("planned trains packed on routed batches") as plain C++:
// which train is void, the bytes of a train, the check of a whole plan, the check of a packed table and the
// host pack.  No HIP, no allocation: qgcm_train_pack_cpu runs it, train_kernels.hip shares the two rules with
// it, qgcm_udp_send_packed checks its tables with it, and tests/cpp_train builds it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_TRAIN_HD __host__ __device__
#else
#define QGCM_TRAIN_HD
#endif

namespace qgcm {

constexpr uint32_t kTrainNoRoom = 0xffffffffu;         // `off` of a train that did not fit, or is void
constexpr uint64_t kTrainMaxCap = 0xffffffffull - 15;  // 2^32 - 16: the largest packed_cap (`off` is 32 bits)
constexpr uint32_t kTrainMaxCount = 1024;              // UIO_MAXIOV, the planner's bound on max_segs

// A train the pack does not touch: a count or a segment length out of range, or members past order's m entries.
// 64-bit: first + count must not wrap.
QGCM_TRAIN_HD inline bool train_void(uint32_t first, uint32_t count, uint32_t seg_len, uint64_t m, uint64_t stride) {
    return count < 1 || count > kTrainMaxCount || seg_len < 1 || seg_len > stride || (uint64_t)first + count > m;
}

// Bytes of a packed train: its datagrams back to back, rounded up to 16.
QGCM_TRAIN_HD inline uint64_t train_bytes(uint32_t count, uint32_t seg_len) {
    return ((uint64_t)count * seg_len + 15) & ~(uint64_t)15;
}

// A well-formed plan: m <= n, t <= m, the trains tile [0, m) in order, none is void, every order[p] < n.
inline bool train_plan_ok(uint64_t stride, uint32_t n, const uint32_t *order, uint32_t m, const qgcm_train *trains,
                          uint32_t t) {
    if (m > n || t > m) return false;
    uint64_t at = 0;
    for (uint32_t j = 0; j < t; ++j) {
        const qgcm_train &tr = trains[j];
        if (tr.first != at || train_void(tr.first, tr.count, tr.seg_len, m, stride)) return false;
        at += tr.count;
    }
    if (at != m) return false;
    for (uint32_t p = 0; p < m; ++p)
        if (order[p] >= n) return false;
    return true;
}

// What qgcm_udp_send_packed asks of a table: every train inside the packed area (one that did not fit, off =
// 0xffffffff, is not), a count the kernel takes as iovecs or segments, a peer with an address, a segment size
// that is nonzero and, where it travels in a control message, fits its 16 bits.
inline bool train_table_ok(const qgcm_ptrain *ptrains, uint32_t n_trains, uint64_t packed_len, uint32_t n_addrs) {
    for (uint32_t j = 0; j < n_trains; ++j) {
        const qgcm_ptrain &tr = ptrains[j];
        if (tr.count < 1 || tr.count > kTrainMaxCount || tr.peer >= n_addrs || tr.seg_len == 0) return false;
        if (tr.count > 1 && tr.seg_len > 65535u) return false;
        if ((uint64_t)tr.off + (uint64_t)tr.count * tr.seg_len > packed_len) return false;
    }
    return true;
}

// The pack by the host, of a plan train_plan_ok has passed: the trains that fit below packed_cap (zero padding
// included), ptrains[0..t), pcounts = {t, the sum of all train sizes}; nothing else is written.
inline void train_pack_cpu(const uint8_t *arena, uint64_t stride, const uint32_t *order, const qgcm_train *trains,
                           uint32_t t, uint8_t *packed, uint64_t packed_cap, qgcm_ptrain *ptrains, uint64_t pcounts[2]) {
    uint64_t bytes = 0;
    for (uint32_t j = 0; j < t; ++j) {
        const qgcm_train &tr = trains[j];
        const uint64_t R = train_bytes(tr.count, tr.seg_len), used = (uint64_t)tr.count * tr.seg_len;
        const bool fits = bytes + R <= packed_cap;
        ptrains[j] = qgcm_ptrain{fits ? (uint32_t)bytes : kTrainNoRoom, tr.count, tr.peer, tr.seg_len};
        if (fits) {
            for (uint32_t k = 0; k < tr.count; ++k)
                memcpy(packed + bytes + (uint64_t)k * tr.seg_len, arena + (uint64_t)order[tr.first + k] * stride, tr.seg_len);
            memset(packed + bytes + used, 0, (size_t)(R - used));
        }
        bytes += R;
    }
    pcounts[0] = t;
    pcounts[1] = bytes;
}

}  // namespace qgcm
