// pack_core.h -- the delivered-packet pack of include/qgcm.h ("delivered packets packed on routed batches")
// as plain C++: which packet is delivered, the bytes of its record, the record table's check and the host
// pack.  No HIP, no allocation: qgcm_deliver_pack_cpu runs it, pack_kernels.hip shares the two rules with it,
// qgcm_tun_write_packed checks its tables with it, and tests/cpp_pack builds it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_PACK_HD __host__ __device__
#else
#define QGCM_PACK_HD
#endif

namespace qgcm {

constexpr uint32_t kPackNoRoom = 0xffffffffu;             // `off` of a record that did not fit
constexpr uint64_t kPackMaxCap = 0xffffffffull - 15;      // 2^32 - 16: the largest packed_cap (`off` is 32 bits)

// Packet i is delivered when its status is 1 and header and packet fit its slot.  64-bit: a length of
// 0xffffffff must not wrap into a small one.
QGCM_PACK_HD inline bool pack_delivered(uint32_t status, uint32_t len, uint64_t stride) {
    return status == 1 && (uint64_t)4 + len <= stride;
}

// Bytes of a record: the 4-byte header and the packet, rounded up to 16.
QGCM_PACK_HD inline uint64_t pack_rec_bytes(uint32_t len) { return ((uint64_t)4 + len + 15) & ~(uint64_t)15; }

// What qgcm_tun_write_packed asks of a table: every record inside the packed area.
inline bool pack_table_ok(const qgcm_pack_rec *recs, uint32_t m, uint64_t packed_len) {
    for (uint32_t k = 0; k < m; ++k)
        if ((uint64_t)recs[k].off + 4 + recs[k].len > packed_len) return false;
    return true;
}

// The pack by the host: the records that fit below packed_cap (zero padding included), recs[0..m), counts =
// {m, the sum of all record sizes}; nothing else is written.
inline void deliver_pack_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                             const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_pack_rec *recs,
                             uint64_t counts[2]) {
    uint64_t m = 0, bytes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t L = lens[i];
        if (!pack_delivered(status ? status[i] : 1u, L, stride)) continue;
        const uint64_t R = pack_rec_bytes(L);
        const bool fits = bytes + R <= packed_cap;
        recs[m++] = qgcm_pack_rec{fits ? (uint32_t)bytes : kPackNoRoom, L, i, peer[i]};
        if (fits) {
            memcpy(packed + bytes, arena + (uint64_t)i * stride, (size_t)4 + L);
            memset(packed + bytes + 4 + L, 0, (size_t)(R - 4 - L));
        }
        bytes += R;
    }
    counts[0] = m;
    counts[1] = bytes;
}

}  // namespace qgcm
