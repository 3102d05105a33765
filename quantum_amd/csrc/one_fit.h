// Size arithmetic of the latency engine's per-packet calls (qgcm_seal_one / qgcm_open_one), shared by
// the launch path (qgcm_api.cpp), the resident path (resident.cpp) and the kernels' own checks
// (gcm_kernels.hip).  Header-only and free of HIP, so a stand-alone host program can sweep it under
// the sanitizers (tools/one_fit_sweep.cpp).
//
// A call's staging area is the record [aad 4][payload][tag 16][nonce 12] rounded up to 16-B rows,
// followed -- only when the additional data is longer than the record's 4 bytes -- by a tail of
// ceil(aad_len / 16) rows that holds it (padding zeroed); the record's first 4 bytes are then zero.
#pragma once
#include <stdint.h>

#include "../../include/qgcm.h"

namespace qgcm {

constexpr uint32_t kOneCap = 32768;        // the LDS staging area of one_packet; record + tail <= kOneCap - 16
constexpr uint32_t kResSlotBytes = 16384;  // request slot of the resident service

// the 16-B-rounded record of a call: len = L on seal (tag and nonce are appended), L + 28 on open
constexpr uint64_t one_record_bytes(uint64_t len, bool seal) {
    return (4ull + len + (seal ? (uint64_t)QGCM_OVERHEAD : 0ull) + 15ull) & ~15ull;
}
// GHASH blocks of the additional data: one (the masked first word of the record, zero without any) up
// to 4 bytes, else ceil(aad_len / 16) (no wrap-around for any 32-bit length)
constexpr uint32_t one_aad_blocks(uint32_t aad_len) {
    return aad_len <= 4u ? 1u : (aad_len >> 4) + ((aad_len & 15u) ? 1u : 0u);
}
// rows of the tail behind the record: none up to 4 bytes
constexpr uint32_t one_tail_rows(uint32_t aad_len) { return aad_len <= 4u ? 0u : one_aad_blocks(aad_len); }
constexpr uint64_t one_tail_bytes(uint32_t aad_len) { return 16ull * one_tail_rows(aad_len); }
// record + tail fit the latency engine's LDS staging area (a gcm_one_kernel launch can serve the call)
constexpr bool one_fits_launch(uint64_t len, bool seal, uint32_t aad_len) {
    return aad_len <= (uint32_t)QGCM_MAX_AAD && len < (uint64_t)QGCM_MAX_PAYLOAD + QGCM_OVERHEAD &&
           one_record_bytes(len, seal) + one_tail_bytes(aad_len) <= kOneCap - 16u;
}
// ... and a resident slot too; `announce`: the slot's last 16 B carry the next seal's nonce, which the
// tail must not reach
constexpr bool one_fits_resident(uint64_t len, bool seal, uint32_t aad_len, bool announce) {
    return one_fits_launch(len, seal, aad_len) &&
           one_record_bytes(len, seal) + one_tail_bytes(aad_len) + (announce ? 16u : 0u) <= kResSlotBytes;
}

}  // namespace qgcm
