// dtls_core.h -- the rules of the DTLS 1.2 record layer on routed batches (include/qgcm.h "DTLS 1.2 records on
// routed batches"), once for the host (qgcm_dtls_number_cpu, qgcm_dtls_replay_cpu) and the kernels
// (dtls_kernels.hip, gcm_dtls_kernel): the record header, the per-packet checks of seal and open, and the
// RFC 6347 4.1.2.6 anti-replay window in its packet-by-packet and its parallel form.
#pragma once
#include <stdint.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_HD __host__ __device__ inline
#else
#define QGCM_HD inline
#endif

namespace qgcm {

constexpr uint64_t kDtlsSeqEnd = 1ull << 48;  // sequence numbers are 48 bits; write_seq saturates here
constexpr uint32_t kDtlsTag = 16;
constexpr uint32_t kDtlsWindow = 64;

// One entry of the device session table (64 B).  IVs as the little-endian word of their four bytes: the first
// nonce word of the GCM kernels.
struct DtlsSession {
    uint32_t write_slot, read_slot;
    uint32_t write_iv, read_iv;
    uint32_t write_epoch, read_epoch;
    uint32_t set, pad;
    uint64_t write_seq, R, W, pad2;
};

// record header and explicit nonce of a sealed record: 23 | FE FD | epoch | seq48 | 8 + L + 16 | epoch | seq48,
// then zeros
QGCM_HD void dtls_write_hdr(uint8_t b[32], uint32_t epoch, uint64_t seq, uint32_t L) {
    const uint32_t rec = 8u + L + kDtlsTag;
    b[0] = 23;
    b[1] = 0xfe;
    b[2] = 0xfd;
    b[3] = (uint8_t)(epoch >> 8);
    b[4] = (uint8_t)epoch;
    for (int k = 0; k < 6; ++k) b[5 + k] = (uint8_t)(seq >> (40 - 8 * k));
    b[11] = (uint8_t)(rec >> 8);
    b[12] = (uint8_t)rec;
    for (int k = 0; k < 8; ++k) b[13 + k] = b[3 + k];
    for (int k = 21; k < 32; ++k) b[k] = 0;
}

QGCM_HD uint64_t dtls_hdr_seq(const uint8_t *b) {
    uint64_t s = 0;
    for (int k = 0; k < 6; ++k) s = (s << 8) | b[5 + k];
    return s;
}

// seal step 2
QGCM_HD uint32_t dtls_seal_check(uint32_t L, uint64_t stride) {
    return (L == 0 || L > QGCM_DTLS_MAX_PLAIN || (uint64_t)L + kDtlsTag > stride) ? QGCM_DTLS_MALFORMED : QGCM_DTLS_OK;
}

// open steps 2 and 3: B bytes in the slot under header entry b
QGCM_HD uint32_t dtls_open_check(const uint8_t *b, uint32_t B, uint64_t stride, uint32_t read_epoch) {
    if (b[0] != 23) return QGCM_DTLS_NOT_APPDATA;
    if (b[1] != 0xfe || b[2] != 0xfd) return QGCM_DTLS_MALFORMED;
    if ((((uint32_t)b[3] << 8) | b[4]) != read_epoch) return QGCM_DTLS_MALFORMED;
    if (B < kDtlsTag + 1 || B > QGCM_DTLS_MAX_PLAIN + kDtlsTag || B > stride) return QGCM_DTLS_MALFORMED;
    if ((((uint32_t)b[11] << 8) | b[12]) != 8u + B) return QGCM_DTLS_MALFORMED;
    return QGCM_DTLS_OK;
}

// The window, packet by packet (RFC 6347 4.1.2.6; OpenSSL's bitmap rule): bit k of W means R - k was seen.
QGCM_HD bool dtls_window_step(uint64_t &R, uint64_t &W, uint64_t s) {
    if (s > R) {
        const uint64_t sh = s - R;
        W = sh >= kDtlsWindow ? 1ull : ((W << sh) | 1ull);
        R = s;
        return true;
    }
    const uint64_t d = R - s;
    if (d >= kDtlsWindow || ((W >> d) & 1ull)) return false;
    W |= 1ull << d;
    return true;
}

// The window in parallel form.  M = max(R0, the numbers of the session's earlier authentic packets), dup = an
// earlier authentic packet of the session carries the same number.
QGCM_HD bool dtls_window_accept(uint64_t R0, uint64_t W0, uint64_t M, uint64_t s, bool dup) {
    if (s > M) return true;
    if (M - s >= kDtlsWindow || dup) return false;
    if (s <= R0 && R0 - s < kDtlsWindow && ((W0 >> (R0 - s)) & 1ull)) return false;  // inside the old window
    return true;
}
// End state: R1 = max(R0, every authentic s), W1 = dtls_window_carry(R0, W0, R1) | dtls_window_bit(R1, s) of
// every authentic s.
QGCM_HD uint64_t dtls_window_carry(uint64_t R0, uint64_t W0, uint64_t R1) {
    const uint64_t sh = R1 - R0;
    return sh >= kDtlsWindow ? 0ull : W0 << sh;
}
QGCM_HD uint64_t dtls_window_bit(uint64_t R1, uint64_t s) {
    return R1 - s < kDtlsWindow ? 1ull << (R1 - s) : 0ull;
}

}  // namespace qgcm
