// dtls_host.cpp -- the host forms of the DTLS record layer's two ordered rules (include/qgcm.h "DTLS 1.2 records
// on routed batches"): qgcm_dtls_number_cpu, the seal's checks, numbering and header entries, and
// qgcm_dtls_replay_cpu, the anti-replay window over (session, seq, authentic), packet by packet or in the
// parallel form the kernels of dtls_kernels.hip evaluate.  Both are dtls_core.h's rules; no crypto here.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/qgcm.h"
#include "dtls_core.h"

using namespace qgcm;

extern "C" {

int qgcm_dtls_number_cpu(const qgcm_dtls_keys *keys, const uint8_t *set, uint64_t *write_seq, uint32_t n_sessions,
                         uint64_t stride, uint32_t n, uint32_t *lens, const uint32_t *peer, qgcm_dtls_hdr *hdr,
                         uint8_t *status, uint8_t *reason) {
    if ((n_sessions && (!keys || !write_seq)) || (n && (!lens || !peer || !hdr || !status))) return QGCM_E_ARG;
    if ((stride & 3) || stride < 20) return QGCM_E_ARG;
    for (uint32_t p = 0; p < n_sessions; ++p)
        if (write_seq[p] > kDtlsSeqEnd) return QGCM_E_ARG;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t p = peer[i];
        uint32_t why = QGCM_DTLS_OK;
        if (p >= n_sessions || (set && !set[p]))
            why = QGCM_DTLS_NO_SESSION;
        else
            why = dtls_seal_check(lens[i], stride);
        if (why == QGCM_DTLS_OK) {
            const uint64_t seq = write_seq[p];
            if (seq < kDtlsSeqEnd) {
                ++write_seq[p];
                dtls_write_hdr(hdr[i].b, keys[p].write_epoch, seq, lens[i]);
                lens[i] += kDtlsTag;
            } else {
                why = QGCM_DTLS_SEQ_EXHAUSTED;
            }
        }
        status[i] = why == QGCM_DTLS_OK ? 1 : 0;
        if (reason) reason[i] = (uint8_t)why;
    }
    return QGCM_OK;
}

int qgcm_dtls_replay_cpu(uint32_t n, const uint32_t *session, const uint64_t *seq, const uint8_t *authentic,
                         uint32_t n_sessions, uint64_t *state, uint8_t *accept, int parallel) {
    if ((n && (!session || !seq || !authentic || !accept)) || (n_sessions && !state)) return QGCM_E_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (authentic[i] && session[i] < n_sessions && seq[i] >= kDtlsSeqEnd) return QGCM_E_ARG;
    auto counts = [&](uint32_t i) { return authentic[i] != 0 && session[i] < n_sessions; };
    if (!parallel) {
        for (uint32_t i = 0; i < n; ++i) {
            accept[i] = 0;
            if (!counts(i)) continue;
            uint64_t &R = state[2ull * session[i]], &W = state[2ull * session[i] + 1];
            accept[i] = dtls_window_step(R, W, seq[i]) ? 1 : 0;
        }
        return QGCM_OK;
    }
    // The parallel form, in the kernels' steps: the counting packets by (session, arena order) for the running
    // maximum, by (session, seq, arena order) for the duplicate test, then the closed-form end state.
    std::vector<uint32_t> a;
    for (uint32_t i = 0; i < n; ++i) {
        accept[i] = 0;
        if (counts(i)) a.push_back(i);
    }
    std::stable_sort(a.begin(), a.end(), [&](uint32_t x, uint32_t y) { return session[x] < session[y]; });
    std::vector<uint32_t> b = a;
    std::stable_sort(b.begin(), b.end(), [&](uint32_t x, uint32_t y) {
        return session[x] != session[y] ? session[x] < session[y] : seq[x] < seq[y];
    });
    std::vector<uint8_t> dup(n, 0);
    for (size_t j = 1; j < b.size(); ++j)
        if (session[b[j]] == session[b[j - 1]] && seq[b[j]] == seq[b[j - 1]]) dup[b[j]] = 1;
    for (size_t j = 0; j < a.size();) {
        const uint32_t p = session[a[j]];
        const uint64_t R0 = state[2ull * p], W0 = state[2ull * p + 1];
        uint64_t M = R0;
        size_t e = j;
        for (; e < a.size() && session[a[e]] == p; ++e) {
            const uint32_t i = a[e];
            accept[i] = dtls_window_accept(R0, W0, M, seq[i], dup[i] != 0) ? 1 : 0;
            M = std::max(M, seq[i]);
        }
        uint64_t W1 = dtls_window_carry(R0, W0, M);
        for (size_t k = j; k < e; ++k) W1 |= dtls_window_bit(M, seq[a[k]]);
        state[2ull * p] = M;
        state[2ull * p + 1] = W1;
        j = e;
    }
    return QGCM_OK;
}

}  // extern "C"
