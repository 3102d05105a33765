// dtls_kernels.hip -- the ordered, per-session steps of the DTLS record layer on routed batches (include/qgcm.h
// "DTLS 1.2 records on routed batches"; the rules are dtls_core.h's): sequence numbers handed out in arena order
// on the way out, the RFC 6347 4.1.2.6 anti-replay window on the way in.  The GCM work between them is
// gcm_dtls_kernel (gcm_kernels.hip) over the descriptors written here.
//
// Seal (launch_dtls_seal_number, before the GCM launch):
//   dtls_seal_keys_kernel     steps 1-2; key = sealable ? session : max_keys, val = i      one lane per packet
//   radix sort                (key, val), stable, over the bits of max_keys                 as plan_kernels.hip
//   dtls_first_kernel         first[session] = where its run starts in the sorted order    one lane per position
//   dtls_seal_number_kernel   seq = write_seq + (position - first): header entry, length,  one lane per position
//                             descriptor -- or SEQ_EXHAUSTED
//   dtls_seal_advance_kernel  the run's last position advances write_seq (a launch of its own: the kernel
//                             before reads write_seq at every position)
// Open, before the GCM launch (launch_dtls_open_prep):
//   dtls_open_prep_kernel     steps 1-3; open descriptors of what passes                    one lane per packet
// Open, after it (launch_dtls_open_replay), over the packets the GCM kernel found authentic:
//   dtls_replay_keys_kernel   AUTH for the others; key = authentic ? session : max_keys, the 48-bit number
//   radix sort A              (session, i): the sessions' packets in arena order
//   radix sorts B1, B2        by number, then stably by session: (session, seq, i) order; a position whose
//   dtls_dup_kernel           predecessor has its session and number is a duplicate of an earlier packet
//   dtls_max_tile_kernel      over order A, the segmented running maximum of the numbers: reduce-then-scan in
//   dtls_max_spine_kernel     three launches (tile summaries, their exclusive prefix in one workgroup, the tile's
//   dtls_replay_emit_kernel   scan again under its prefix); then dtls_window_accept per packet with M = max(R0,
//                             the maximum before it), status, reason, length, and R1 of the session at its run's end
//   dtls_window_carry_kernel  W <- W0 shifted to R1 (run heads; a launch of its own: the emit kernel reads W0)
//   dtls_window_bits_kernel   W |= the bit of every authentic number inside the new window (an atomic OR: the
//                             result does not depend on the order), R <- R1
// No workgroup waits for another, and nothing depends on scheduling.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdint.h>

#include "dtls_core.h"
#include "gcm_internal.h"

namespace qgcm {

constexpr uint32_t kDtlsTile = 256;  // positions per workgroup, one per lane
constexpr uint32_t kDtlsSpineThreads = 1024;
constexpr uint32_t kDtlsNoKey = 0xffffffffu;  // descriptor key of a packet the GCM launch must leave alone

__device__ inline bool dtls_session_ok(const DtlsCall &c, uint32_t p, bool seal) {
    if (p >= c.max_keys) return false;
    const DtlsSession &s = c.sessions[p];
    if (!s.set) return false;
    const uint32_t slot = seal ? s.write_slot : s.read_slot;
    return slot < c.max_keys && c.key_valid[slot] != 0;
}

__device__ inline void dtls_reject(const DtlsCall &c, uint32_t i, uint32_t why) {
    c.descs[i] = qgcm_desc{0, 0, kDtlsNoKey};
    c.status[i] = 0;
    if (c.reason) c.reason[i] = (uint8_t)why;
}

__global__ void __launch_bounds__(kDtlsTile) dtls_seal_keys_kernel(DtlsCall c, uint32_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * kDtlsTile + threadIdx.x;
    if (i >= c.n) return;
    uint32_t why = QGCM_DTLS_OK;
    const uint32_t p = c.peer[i];
    if (!dtls_session_ok(c, p, true))
        why = QGCM_DTLS_NO_SESSION;
    else
        why = dtls_seal_check(c.lens[i], c.stride);
    if (why != QGCM_DTLS_OK) dtls_reject(c, i, why);
    keys[i] = why == QGCM_DTLS_OK ? p : c.max_keys;
    vals[i] = i;
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_first_kernel(const uint32_t *keys, uint32_t n, uint32_t max_keys, uint32_t *first) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = keys[j];
    if (k < max_keys && (j == 0 || keys[j - 1] != k)) first[k] = j;
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_seal_number_kernel(DtlsCall c, const uint32_t *keys, const uint32_t *order, const uint32_t *first) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j >= c.n) return;
    const uint32_t k = keys[j];
    if (k >= c.max_keys) return;
    const uint32_t i = order[j];
    const DtlsSession &s = c.sessions[k];
    const uint64_t seq = s.write_seq + (j - first[k]);
    if (seq >= kDtlsSeqEnd) {
        dtls_reject(c, i, QGCM_DTLS_SEQ_EXHAUSTED);
        return;
    }
    const uint32_t L = c.lens[i];
    uint8_t b[32];
    dtls_write_hdr(b, s.write_epoch, seq, L);
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        w[q] = (uint32_t)b[4 * q] | ((uint32_t)b[4 * q + 1] << 8) | ((uint32_t)b[4 * q + 2] << 16) |
               ((uint32_t)b[4 * q + 3] << 24);
    uint4 *dst = reinterpret_cast<uint4 *>(c.hdr + i);
    dst[0] = uint4{w[0], w[1], w[2], w[3]};
    dst[1] = uint4{w[4], w[5], w[6], w[7]};
    c.descs[i] = qgcm_desc{(uint64_t)i * c.stride, L, s.write_slot};
    c.lens[i] = L + kDtlsTag;
    c.status[i] = 0;  // the GCM kernel sets it once the record is sealed
    if (c.reason) c.reason[i] = QGCM_DTLS_OK;
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_seal_advance_kernel(DtlsCall c, const uint32_t *keys, const uint32_t *first) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j >= c.n) return;
    const uint32_t k = keys[j];
    if (k >= c.max_keys || (j + 1 < c.n && keys[j + 1] == k)) return;
    DtlsSession &s = c.sessions[k];
    const uint64_t next = s.write_seq + (uint64_t)(j + 1 - first[k]);
    s.write_seq = next < kDtlsSeqEnd ? next : kDtlsSeqEnd;
}

__global__ void __launch_bounds__(kDtlsTile) dtls_open_prep_kernel(DtlsCall c) {
    const uint32_t i = blockIdx.x * kDtlsTile + threadIdx.x;
    if (i >= c.n) return;
    const uint32_t p = c.peer[i];
    if (!dtls_session_ok(c, p, false)) {
        dtls_reject(c, i, QGCM_DTLS_NO_SESSION);
        return;
    }
    const DtlsSession &s = c.sessions[p];
    const uint32_t B = c.lens[i];
    const uint4 *src = reinterpret_cast<const uint4 *>(c.hdr + i);
    const uint4 h = src[0];
    const uint32_t w[4] = {h.x, h.y, h.z, h.w};
    uint8_t b[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) b[q] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
    const uint32_t why = dtls_open_check(b, B, c.stride, s.read_epoch);
    if (why != QGCM_DTLS_OK) {
        dtls_reject(c, i, why);
        return;
    }
    // the batch kernels' open descriptor: the record's bytes plus QGCM_OVERHEAD, here B - 16 of payload
    c.descs[i] = qgcm_desc{(uint64_t)i * c.stride, B - kDtlsTag + (uint32_t)QGCM_OVERHEAD, s.read_slot};
    c.status[i] = 0;
    if (c.reason) c.reason[i] = QGCM_DTLS_OK;
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_replay_keys_kernel(DtlsCall c, uint32_t *keys, uint32_t *vals, uint64_t *seq, uint8_t *dup) {
    const uint32_t i = blockIdx.x * kDtlsTile + threadIdx.x;
    if (i >= c.n) return;
    const bool tried = c.descs[i].key_idx != kDtlsNoKey;
    const bool auth = tried && c.status[i] == 1;
    if (tried && !auth && c.reason) c.reason[i] = QGCM_DTLS_AUTH;
    uint64_t s = ~0ull;
    if (auth) {
        const uint4 *src = reinterpret_cast<const uint4 *>(c.hdr + i);
        const uint4 h = src[0];
        // b[5:11], big endian: b[5..7] in the second word, b[8..10] in the third
        s = ((uint64_t)((h.y >> 8) & 0xff) << 40) | ((uint64_t)((h.y >> 16) & 0xff) << 32) |
            ((uint64_t)(h.y >> 24) << 24) | ((uint64_t)(h.z & 0xff) << 16) | ((uint64_t)((h.z >> 8) & 0xff) << 8) |
            (uint64_t)((h.z >> 16) & 0xff);
    }
    keys[i] = auth ? c.peer[i] : c.max_keys;
    vals[i] = i;
    seq[i] = s;
    dup[i] = 0;
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_gather_kernel(const uint32_t *keys, const uint32_t *order, uint32_t n, uint32_t *out) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j < n) out[j] = keys[order[j]];
}

// order: (session, seq, i) ascending.  Position j repeats an earlier authentic packet of its session when its
// predecessor has the same session and number.
__global__ void __launch_bounds__(kDtlsTile)
dtls_dup_kernel(const uint32_t *keys, const uint32_t *order, const uint64_t *seq, uint32_t n, uint32_t max_keys,
                uint8_t *dup) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j >= n || j == 0) return;
    const uint32_t k = keys[j];
    if (k >= max_keys || keys[j - 1] != k) return;
    if (seq[order[j - 1]] == seq[order[j]]) dup[order[j]] = 1;
}

// The running maximum since the last run head: {head seen, maximum}.
struct DtlsMax {
    uint32_t head;
    uint64_t max;
};
__device__ inline DtlsMax dtls_max_combine(const DtlsMax &l, const DtlsMax &r) {
    if (r.head) return r;
    return DtlsMax{l.head, l.max > r.max ? l.max : r.max};
}

struct DtlsItem {
    uint32_t key, i;
    uint64_t s;
    bool valid, head;
};
__device__ inline DtlsItem dtls_item(uint32_t j, uint32_t n, uint32_t max_keys, const uint32_t *keys,
                                     const uint32_t *order, const uint64_t *seq) {
    DtlsItem it{max_keys, 0u, 0ull, false, false};
    if (j < n) {
        it.key = keys[j];
        it.valid = it.key < max_keys;
        if (it.valid) {
            it.i = order[j];
            it.s = seq[it.i];
            it.head = j == 0 || keys[j - 1] != it.key;
        }
    }
    return it;
}

// inclusive scan of one summary per lane over the workgroup's kDtlsTile lanes
__device__ inline DtlsMax dtls_tile_scan(DtlsMax v, uint32_t *sh, uint64_t *sm) {
    const uint32_t t = threadIdx.x;
    for (uint32_t d = 1; d < kDtlsTile; d <<= 1) {
        sh[t] = v.head;
        sm[t] = v.max;
        __syncthreads();
        if (t >= d) v = dtls_max_combine(DtlsMax{sh[t - d], sm[t - d]}, v);
        __syncthreads();
    }
    return v;
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_max_tile_kernel(const uint32_t *keys, const uint32_t *order, const uint64_t *seq, uint32_t n, uint32_t max_keys,
                     uint32_t *tile_head, uint64_t *tile_max) {
    __shared__ uint32_t sh[kDtlsTile];
    __shared__ uint64_t sm[kDtlsTile];
    const DtlsItem it = dtls_item(blockIdx.x * kDtlsTile + threadIdx.x, n, max_keys, keys, order, seq);
    const DtlsMax v = dtls_tile_scan(DtlsMax{it.head ? 1u : 0u, it.s}, sh, sm);
    if (threadIdx.x == kDtlsTile - 1) {
        tile_head[blockIdx.x] = v.head;
        tile_max[blockIdx.x] = v.max;
    }
}

// tile k <- the summary of tiles [0, k).  One workgroup: each lane folds a stretch of consecutive tiles, the
// stretches' sums are scanned in LDS, and each lane walks its stretch again (plan_spine_kernel's shape).
__global__ void __launch_bounds__(kDtlsSpineThreads)
dtls_max_spine_kernel(uint32_t *tile_head, uint64_t *tile_max, uint32_t ntiles) {
    __shared__ uint32_t sh[kDtlsSpineThreads];
    __shared__ uint64_t sm[kDtlsSpineThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kDtlsSpineThreads - 1) / kDtlsSpineThreads;
    const uint32_t lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    DtlsMax v{0u, 0ull};
    for (uint32_t k = lo; k < hi; ++k) v = dtls_max_combine(v, DtlsMax{tile_head[k], tile_max[k]});
    for (uint32_t d = 1; d < kDtlsSpineThreads; d <<= 1) {
        sh[t] = v.head;
        sm[t] = v.max;
        __syncthreads();
        if (t >= d) v = dtls_max_combine(DtlsMax{sh[t - d], sm[t - d]}, v);
        __syncthreads();
    }
    sh[t] = v.head;
    sm[t] = v.max;
    __syncthreads();
    DtlsMax run = t ? DtlsMax{sh[t - 1], sm[t - 1]} : DtlsMax{0u, 0ull};
    for (uint32_t k = lo; k < hi; ++k) {
        const DtlsMax x{tile_head[k], tile_max[k]};
        tile_head[k] = run.head;
        tile_max[k] = run.max;
        run = dtls_max_combine(run, x);
    }
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_replay_emit_kernel(DtlsCall c, const uint32_t *keys, const uint32_t *order, const uint64_t *seq,
                        const uint8_t *dup, const uint32_t *tile_head, const uint64_t *tile_max, uint64_t *r_new) {
    __shared__ uint32_t sh[kDtlsTile];
    __shared__ uint64_t sm[kDtlsTile];
    const uint32_t t = threadIdx.x;
    const uint32_t j = blockIdx.x * kDtlsTile + t;
    const DtlsItem it = dtls_item(j, c.n, c.max_keys, keys, order, seq);
    const DtlsMax v = dtls_tile_scan(DtlsMax{it.head ? 1u : 0u, it.s}, sh, sm);
    sh[t] = v.head;
    sm[t] = v.max;
    __syncthreads();
    if (!it.valid) return;
    const DtlsMax carry{tile_head[blockIdx.x], tile_max[blockIdx.x]};
    const DtlsSession &s = c.sessions[it.key];
    const uint64_t R0 = s.R, W0 = s.W;
    uint64_t M = R0;
    if (!it.head) {  // the maximum of the run's earlier numbers: the run head lies before j
        const DtlsMax before = t ? dtls_max_combine(carry, DtlsMax{sh[t - 1], sm[t - 1]}) : carry;
        if (before.max > M) M = before.max;
    }
    const bool ok = dtls_window_accept(R0, W0, M, it.s, dup[it.i] != 0);
    c.status[it.i] = ok ? 1 : 0;
    if (c.reason) c.reason[it.i] = ok ? QGCM_DTLS_OK : QGCM_DTLS_REPLAY;
    if (ok) c.lens[it.i] -= kDtlsTag;
    if (j + 1 == c.n || keys[j + 1] != it.key) {
        const DtlsMax all = dtls_max_combine(carry, v);
        r_new[it.key] = all.max > R0 ? all.max : R0;
    }
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_window_carry_kernel(DtlsCall c, const uint32_t *keys, const uint64_t *r_new) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j >= c.n) return;
    const uint32_t k = keys[j];
    if (k >= c.max_keys || (j != 0 && keys[j - 1] == k)) return;
    DtlsSession &s = c.sessions[k];
    s.W = dtls_window_carry(s.R, s.W, r_new[k]);
}

__global__ void __launch_bounds__(kDtlsTile)
dtls_window_bits_kernel(DtlsCall c, const uint32_t *keys, const uint32_t *order, const uint64_t *seq,
                        const uint64_t *r_new) {
    const uint32_t j = blockIdx.x * kDtlsTile + threadIdx.x;
    if (j >= c.n) return;
    const uint32_t k = keys[j];
    if (k >= c.max_keys) return;
    DtlsSession &s = c.sessions[k];
    const uint64_t R1 = r_new[k];
    const uint64_t bit = dtls_window_bit(R1, seq[order[j]]);
    if (bit) atomicOr(reinterpret_cast<unsigned long long *>(&s.W), (unsigned long long)bit);
    if (j + 1 == c.n || keys[j + 1] != k) s.R = R1;
}

// Onesweep for every size, as worklist.hip's sort (its comment says why not the merge-sort path)
using DtlsSortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                  rocprim::default_config, 0>;

static hipError_t sort32(void *tmp, size_t &bytes, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in,
                         uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs<DtlsSortConfig>(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, end_bit, s);
}
static hipError_t sort64(void *tmp, size_t &bytes, const uint64_t *k_in, uint64_t *k_out, const uint32_t *v_in,
                         uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs<DtlsSortConfig>(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, end_bit, s);
}

namespace {

inline uint64_t al256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline uint32_t dtls_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kDtlsTile - 1) / kDtlsTile); }

// The work area, in 256-B aligned pieces (the send plan's convention): the descriptors, then the sorts' arrays.
struct DtlsWork {
    uint32_t *k_in, *v_in, *k_out, *order, *o1, *k2_in, *k2_out, *o2, *first, *tile_head;
    uint64_t *seq, *seq_out, *tile_max, *r_new;
    uint8_t *dup;
    void *sort;
    size_t sort_bytes;
};

uint64_t dtls_fixed_bytes(uint32_t n, uint32_t max_keys) {
    const uint32_t nt = dtls_tiles(n);
    return al256(16ull * n) + 8 * al256(4ull * n) + 2 * al256(8ull * n) + al256(n) + al256(4ull * max_keys) +
           al256(8ull * max_keys) + al256(4ull * nt) + al256(8ull * nt);
}

bool dtls_carve(const DtlsCall &c, DtlsWork &w, qgcm_desc *&descs) {
    const uint64_t fixed = dtls_fixed_bytes(c.n, c.max_keys);
    if (c.work_bytes < fixed) return false;
    const uint32_t nt = dtls_tiles(c.n);
    char *p = static_cast<char *>(c.work);
    descs = (qgcm_desc *)p;    p += al256(16ull * c.n);
    w.k_in = (uint32_t *)p;    p += al256(4ull * c.n);
    w.v_in = (uint32_t *)p;    p += al256(4ull * c.n);
    w.k_out = (uint32_t *)p;   p += al256(4ull * c.n);
    w.order = (uint32_t *)p;   p += al256(4ull * c.n);
    w.o1 = (uint32_t *)p;      p += al256(4ull * c.n);
    w.k2_in = (uint32_t *)p;   p += al256(4ull * c.n);
    w.k2_out = (uint32_t *)p;  p += al256(4ull * c.n);
    w.o2 = (uint32_t *)p;      p += al256(4ull * c.n);
    w.seq = (uint64_t *)p;     p += al256(8ull * c.n);
    w.seq_out = (uint64_t *)p; p += al256(8ull * c.n);
    w.dup = (uint8_t *)p;      p += al256(c.n);
    w.first = (uint32_t *)p;   p += al256(4ull * c.max_keys);
    w.r_new = (uint64_t *)p;   p += al256(8ull * c.max_keys);
    w.tile_head = (uint32_t *)p; p += al256(4ull * nt);
    w.tile_max = (uint64_t *)p;  p += al256(8ull * nt);
    w.sort = p;
    w.sort_bytes = (size_t)(c.work_bytes - fixed);  // what is left of the area is the sorts'
    return true;
}

int key_bits(uint32_t max_keys) {  // keys are at most max_keys: the bits of that value
    int end_bit = 1;
    while (end_bit < 32 && (1ull << end_bit) <= max_keys) ++end_bit;
    return end_bit;
}

}  // namespace

// The sorts' area is asked for all key bits, so the size is a function of n and max_keys alone (rocprim takes an
// area larger than a sort of fewer bits needs).
uint64_t dtls_work_bytes(uint32_t n, uint32_t max_keys) {
    size_t a = 0, b = 0;
    if (n && sort32(nullptr, a, nullptr, nullptr, nullptr, nullptr, n, 32, 0) != hipSuccess) a = 0;
    if (n && sort64(nullptr, b, nullptr, nullptr, nullptr, nullptr, n, 48, 0) != hipSuccess) b = 0;
    return dtls_fixed_bytes(n, max_keys) + al256(a > b ? a : b);
}

qgcm_desc *dtls_work_descs(const DtlsCall &c) { return static_cast<qgcm_desc *>(c.work); }

hipError_t launch_dtls_seal_number(const DtlsCall &call, hipStream_t s) {
    if (call.n == 0) return hipSuccess;
    DtlsCall c = call;
    DtlsWork w;
    if (!dtls_carve(c, w, c.descs)) return hipErrorInvalidValue;
    const dim3 g(dtls_tiles(c.n)), bs(kDtlsTile);
    hipError_t e;
    hipLaunchKernelGGL(dtls_seal_keys_kernel, g, bs, 0, s, c, w.k_in, w.v_in);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t sb = w.sort_bytes;
    if ((e = sort32(w.sort, sb, w.k_in, w.k_out, w.v_in, w.order, c.n, key_bits(c.max_keys), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(dtls_first_kernel, g, bs, 0, s, w.k_out, c.n, c.max_keys, w.first);
    hipLaunchKernelGGL(dtls_seal_number_kernel, g, bs, 0, s, c, w.k_out, w.order, w.first);
    hipLaunchKernelGGL(dtls_seal_advance_kernel, g, bs, 0, s, c, w.k_out, w.first);
    return hipGetLastError();
}

hipError_t launch_dtls_open_prep(const DtlsCall &call, hipStream_t s) {
    if (call.n == 0) return hipSuccess;
    DtlsCall c = call;
    DtlsWork w;
    if (!dtls_carve(c, w, c.descs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtls_open_prep_kernel, dim3(dtls_tiles(c.n)), dim3(kDtlsTile), 0, s, c);
    return hipGetLastError();
}

hipError_t launch_dtls_open_replay(const DtlsCall &call, hipStream_t s) {
    if (call.n == 0) return hipSuccess;
    DtlsCall c = call;
    DtlsWork w;
    if (!dtls_carve(c, w, c.descs)) return hipErrorInvalidValue;
    const uint32_t nt = dtls_tiles(c.n);
    const dim3 g(nt), bs(kDtlsTile);
    const int kb = key_bits(c.max_keys);
    hipError_t e;
    hipLaunchKernelGGL(dtls_replay_keys_kernel, g, bs, 0, s, c, w.k_in, w.v_in, w.seq, w.dup);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t sb = w.sort_bytes;
    if ((e = sort32(w.sort, sb, w.k_in, w.k_out, w.v_in, w.order, c.n, kb, s)) != hipSuccess) return e;
    sb = w.sort_bytes;
    if ((e = sort64(w.sort, sb, w.seq, w.seq_out, w.v_in, w.o1, c.n, 48, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(dtls_gather_kernel, g, bs, 0, s, w.k_in, w.o1, c.n, w.k2_in);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    sb = w.sort_bytes;
    if ((e = sort32(w.sort, sb, w.k2_in, w.k2_out, w.o1, w.o2, c.n, kb, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(dtls_dup_kernel, g, bs, 0, s, w.k2_out, w.o2, w.seq, c.n, c.max_keys, w.dup);
    hipLaunchKernelGGL(dtls_max_tile_kernel, g, bs, 0, s, w.k_out, w.order, w.seq, c.n, c.max_keys, w.tile_head,
                       w.tile_max);
    hipLaunchKernelGGL(dtls_max_spine_kernel, dim3(1), dim3(kDtlsSpineThreads), 0, s, w.tile_head, w.tile_max, nt);
    hipLaunchKernelGGL(dtls_replay_emit_kernel, g, bs, 0, s, c, w.k_out, w.order, w.seq, w.dup, w.tile_head,
                       w.tile_max, w.r_new);
    hipLaunchKernelGGL(dtls_window_carry_kernel, g, bs, 0, s, c, w.k_out, w.r_new);
    hipLaunchKernelGGL(dtls_window_bits_kernel, g, bs, 0, s, c, w.k_out, w.order, w.seq, w.r_new);
    return hipGetLastError();
}

}  // namespace qgcm
