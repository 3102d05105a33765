// plan_kernels.hip -- the send plan of a routed batch on the GPU (include/qgcm.h "send plan on routed
// batches"): the sendable packets grouped by peer in arena order, and each stretch of equal
// (peer, length) cut into trains that one UDP_SEGMENT message can carry.
//
//   plan_keys_kernel    key = sendable ? peer : max_keys, val = i            one lane per packet
//   radix sort          (key, val) pairs, stable, over the bits of max_keys   rocprim Onesweep, as worklist.hip
//                       (the sorted values land in `order` directly)
//   plan_tile_kernel    each 256-position tile's summary                      one lane per position
//   plan_spine_kernel   exclusive prefix of the tile summaries, in place      one workgroup
//   plan_emit_kernel    the tile's scan again under its prefix, then the      one lane per position
//                       trains and the two counts
//
// No atomics, no counter to zero, no workgroup waits for another: the scan is reduce-then-scan over three
// launches, so calls on several streams share nothing but read-only inputs.
//
// The scan.  Position p < m of the sorted order is a run head when p == 0 or its (key, length) differs from
// p - 1's.  A train's index needs the run head before p (a max-scan) and the trains of all earlier runs (a
// sum-scan whose terms depend on the first scan).  Both are one scan over interval summaries
//   {first, last: the first and last run head inside the interval (first == kNone: none),
//    cap: cap(length) of the run that `last` starts,
//    closed: trains of the runs that start at `first` .. and end at `last`}
// combined as
//   L . R = R has no head ? L : L has no head ? R :
//           {L.first, R.last, R.cap, L.closed + ceil((R.first - L.last) / L.cap) + R.closed}
// which is associative; positions that are no run head (and the unsendable tail) are the identity.  With S
// the summary of [0, p]: rank = p - S.last, p starts a train when rank % S.cap == 0, and its train is number
// S.closed + rank / S.cap.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdint.h>

#include "gcm_internal.h"
#include "send_plan_core.h"

namespace qgcm {

constexpr uint32_t kPlanTile = 256;  // positions per workgroup of the tile and emit kernels, one per lane
constexpr uint32_t kPlanSpineThreads = 1024;
constexpr uint32_t kNone = 0xffffffffu;

struct PlanSeg {
    uint32_t first, last, cap, closed;
};

__device__ inline PlanSeg plan_identity() { return PlanSeg{kNone, 0u, 1u, 0u}; }

__device__ inline PlanSeg plan_combine(const PlanSeg &l, const PlanSeg &r) {
    if (r.first == kNone) return l;
    if (l.first == kNone) return r;
    return PlanSeg{l.first, r.last, r.cap, l.closed + (r.first - l.last + l.cap - 1u) / l.cap + r.closed};
}

__global__ void __launch_bounds__(kPlanTile)
plan_keys_kernel(const uint32_t *lens, const uint32_t *peer, uint32_t n, uint32_t max_keys, uint32_t *keys,
                 uint32_t *vals) {
    const uint32_t i = blockIdx.x * kPlanTile + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = peer[i];
    keys[i] = (p < max_keys && lens[i] != 0u) ? p : max_keys;
    vals[i] = i;
}

// What a lane knows of its position p: the sorted key, the packet's length (the one scattered read), whether
// p is a run head.  s_len[1 + lane] holds the tile's lengths, s_len[0] the length before the tile.
struct PlanItem {
    uint32_t key, len;
    bool sendable, head;
};

__device__ inline PlanItem plan_item(uint32_t p, uint32_t n, uint32_t max_keys, const uint32_t *keys,
                                     const uint32_t *order, const uint32_t *lens, uint32_t *s_len) {
    const uint32_t t = threadIdx.x;
    PlanItem it{max_keys, 0u, false, false};
    if (p < n) {
        it.key = keys[p];
        it.sendable = it.key < max_keys;
        if (it.sendable) it.len = lens[order[p]];
    }
    s_len[1 + t] = it.len;
    // sendable positions come first, so the one before a sendable position is sendable too
    if (t == 0) s_len[0] = (it.sendable && p > 0) ? lens[order[p - 1]] : 0u;
    __syncthreads();
    if (it.sendable) it.head = p == 0 || keys[p - 1] != it.key || s_len[t] != it.len;
    return it;
}

// inclusive scan of one summary per lane over the workgroup's kPlanTile lanes
__device__ inline PlanSeg plan_tile_scan(PlanSeg v, uint32_t *sf, uint32_t *sl, uint32_t *sc, uint32_t *sd) {
    const uint32_t t = threadIdx.x;
    for (uint32_t d = 1; d < kPlanTile; d <<= 1) {
        sf[t] = v.first;
        sl[t] = v.last;
        sc[t] = v.cap;
        sd[t] = v.closed;
        __syncthreads();
        if (t >= d) v = plan_combine(PlanSeg{sf[t - d], sl[t - d], sc[t - d], sd[t - d]}, v);
        __syncthreads();
    }
    return v;
}

__global__ void __launch_bounds__(kPlanTile)
plan_tile_kernel(const uint32_t *keys, const uint32_t *order, const uint32_t *lens, uint32_t n, uint32_t max_keys,
                 qgcm_plan_limits lim, uint4 *tiles) {
    __shared__ uint32_t s_len[kPlanTile + 1], sf[kPlanTile], sl[kPlanTile], sc[kPlanTile], sd[kPlanTile];
    const uint32_t p = blockIdx.x * kPlanTile + threadIdx.x;
    const PlanItem it = plan_item(p, n, max_keys, keys, order, lens, s_len);
    PlanSeg v = plan_identity();
    if (it.head) v = PlanSeg{p, p, plan_cap(it.len, lim.max_segs, lim.max_seg_len, lim.max_bytes), 0u};
    v = plan_tile_scan(v, sf, sl, sc, sd);
    if (threadIdx.x == kPlanTile - 1) tiles[blockIdx.x] = uint4{v.first, v.last, v.cap, v.closed};
}

// tiles[k] <- the summary of tiles [0, k).  One workgroup: each lane folds a stretch of consecutive tiles, the
// stretches' sums are scanned in LDS, and each lane walks its stretch again.
__global__ void __launch_bounds__(kPlanSpineThreads) plan_spine_kernel(uint4 *tiles, uint32_t ntiles) {
    __shared__ uint32_t sf[kPlanSpineThreads], sl[kPlanSpineThreads], sc[kPlanSpineThreads], sd[kPlanSpineThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kPlanSpineThreads - 1) / kPlanSpineThreads;
    const uint32_t lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    PlanSeg v = plan_identity();
    for (uint32_t k = lo; k < hi; ++k) {
        const uint4 x = tiles[k];
        v = plan_combine(v, PlanSeg{x.x, x.y, x.z, x.w});
    }
    for (uint32_t d = 1; d < kPlanSpineThreads; d <<= 1) {
        sf[t] = v.first;
        sl[t] = v.last;
        sc[t] = v.cap;
        sd[t] = v.closed;
        __syncthreads();
        if (t >= d) v = plan_combine(PlanSeg{sf[t - d], sl[t - d], sc[t - d], sd[t - d]}, v);
        __syncthreads();
    }
    sf[t] = v.first;
    sl[t] = v.last;
    sc[t] = v.cap;
    sd[t] = v.closed;
    __syncthreads();
    PlanSeg run = t ? PlanSeg{sf[t - 1], sl[t - 1], sc[t - 1], sd[t - 1]} : plan_identity();
    for (uint32_t k = lo; k < hi; ++k) {
        const uint4 x = tiles[k];
        tiles[k] = uint4{run.first, run.last, run.cap, run.closed};
        run = plan_combine(run, PlanSeg{x.x, x.y, x.z, x.w});
    }
}

__global__ void __launch_bounds__(kPlanTile)
plan_emit_kernel(const uint32_t *keys, const uint32_t *order, const uint32_t *lens, uint32_t n, uint32_t max_keys,
                 qgcm_plan_limits lim, const uint4 *tiles, qgcm_train *trains, uint32_t *counts) {
    __shared__ uint32_t s_len[kPlanTile + 1], sf[kPlanTile], sl[kPlanTile], sc[kPlanTile], sd[kPlanTile];
    const uint32_t t = threadIdx.x;
    const uint32_t p = blockIdx.x * kPlanTile + t;
    const PlanItem it = plan_item(p, n, max_keys, keys, order, lens, s_len);
    PlanSeg v = plan_identity();
    if (it.head) v = PlanSeg{p, p, plan_cap(it.len, lim.max_segs, lim.max_seg_len, lim.max_bytes), 0u};
    v = plan_tile_scan(v, sf, sl, sc, sd);
    if (p == 0 && !it.sendable) {  // nothing sendable in the batch
        counts[0] = 0u;
        counts[1] = 0u;
    }
    if (!it.sendable) return;
    const uint4 x = tiles[blockIdx.x];
    const PlanSeg s = plan_combine(PlanSeg{x.x, x.y, x.z, x.w}, v);  // [0, p]: position 0 is a run head
    const uint32_t rank = p - s.last, in_train = rank % s.cap, train = s.closed + rank / s.cap;
    if (in_train == 0u) {
        trains[train].first = p;
        trains[train].peer = it.key;
        trains[train].seg_len = it.len;
    }
    // the train ends here when the batch's sendable part does, when the next position starts a run, or when
    // the train is full
    const bool more = p + 1u < n && keys[p + 1u] < max_keys;
    bool ends = !more || in_train + 1u == s.cap;
    if (!ends) {
        const uint32_t next_len = t + 1u < kPlanTile ? s_len[2u + t] : lens[order[p + 1u]];
        ends = keys[p + 1u] != it.key || next_len != it.len;
    }
    if (ends) trains[train].count = in_train + 1u;
    if (!more) {
        counts[0] = p + 1u;
        counts[1] = train + 1u;
    }
}

// Onesweep for every size, as worklist.hip's sort (its comment says why not the merge-sort path)
using PlanSortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                  rocprim::default_config, 0>;

static hipError_t plan_sort(void *tmp, size_t &bytes, const uint32_t *k_in, uint32_t *k_out, const uint32_t *v_in,
                            uint32_t *v_out, uint32_t n, int end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs<PlanSortConfig>(tmp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, end_bit, s);
}

namespace {

inline uint64_t al256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline uint32_t plan_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kPlanTile - 1) / kPlanTile); }

}  // namespace

// keys in, values in, keys out (the values out are `order`), the tile summaries, the sort's own area.
// The sort's area is asked for all 32 key bits, which no call exceeds (a context's keys need at most 21): the
// size is a function of n alone, so the caller can allocate before it has a context, and rocprim takes an
// area larger than a sort of fewer bits needs (it only refuses one that is too small).  The query launches
// nothing and touches no stream; it picks the sort's configuration for the current device.
uint64_t send_plan_work_bytes(uint32_t n) {
    size_t sort_bytes = 0;
    if (n && plan_sort(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 32, 0) != hipSuccess) sort_bytes = 0;
    return 3 * al256(4ull * n) + al256(16ull * plan_tiles(n)) + al256(sort_bytes);
}

hipError_t launch_send_plan(uint32_t n, uint32_t max_keys, const uint32_t *lens, const uint32_t *peer,
                            const qgcm_plan_limits &lim, uint32_t *order, qgcm_train *trains, uint32_t *counts,
                            void *work, uint64_t work_bytes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t fixed = 3 * al256(4ull * n) + al256(16ull * plan_tiles(n));
    if (work_bytes < fixed) return hipErrorInvalidValue;
    char *p = static_cast<char *>(work);
    uint32_t *k_in = (uint32_t *)p;  p += al256(4ull * n);
    uint32_t *v_in = (uint32_t *)p;  p += al256(4ull * n);
    uint32_t *k_out = (uint32_t *)p; p += al256(4ull * n);
    const uint32_t ntiles = plan_tiles(n);
    uint4 *tiles = (uint4 *)p;       p += al256(16ull * ntiles);
    size_t sort_bytes = (size_t)(work_bytes - fixed);  // what is left of the area is the sort's
    hipError_t e;
    hipLaunchKernelGGL(plan_keys_kernel, dim3(ntiles), dim3(kPlanTile), 0, s, lens, peer, n, max_keys, k_in, v_in);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // keys are at most max_keys: the bits of that value
    int end_bit = 1;
    while (end_bit < 32 && (1ull << end_bit) <= max_keys) ++end_bit;
    if ((e = plan_sort(p, sort_bytes, k_in, k_out, v_in, order, n, end_bit, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(plan_tile_kernel, dim3(ntiles), dim3(kPlanTile), 0, s, k_out, order, lens, n, max_keys, lim,
                       tiles);
    hipLaunchKernelGGL(plan_spine_kernel, dim3(1), dim3(kPlanSpineThreads), 0, s, tiles, ntiles);
    hipLaunchKernelGGL(plan_emit_kernel, dim3(ntiles), dim3(kPlanTile), 0, s, k_out, order, lens, n, max_keys, lim,
                       tiles, trains, counts);
    return hipGetLastError();
}

}  // namespace qgcm
