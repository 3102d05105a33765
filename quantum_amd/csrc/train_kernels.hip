// train_kernels.hip -- the trains of a planned batch packed back to back (include/qgcm.h "planned trains packed
// on routed batches"): the mirror of gro_kernels.hip.  After the outgoing chain the sealed
// datagrams lie in slots of `stride` bytes and the plan of qgcm_send_plan names them train by train; here every
// train's datagrams Raw[0 : seg_len] are laid one behind the other with no gap, the train rounded up to 16 bytes
// with zeros, so that the copy back moves datagram bytes only and the sender needs one iovec a train.
//
//   train_tile_kernel    each 256-train tile's sum of R                                 one lane per train
//   train_spine_kernel   exclusive prefix of the tile sums, in place                     one workgroup
//   train_emit_kernel    the tile's scan again under its prefix: ptrains and pcounts     one lane per train
//   train_copy_kernel    the datagrams' bytes, 16 lanes per datagram                     grid-stride over p < m
//
// No atomics, no counter to zero, no workgroup waits for another: the scan is reduce-then-scan over separate
// launches as in pack_kernels.hip.  Every kernel reads m and t from the plan's counts on the device (clamped to
// n); the grids are sized by n, so the host does not synchronise between plan and pack.
//
// The copy.  kTrainLanes = 16 lanes per datagram, four datagrams per wave, 16 per workgroup.  A position p of
// `order` finds its train by gro_unpack_kernel's search over trains[].first: a first guess at p * t / m, exact
// for trains of equal counts, a bracket grown from there in doubling steps, a binary search inside it.  The
// source (the slot) is aligned, the destination off + k * seg_len has any alignment: with a seg_len of 1382 it
// walks through every even residue of 16.  The work is divided by destination granule: lane g takes granules
// g, g + 16, ... of the 16-byte lines the datagram touches.  A granule needs source bytes that straddle two
// aligned 16-byte pieces; both are loaded (the second is the next lane's first, so it is served on chip) and
// realigned in registers -- a dword select for bits 2-3 of the shift, the byte-align funnel shift
// (v_alignbyte_b32) for bits 0-1 -- as copy_slot16 does in the other direction.  A piece is loaded only when it
// holds a byte below seg_len, so no read reaches min(round16(seg_len), stride) of the slot; its bytes at or past
// seg_len are masked to zero, which is the train's padding where the last datagram owns it.
// A granule the datagram owns whole is one aligned 16-byte store.  The first and the last granule may be shared
// with the neighbouring datagrams, whose lane groups -- in other waves, other workgroups -- write them at the same
// time: such a granule is never read and never written whole.  Each owner stores the dwords it owns whole and at
// most three single bytes at each end, so every byte of the packed area has exactly one writer.
// A lane issues the loads of kTrainFlight granules before it stores the first (kPackFlight's reason).
// Dword path (a stride that is only a multiple of 4, or an arena off its 16-B boundary): the same by
// destination dword, with aligned dword loads.
//
// A malformed plan stays memory-safe: every train index is checked against t, every position against m <= n, a
// void train (train_core.h) has off = 0xffffffff and is not copied, a member with order[p] >= n is copied as
// zeros, and a train is copied only when the emit pass found off + R <= packed_cap for the same table entry.
#include "gcm_internal.h"
#include "train_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kTrainTile = 256;  // trains per workgroup of the tile and emit kernels, one per lane
constexpr uint32_t kTrainSpineThreads = 1024;
constexpr uint32_t kTrainThreads = 256;                          // the copy kernel
constexpr uint32_t kTrainLanes = 16;                             // lanes of one datagram
constexpr uint32_t kTrainDgrams = kTrainThreads / kTrainLanes;   // datagrams of one workgroup per pass
constexpr uint32_t kTrainMaxBlocks = 4096;                       // as gro_unpack_kernel's grid
constexpr uint32_t kTrainFlight = 4;                             // granules a lane loads before it stores the first

struct TrainArgs {
    const uint8_t *arena;
    uint64_t stride;
    uint32_t n;
    const uint32_t *order;
    const qgcm_train *trains;
    const uint32_t *plan_counts;  // {m, t}, read on the device
    uint8_t *packed;
    uint64_t packed_cap;
    qgcm_ptrain *ptrains;
    uint64_t *pcounts;
    uint64_t *tiles;  // sum of R per tile
};

__device__ inline uint32_t plan_m(const TrainArgs &a) { return min(a.plan_counts[0], a.n); }
__device__ inline uint32_t plan_t(const TrainArgs &a) { return min(a.plan_counts[1], a.n); }

// A lane's train {first, count, peer, seg_len} and its size (0: void, or past t)
__device__ inline uint64_t train_item(const TrainArgs &a, uint32_t j, uint32_t m, uint32_t t, uint4 &tr) {
    tr = make_uint4(0, 0, 0, 0);
    if (j >= t) return 0;
    tr = *reinterpret_cast<const uint4 *>(a.trains + j);
    return train_void(tr.x, tr.y, tr.w, m, a.stride) ? 0 : train_bytes(tr.y, tr.w);
}

// inclusive scan over the workgroup's kThreads lanes
template <uint32_t kThreads>
__device__ inline void train_scan(uint64_t &bytes, uint64_t *sb) {
    const uint32_t t = threadIdx.x;
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        sb[t] = bytes;
        __syncthreads();
        if (t >= d) bytes += sb[t - d];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kTrainTile) train_tile_kernel(TrainArgs a) {
    __shared__ uint64_t sb[kTrainTile];
    uint4 tr;
    uint64_t bytes = train_item(a, blockIdx.x * kTrainTile + threadIdx.x, plan_m(a), plan_t(a), tr);
    train_scan<kTrainTile>(bytes, sb);
    if (threadIdx.x == kTrainTile - 1) a.tiles[blockIdx.x] = bytes;
}

// tiles[k] <- the sum of tiles [0, k).  One workgroup: each lane folds a stretch of consecutive tiles, the
// stretches' sums are scanned in LDS, and each lane walks its stretch again.
__global__ void __launch_bounds__(kTrainSpineThreads) train_spine_kernel(uint64_t *tiles, uint32_t ntiles) {
    __shared__ uint64_t sb[kTrainSpineThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kTrainSpineThreads - 1) / kTrainSpineThreads;
    const uint32_t lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    uint64_t bytes = 0;
    for (uint32_t k = lo; k < hi; ++k) bytes += tiles[k];
    const uint64_t own = bytes;
    train_scan<kTrainSpineThreads>(bytes, sb);
    uint64_t run = bytes - own;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint64_t x = tiles[k];
        tiles[k] = run;
        run += x;
    }
}

__global__ void __launch_bounds__(kTrainTile) train_emit_kernel(TrainArgs a) {
    __shared__ uint64_t sb[kTrainTile];
    const uint32_t j = blockIdx.x * kTrainTile + threadIdx.x;
    const uint32_t t = plan_t(a);
    uint4 tr;
    const uint64_t R = train_item(a, j, plan_m(a), t, tr);
    uint64_t bytes = R;
    train_scan<kTrainTile>(bytes, sb);
    const uint64_t before = a.tiles[blockIdx.x];
    if (j < t) {
        const uint64_t off = before + bytes - R;
        const bool fits = R != 0 && off + R <= a.packed_cap;  // R == 0: a void train
        *reinterpret_cast<uint4 *>(a.ptrains + j) = make_uint4(fits ? (uint32_t)off : kTrainNoRoom, tr.y, tr.z, tr.w);
    }
    if (j == (t ? t - 1u : 0u)) {
        a.pcounts[0] = t;
        a.pcounts[1] = before + bytes;
    }
}

// ({hi, lo} >> 8 * (shift & 3)) & 0xffffffff
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t shift) {
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
}

// w with its bytes from `keep` (0..4, clamped) on set to zero
__device__ __forceinline__ uint32_t keep_bytes(uint32_t w, int32_t keep) {
    return keep >= 4 ? w : keep <= 0 ? 0u : w & ((1u << (8 * keep)) - 1u);
}

__device__ __forceinline__ uint4 keep_bytes16(uint4 v, int32_t keep) {
    return make_uint4(keep_bytes(v.x, keep), keep_bytes(v.y, keep - 4), keep_bytes(v.z, keep - 8), keep_bytes(v.w, keep - 12));
}

// bytes [b0, b1) of the aligned dword at d from w (0 <= b0 < b1 <= 4): the dword when it is owned whole, else
// single bytes -- never a read-modify-write, the other bytes are a neighbour's
__device__ __forceinline__ void store_dword_part(uint8_t *d, uint32_t w, uint32_t b0, uint32_t b1) {
    if (b0 == 0 && b1 == 4) {
        *reinterpret_cast<uint32_t *>(d) = w;
        return;
    }
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if (b >= b0 && b < b1) d[b] = (uint8_t)(w >> (8 * b));
}

// The datagram at packed + at (any alignment) from src (16-B aligned): bytes [0, have) from the slot, bytes
// [have, total) zero, by the kTrainLanes lanes of a group, lane g of them.
__device__ __forceinline__ void copy_dgram16(uint8_t *__restrict__ packed, uint64_t at, const uint8_t *__restrict__ src,
                                             uint32_t have, uint32_t total, uint32_t g) {
    const uint32_t a = (uint32_t)at & 15u;
    uint8_t *__restrict__ dst = packed + (at - a);  // the first granule the datagram touches
    // granule j holds datagram bytes [16 j - a, 16 j - a + 16): byte sh of {piece j - back, piece j}
    const uint32_t sh = (16u - a) & 15u, back = a ? 1u : 0u;
    const bool q2 = sh & 8u, q1 = sh & 4u;
    const uint32_t r = sh & 3u;
    const uint4 *__restrict__ s16 = reinterpret_cast<const uint4 *>(src);
    const uint32_t granules = (a + total + 15u) >> 4;
    for (uint32_t j0 = g; j0 < granules; j0 += kTrainFlight * kTrainLanes) {
        uint4 lo[kTrainFlight], hi[kTrainFlight];
#pragma unroll
        for (uint32_t f = 0; f < kTrainFlight; ++f) {
            const uint32_t j = j0 + f * kTrainLanes;
            lo[f] = hi[f] = make_uint4(0, 0, 0, 0);
            if (j < granules) {
                // a piece is read only when it holds a byte below `have`
                if (j >= back && 16ull * (j - back) < have) lo[f] = s16[j - back];
                if (back && 16ull * j < have) hi[f] = s16[j];
            }
        }
#pragma unroll
        for (uint32_t f = 0; f < kTrainFlight; ++f) {
            const uint32_t j = j0 + f * kTrainLanes;
            if (j >= granules) break;
            const int64_t keep_lo = (int64_t)have - 16ll * ((int64_t)j - back), keep_hi = (int64_t)have - 16ll * j;
            if (keep_lo < 16) lo[f] = keep_bytes16(lo[f], keep_lo < 0 ? 0 : (int32_t)keep_lo);
            if (keep_hi < 16) hi[f] = keep_bytes16(hi[f], keep_hi < 0 ? 0 : (int32_t)keep_hi);
            const uint4 l = lo[f], h = hi[f];
            // dwords q .. q + 4 of {l, h}, q = sh >> 2
            const uint32_t a0 = q2 ? l.z : l.x, a1 = q2 ? l.w : l.y, a2 = q2 ? h.x : l.z, a3 = q2 ? h.y : l.w,
                           a4 = q2 ? h.z : h.x, a5 = q2 ? h.w : h.y;
            const uint32_t b0 = q1 ? a1 : a0, b1 = q1 ? a2 : a1, b2 = q1 ? a3 : a2, b3 = q1 ? a4 : a3, b4 = q1 ? a5 : a4;
            const uint4 out = make_uint4(funnel(b1, b0, r), funnel(b2, b1, r), funnel(b3, b2, r), funnel(b4, b3, r));
            // the bytes [own0, own1) of the granule are this datagram's
            const uint32_t own0 = j == 0 ? a : 0u;
            const uint32_t left = a + total - 16u * j;  // >= 1
            const uint32_t own1 = left < 16u ? left : 16u;
            uint8_t *d = dst + 16ull * j;
            if (own0 == 0 && own1 == 16) {
                *reinterpret_cast<uint4 *>(d) = out;
            } else {
                const uint32_t w[4] = {out.x, out.y, out.z, out.w};
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t s = own0 > 4 * q ? own0 : 4 * q, e = own1 < 4 * q + 4 ? own1 : 4 * q + 4;
                    if (s < e) store_dword_part(d + 4 * q, w[q], s - 4 * q, e - 4 * q);
                }
            }
        }
    }
}

// the same by destination dword, for a src that is only 4-B aligned
__device__ __forceinline__ void copy_dgram4(uint8_t *__restrict__ packed, uint64_t at, const uint8_t *__restrict__ src,
                                            uint32_t have, uint32_t total, uint32_t g) {
    const uint32_t a = (uint32_t)at & 3u;
    uint8_t *__restrict__ dst = packed + (at - a);
    const uint32_t sh = (4u - a) & 3u, back = a ? 1u : 0u;
    const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(src);
    const uint32_t words = (a + total + 3u) >> 2;
    for (uint32_t j0 = g; j0 < words; j0 += kTrainFlight * kTrainLanes) {
        uint32_t lo[kTrainFlight], hi[kTrainFlight];
#pragma unroll
        for (uint32_t f = 0; f < kTrainFlight; ++f) {
            const uint32_t j = j0 + f * kTrainLanes;
            lo[f] = hi[f] = 0;
            if (j < words) {
                if (j >= back && 4ull * (j - back) < have) lo[f] = s4[j - back];
                if (back && 4ull * j < have) hi[f] = s4[j];
            }
        }
#pragma unroll
        for (uint32_t f = 0; f < kTrainFlight; ++f) {
            const uint32_t j = j0 + f * kTrainLanes;
            if (j >= words) break;
            const int64_t keep_lo = (int64_t)have - 4ll * ((int64_t)j - back), keep_hi = (int64_t)have - 4ll * j;
            const uint32_t l = keep_bytes(lo[f], keep_lo > 4 ? 4 : keep_lo < 0 ? 0 : (int32_t)keep_lo);
            const uint32_t h = keep_bytes(hi[f], keep_hi > 4 ? 4 : keep_hi < 0 ? 0 : (int32_t)keep_hi);
            const uint32_t own0 = j == 0 ? a : 0u;
            const uint32_t left = a + total - 4u * j;  // >= 1
            store_dword_part(dst + 4ull * j, funnel(h, l, sh), own0, left < 4u ? left : 4u);
        }
    }
}

template <bool kWide>
__global__ void __launch_bounds__(kTrainThreads) train_copy_kernel(TrainArgs a) {
    const uint32_t g = threadIdx.x % kTrainLanes;
    const uint32_t m = plan_m(a), t = plan_t(a);
    if (t == 0) return;
    for (uint64_t p = (uint64_t)blockIdx.x * kTrainDgrams + threadIdx.x / kTrainLanes; p < m;
         p += (uint64_t)gridDim.x * kTrainDgrams) {
        // the last train whose first is at or below p, kept in [lo, hi): trains[lo].first <= p unless lo is 0,
        // trains[hi].first > p unless hi is t.  Trains of equal counts would put position p into train
        // p * t / m; the bracket is grown from there in doubling steps, then halved.
        uint32_t lo = 0, hi = t;
        const uint32_t guess = (uint32_t)(p * t / m);  // < t
        if (a.trains[guess].first <= p) {
            lo = guess;
            uint32_t step = 1;
            while (hi - lo > step && a.trains[lo + step].first <= p) {
                lo += step;
                step <<= 1;
            }
            if (hi - lo > step) hi = lo + step;
        } else {
            hi = guess;
            uint32_t step = 1;
            while (step <= hi && a.trains[hi - step].first > p) {
                hi -= step;
                step <<= 1;
            }
            lo = step <= hi ? hi - step : 0;
        }
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (a.trains[mid].first <= p)
                lo = mid;
            else
                hi = mid;
        }
        const uint4 tr = *reinterpret_cast<const uint4 *>(a.trains + lo);  // {first, count, peer, seg_len}
        if (p < tr.x || p - tr.x >= tr.y) continue;
        // what the emit pass made of the same entry: a void train and one that did not fit have nothing to move
        const uint32_t off = a.ptrains[lo].off;
        if (off == kTrainNoRoom) continue;
        const uint32_t k = (uint32_t)(p - tr.x), L = tr.w;
        const uint64_t at = (uint64_t)off + (uint64_t)k * L;  // off + R <= packed_cap < 2^32
        // the train's last datagram owns the padding up to R
        const uint32_t total = k + 1 == tr.y ? (uint32_t)(train_bytes(tr.y, L) - (uint64_t)k * L) : L;
        const uint32_t slot = a.order[p];
        const bool named = slot < a.n;  // else the member is zeros: no slot is read
        const uint8_t *src = a.arena + (named ? (uint64_t)slot * a.stride : 0);
        if (kWide)
            copy_dgram16(a.packed, at, src, named ? L : 0u, total, g);
        else
            copy_dgram4(a.packed, at, src, named ? L : 0u, total, g);
    }
}

inline uint32_t train_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kTrainTile - 1) / kTrainTile); }

}  // namespace

uint64_t train_pack_work_bytes(uint32_t n) {
    const uint64_t b = 8ull * train_tiles(n);
    return b < 256 ? 256 : (b + 255) & ~(uint64_t)255;
}

hipError_t launch_train_pack(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *order,
                             const qgcm_train *trains, const uint32_t *plan_counts, uint8_t *packed, uint64_t packed_cap,
                             qgcm_ptrain *ptrains, uint64_t *pcounts, void *work, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(pcounts, 0, 16, s);
    TrainArgs a{arena, stride, n, order, trains, plan_counts, packed, packed_cap, ptrains, pcounts, static_cast<uint64_t *>(work)};
    const uint32_t ntiles = train_tiles(n);
    hipLaunchKernelGGL(train_tile_kernel, dim3(ntiles), dim3(kTrainTile), 0, s, a);
    hipLaunchKernelGGL(train_spine_kernel, dim3(1), dim3(kTrainSpineThreads), 0, s, a.tiles, ntiles);
    hipLaunchKernelGGL(train_emit_kernel, dim3(ntiles), dim3(kTrainTile), 0, s, a);
    const uint64_t blocks = ((uint64_t)n + kTrainDgrams - 1) / kTrainDgrams;
    const dim3 grid((uint32_t)(blocks < kTrainMaxBlocks ? blocks : kTrainMaxBlocks));
    if ((stride & 15) == 0 && ((uintptr_t)arena & 15) == 0)
        hipLaunchKernelGGL(train_copy_kernel<true>, grid, dim3(kTrainThreads), 0, s, a);
    else
        hipLaunchKernelGGL(train_copy_kernel<false>, grid, dim3(kTrainThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
