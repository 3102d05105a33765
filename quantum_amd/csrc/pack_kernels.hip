// pack_kernels.hip -- delivered packets of a routed batch packed back to back (include/qgcm.h "delivered
// packets packed on routed batches"): the mirror of gro_kernels.hip.  After the incoming chain
// the delivered packets lie scattered over slots of `stride` bytes; here their records Raw[0 : 4 + L], each
// rounded up to 16 bytes with zeros, are laid one behind the other in arena order, with a table that names
// them, so that the copy back and the TUN write move delivered bytes only.
//
//   pack_tile_kernel    each 256-packet tile's summary {sum of R, delivered count}     one lane per packet
//   pack_spine_kernel   exclusive prefix of the tile summaries, in place               one workgroup
//   pack_emit_kernel    the tile's scan again under its prefix: recs and counts        one lane per packet
//   pack_copy_kernel    the records' bytes, 16 lanes per record                        grid-stride over k < m
//
// No atomics, no counter to zero, no workgroup waits for another: the scan is reduce-then-scan over separate
// launches as in plan_kernels.hip, so calls on several streams share nothing but read-only inputs.  The copy
// reads m from `counts` on the device; the host does not synchronise between the launches.
//
// The copy.  kPackLanes = 16 lanes per record, four records per wave, 16 per workgroup, as the unpack divides
// its slots.  A group reads its table entry with one 16-byte load -- no search: the emit pass has written where
// every record goes, which is the advantage this direction has over the unpack.  Source (the slot) and
// destination (off, a multiple of 16) are both aligned, so a piece is one aligned 16-byte load and one aligned
// 16-byte store with nothing to realign; the record's last piece is masked to zero behind byte 4 + L in
// registers.  No byte loads, no byte stores.  A lane issues kPackFlight loads before it stores the first of
// them (DESIGN.md 4.5 has what one load in flight cost).  R <= stride on the 16-byte path (stride is a multiple of 16 and
// 4 + L <= stride), so no load reaches the next slot; the dword path loads only dwords that hold a byte below
// 4 + L, which end at or below stride because stride is a multiple of 4.  A record whose `off` says it did not
// fit is not copied, so nothing at or past packed_cap is written.
#include "gcm_internal.h"
#include "pack_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kPackTile = 256;  // packets per workgroup of the tile and emit kernels, one per lane
constexpr uint32_t kPackSpineThreads = 1024;
constexpr uint32_t kPackThreads = 256;                       // the copy kernel
constexpr uint32_t kPackLanes = 16;                          // lanes of one record
constexpr uint32_t kPackRecs = kPackThreads / kPackLanes;    // records of one workgroup per pass
constexpr uint32_t kPackMaxBlocks = 4096;                    // as gro_unpack_kernel's grid
constexpr uint32_t kPackFlight = 4;                          // pieces a lane loads before it stores the first

struct PackArgs {
    const uint8_t *arena;
    uint64_t stride;
    uint32_t n;
    const uint32_t *lens, *peer;
    const uint8_t *status;  // NULL: every packet has status 1
    uint8_t *packed;
    uint64_t packed_cap;
    qgcm_pack_rec *recs;
    uint64_t *counts;
    ulonglong2 *tiles;  // {sum of R, delivered count} per tile
};

// A lane's packet: its length and record size (0: not delivered)
struct PackItem {
    uint32_t len;
    uint64_t rec;
};

__device__ inline PackItem pack_item(const PackArgs &a, uint32_t i) {
    PackItem it{0u, 0ull};
    if (i < a.n) {
        it.len = a.lens[i];
        if (pack_delivered(a.status ? a.status[i] : 1u, it.len, a.stride)) it.rec = pack_rec_bytes(it.len);
    }
    return it;
}

// inclusive scan of {bytes, count} over the workgroup's kThreads lanes
template <uint32_t kThreads>
__device__ inline void pack_scan(uint64_t &bytes, uint32_t &count, uint64_t *sb, uint32_t *sc) {
    const uint32_t t = threadIdx.x;
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        sb[t] = bytes;
        sc[t] = count;
        __syncthreads();
        if (t >= d) {
            bytes += sb[t - d];
            count += sc[t - d];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kPackTile) pack_tile_kernel(PackArgs a) {
    __shared__ uint64_t sb[kPackTile];
    __shared__ uint32_t sc[kPackTile];
    const PackItem it = pack_item(a, blockIdx.x * kPackTile + threadIdx.x);
    uint64_t bytes = it.rec;
    uint32_t count = it.rec != 0;
    pack_scan<kPackTile>(bytes, count, sb, sc);
    if (threadIdx.x == kPackTile - 1) a.tiles[blockIdx.x] = ulonglong2{bytes, count};
}

// tiles[k] <- the sum of tiles [0, k).  One workgroup: each lane folds a stretch of consecutive tiles, the
// stretches' sums are scanned in LDS, and each lane walks its stretch again.
__global__ void __launch_bounds__(kPackSpineThreads) pack_spine_kernel(ulonglong2 *tiles, uint32_t ntiles) {
    __shared__ uint64_t sb[kPackSpineThreads];
    __shared__ uint32_t sc[kPackSpineThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kPackSpineThreads - 1) / kPackSpineThreads;
    const uint32_t lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    uint64_t bytes = 0;
    uint32_t count = 0;
    for (uint32_t k = lo; k < hi; ++k) {
        const ulonglong2 x = tiles[k];
        bytes += x.x;
        count += (uint32_t)x.y;
    }
    const uint64_t own_b = bytes;
    const uint32_t own_c = count;
    pack_scan<kPackSpineThreads>(bytes, count, sb, sc);
    uint64_t run_b = bytes - own_b;
    uint64_t run_c = count - own_c;
    for (uint32_t k = lo; k < hi; ++k) {
        const ulonglong2 x = tiles[k];
        tiles[k] = ulonglong2{run_b, run_c};
        run_b += x.x;
        run_c += x.y;
    }
}

__global__ void __launch_bounds__(kPackTile) pack_emit_kernel(PackArgs a) {
    __shared__ uint64_t sb[kPackTile];
    __shared__ uint32_t sc[kPackTile];
    const uint32_t i = blockIdx.x * kPackTile + threadIdx.x;
    const PackItem it = pack_item(a, i);
    uint64_t bytes = it.rec;
    uint32_t count = it.rec != 0;
    pack_scan<kPackTile>(bytes, count, sb, sc);
    if (i >= a.n) return;
    const ulonglong2 before = a.tiles[blockIdx.x];
    if (it.rec) {
        const uint64_t off = before.x + bytes - it.rec;
        const uint32_t k = (uint32_t)before.y + count - 1u;
        const bool fits = off + it.rec <= a.packed_cap;
        *reinterpret_cast<uint4 *>(a.recs + k) = make_uint4(fits ? (uint32_t)off : kPackNoRoom, it.len, i, a.peer[i]);
    }
    if (i == a.n - 1u) {
        a.counts[0] = before.y + count;
        a.counts[1] = before.x + bytes;
    }
}

// w with its bytes from `keep` (0..4, clamped) on set to zero
__device__ __forceinline__ uint32_t keep_bytes(uint32_t w, int32_t keep) {
    return keep >= 4 ? w : keep <= 0 ? 0u : w & ((1u << (8 * keep)) - 1u);
}

template <bool kWide>
__global__ void __launch_bounds__(kPackThreads) pack_copy_kernel(PackArgs a) {
    const uint32_t g = threadIdx.x % kPackLanes;
    const uint64_t m = a.counts[0];
    for (uint64_t k = (uint64_t)blockIdx.x * kPackRecs + threadIdx.x / kPackLanes; k < m;
         k += (uint64_t)gridDim.x * kPackRecs) {
        const uint4 rec = *reinterpret_cast<const uint4 *>(a.recs + k);  // {off, len, slot, peer}
        // a record that did not fit has nothing to move (no early way out: the entry stays one load)
        const uint32_t need = rec.x == kPackNoRoom ? 0u : 4u + rec.y;  // off + R <= packed_cap < 2^32: no wrap
        const uint8_t *__restrict__ src = a.arena + (uint64_t)rec.z * a.stride;
        uint8_t *__restrict__ dst = a.packed + rec.x;
        if (kWide) {
            const uint4 *__restrict__ s16 = reinterpret_cast<const uint4 *>(src);
            uint4 *__restrict__ d16 = reinterpret_cast<uint4 *>(dst);
            const uint32_t pieces = (need + 15u) >> 4;
            // kPackFlight loads of a lane are issued before the first of them is stored: written as one loop
            // the compiler keeps a single load in flight (each store waits for the load before it)
            for (uint32_t p0 = g; p0 < pieces; p0 += kPackFlight * kPackLanes) {
                uint4 v[kPackFlight];
#pragma unroll
                for (uint32_t j = 0; j < kPackFlight; ++j) {
                    const uint32_t p = p0 + j * kPackLanes;
                    if (p < pieces) v[j] = s16[p];
                }
#pragma unroll
                for (uint32_t j = 0; j < kPackFlight; ++j) {
                    const uint32_t p = p0 + j * kPackLanes;
                    if (p >= pieces) break;
                    const uint32_t left = need - 16u * p;  // >= 1
                    if (left < 16u) {
                        const int32_t keep = (int32_t)left;
                        v[j].x = keep_bytes(v[j].x, keep);
                        v[j].y = keep_bytes(v[j].y, keep - 4);
                        v[j].z = keep_bytes(v[j].z, keep - 8);
                        v[j].w = keep_bytes(v[j].w, keep - 12);
                    }
                    d16[p] = v[j];
                }
            }
        } else {
            const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(src);
            uint32_t *__restrict__ d4 = reinterpret_cast<uint32_t *>(dst);
            const uint32_t words = ((need + 15u) >> 4) << 2;
            for (uint32_t w0 = g; w0 < words; w0 += kPackFlight * kPackLanes) {
                uint32_t v[kPackFlight];
#pragma unroll
                for (uint32_t j = 0; j < kPackFlight; ++j) {
                    const uint32_t w = w0 + j * kPackLanes;
                    v[j] = 0;
                    if (4ull * w < need) v[j] = s4[w];  // else a dword of the padding
                }
#pragma unroll
                for (uint32_t j = 0; j < kPackFlight; ++j) {
                    const uint32_t w = w0 + j * kPackLanes;
                    if (w >= words) break;
                    const int64_t keep = (int64_t)need - 4ll * w;
                    d4[w] = keep_bytes(v[j], keep < 4 ? (int32_t)keep : 4);
                }
            }
        }
    }
}

inline uint32_t pack_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kPackTile - 1) / kPackTile); }

}  // namespace

uint64_t deliver_pack_work_bytes(uint32_t n) {
    const uint64_t b = 16ull * pack_tiles(n);
    return b < 256 ? 256 : (b + 255) & ~(uint64_t)255;
}

hipError_t launch_deliver_pack(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                               const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_pack_rec *recs,
                               uint64_t *counts, void *work, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(counts, 0, 16, s);
    PackArgs a{arena, stride, n, lens, peer, status, packed, packed_cap, recs, counts, static_cast<ulonglong2 *>(work)};
    const uint32_t ntiles = pack_tiles(n);
    hipLaunchKernelGGL(pack_tile_kernel, dim3(ntiles), dim3(kPackTile), 0, s, a);
    hipLaunchKernelGGL(pack_spine_kernel, dim3(1), dim3(kPackSpineThreads), 0, s, a.tiles, ntiles);
    hipLaunchKernelGGL(pack_emit_kernel, dim3(ntiles), dim3(kPackTile), 0, s, a);
    const uint64_t blocks = ((uint64_t)n + kPackRecs - 1) / kPackRecs;
    const dim3 grid((uint32_t)(blocks < kPackMaxBlocks ? blocks : kPackMaxBlocks));
    if ((stride & 15) == 0 && ((uintptr_t)arena & 15) == 0)
        hipLaunchKernelGGL(pack_copy_kernel<true>, grid, dim3(kPackThreads), 0, s, a);
    else
        hipLaunchKernelGGL(pack_copy_kernel<false>, grid, dim3(kPackThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
