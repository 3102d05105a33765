// frames_kernels.hip -- packed TUN frames put into slots and resolved in one launch (include/qgcm.h "outgoing
// frames packed on routed batches").
//
// The fusion of gro_unpack_kernel (gro_kernels.hip) and route_resolve_kernel<outgoing> (route_kernels.hip) for
// the one case the outgoing worker has: frame i of the table belongs to slot i, every frame starts on a 16-byte
// boundary of the packed area, and the packet goes to Raw[4:] of its slot.  So there is no search over the table
// (one 8-byte read a frame), the shift between source and destination is one whole dword known at compile time
// (no v_alignbyte_b32, no dword select), and the destination address Packet[16:20] is the aligned dword at
// packed + off + 16.
//
// Work division: a wave takes 64 consecutive frames a pass, in two phases, and a grid-stride loop of at most
// kFrMaxBlocks workgroups of four waves walks the batch.
//   Resolve: one lane a frame, as route_resolve_kernel has it: the table entry (one 8-byte load, 512 contiguous
//   bytes a wave), the destination address, the probe of the route table (route_core.h: the code the resolve
//   kernel runs), then lens, peer and the descriptor -- coalesced stores.  64 independent lookups are in flight
//   a wave.  (The first form gave the lookup to lane 0 of each frame's 16 copy lanes: four lookups in flight a
//   wave, each a chain of three dependent loads, and 2^20 64-byte frames took 855 us of which the copy was 116;
//   DESIGN.md 4.5.)
//   Copy: eight lanes a frame (128 contiguous bytes a load), eight frames at a time, eight turns; the lanes of a
//   frame read its offset, length and peer from the lane that resolved it (ds_bpermute through __shfl, no LDS
//   allocation, no barrier).  A lane issues the loads of four granules before its first store: the copy of a
//   turn is a chain of load, wait, store, and with one granule in flight a 1350-byte frame was six such chains
//   a turn (1062 us per 2^20 against 1067 for the pair).
//
// Wide path (stride and arena 16-B aligned): the lanes divide the slot by destination granule.  Granule d is
// slot bytes [16 d, 16 d + 16) = frame bytes [16 d - 4, 16 d + 12): the last dword of source piece d - 1 and the
// first three of piece d.  Piece d comes with one aligned 16-byte load, issued only when it holds a byte of the
// frame; of piece d - 1 only the one dword is loaded -- the neighbouring lane loads the whole piece, so the
// dword is served on chip, and a 16-byte load of it would fetch twelve bytes to drop them.  One aligned 16-byte
// store a granule; the last granule stores its whole dwords and at most three single bytes, so the slot's tail
// keeps its bytes.  No byte loads.  Granule 0 is {Raw[0:4], Packet[0:12]}: on a hit {own_ip, Packet[0:12]} in one
// 16-byte store (a hit has len >= 20), on a miss the packet bytes only, so Raw[0:4] keeps its bytes.
// Dword path (a stride that is only a multiple of 4, or an arena off its boundary): the source is still on its
// boundary, so the lanes divide the frame by source piece: one aligned 16-byte load, four dword stores; lane 0
// stores own_ip on a hit.
//
// Memory safety on any table: a frame that is not valid (frames_core.h) reads and writes no byte of packed area
// or arena; of a valid one every loaded piece holds a byte below off + len <= packed_len and lies on its 16-byte
// boundary, so no read passes the boundary behind packed_len; every store lies below 4 + min(len, stride - 4) of
// slot i < n.
#include "frames_core.h"
#include "gcm_internal.h"
#include "route_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kFrThreads = 256;
constexpr uint32_t kFrWave = 64;                       // frames of one wave per pass
constexpr uint32_t kFrLanes = 8;                       // copy lanes of one frame: 128 contiguous bytes a load
constexpr uint32_t kFrGroups = kFrWave / kFrLanes;     // frames copied at a time
constexpr uint32_t kFrTurns = kFrWave / kFrGroups;     // turns of the copy
constexpr uint32_t kFrFlight = 4;                      // granules a lane loads before it stores
constexpr uint32_t kFrWaves = kFrThreads / kFrWave;    // waves of one workgroup
// 8192 waves, about what the 256 CUs hold at once (seven a SIMD); the grid-stride loop takes batches of more than
// 2^19 frames
constexpr uint32_t kFrMaxBlocks = 2048;

// the first nb (0..16) bytes of {w0, w1, w2, w3} to dst (4-B aligned): whole dwords, then at most three bytes
__device__ __forceinline__ void store_part(uint8_t *dst, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t nb) {
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dst);
    const uint32_t whole = nb >> 2, rest = nb & 3u;
    if (whole > 0) d32[0] = w0;
    if (whole > 1) d32[1] = w1;
    if (whole > 2) d32[2] = w2;
    if (whole > 3) d32[3] = w3;
    if (rest) {
        const uint32_t w = whole == 0 ? w0 : whole == 1 ? w1 : whole == 2 ? w2 : w3;
        uint8_t *t = dst + 4 * whole;
        t[0] = (uint8_t)w;
        if (rest > 1) t[1] = (uint8_t)(w >> 8);
        if (rest > 2) t[2] = (uint8_t)(w >> 16);
    }
}

// Raw[4 : 4 + bytes) of slot (16-B aligned) from src (16-B aligned), and own_ip into Raw[0:4] on a hit, by the
// kFrLanes lanes of a frame, lane g of them; bytes <= stride - 4.  A lane issues the loads of kFrFlight granules
// before the first store.
__device__ __forceinline__ void copy_frame16(uint8_t *__restrict__ slot, const uint8_t *__restrict__ src, uint32_t bytes, bool hit,
                                             uint32_t own_ip, uint32_t g) {
    const uint4 *__restrict__ s16 = reinterpret_cast<const uint4 *>(src);
    const uint64_t end = kFramePacketStart + (uint64_t)bytes;  // of the slot
    constexpr uint64_t kStep = 16 * kFrLanes;
    for (uint64_t at0 = 16ull * g; at0 < end; at0 += kStep * kFrFlight) {
        uint4 hi[kFrFlight];
        uint32_t lo[kFrFlight];
#pragma unroll
        for (uint32_t u = 0; u < kFrFlight; ++u) {
            const uint64_t at = at0 + u * kStep;
            hi[u] = make_uint4(0, 0, 0, 0);
            lo[u] = 0;
            if (at < bytes) hi[u] = s16[at >> 4];
            if (at && at < end) lo[u] = *reinterpret_cast<const uint32_t *>(src + at - 4);  // frame byte at - 4 < bytes
        }
#pragma unroll
        for (uint32_t u = 0; u < kFrFlight; ++u) {
            const uint64_t at = at0 + u * kStep;
            if (at >= end) break;
            if (at == 0) {
                // the header granule: a hit has 20 bytes and more, so its granule is whole
                if (hit)
                    *reinterpret_cast<uint4 *>(slot) = make_uint4(own_ip, hi[u].x, hi[u].y, hi[u].z);  // outgoing.go:30
                else
                    store_part(slot + kFramePacketStart, hi[u].x, hi[u].y, hi[u].z, 0, bytes < 12 ? bytes : 12u);
            } else if (end - at >= 16) {
                *reinterpret_cast<uint4 *>(slot + at) = make_uint4(lo[u], hi[u].x, hi[u].y, hi[u].z);
            } else {
                store_part(slot + at, lo[u], hi[u].x, hi[u].y, hi[u].z, (uint32_t)(end - at));
            }
        }
    }
}

// the same for a slot that is only 4-B aligned: by source piece
__device__ __forceinline__ void copy_frame4(uint8_t *__restrict__ slot, const uint8_t *__restrict__ src, uint32_t bytes, bool hit,
                                            uint32_t own_ip, uint32_t g) {
    const uint4 *__restrict__ s16 = reinterpret_cast<const uint4 *>(src);
    constexpr uint64_t kStep = 16 * kFrLanes;
    if (g == 0 && hit) *reinterpret_cast<uint32_t *>(slot) = own_ip;
    for (uint64_t at0 = 16ull * g; at0 < bytes; at0 += kStep * kFrFlight) {
        uint4 w[kFrFlight];
#pragma unroll
        for (uint32_t u = 0; u < kFrFlight; ++u) {
            const uint64_t at = at0 + u * kStep;
            w[u] = make_uint4(0, 0, 0, 0);
            if (at < bytes) w[u] = s16[at >> 4];
        }
#pragma unroll
        for (uint32_t u = 0; u < kFrFlight; ++u) {
            const uint64_t at = at0 + u * kStep;
            if (at >= bytes) break;
            store_part(slot + kFramePacketStart + at, w[u].x, w[u].y, w[u].z, w[u].w, bytes - at < 16 ? (uint32_t)(bytes - at) : 16u);
        }
    }
}

template <bool kWide>
__global__ void __launch_bounds__(kFrThreads) frames_resolve_kernel(FramesArgs a) {
    const uint32_t lane = threadIdx.x % kFrWave, g = lane % kFrLanes, q = lane / kFrLanes;
    const uint64_t waves = (uint64_t)gridDim.x * kFrWaves;
    for (uint64_t base = ((uint64_t)blockIdx.x * kFrWaves + threadIdx.x / kFrWave) * kFrWave; base < a.n; base += waves * kFrWave) {
        // resolve: lane `lane` has frame base + lane
        const uint64_t i = base + lane;
        uint32_t off = 0, bytes = 0, peer = QGCM_NO_PEER;
        bool valid = false;
        if (i < a.n) {
            const uint2 f = reinterpret_cast<const uint2 *>(a.frames)[i];  // {off, len} in one 8-byte load
            const uint64_t slot_off = i * a.stride;
            uint32_t len = 0;
            valid = frame_valid(f.x, f.y, a.packed_len);
            if (valid) {
                off = f.x;
                len = f.y;
                bytes = frame_slot_bytes(len, a.stride);
                // Packet[16:20] must exist, and the sealed datagram must fit the slot (route_resolve_kernel's rule)
                if (len >= 20 && 4ull + len + QGCM_OVERHEAD <= a.stride) {
                    const uint32_t addr = *reinterpret_cast<const uint32_t *>(a.packed + off + 16);
                    const uint32_t key = ((addr ^ a.net) & a.mask) == 0 ? addr : a.gateway;  // router.go:25-30
                    peer = route_lookup(a.table, a.cap_mask, key);
                }
            }
            // a void frame: a packet of length 0 that no route resolves; its slot is not touched
            a.lens[i] = len;
            a.peer[i] = peer;
            *reinterpret_cast<uint4 *>(a.descs + i) = make_uint4((uint32_t)slot_off, (uint32_t)(slot_off >> 32), len, peer);
        }
        // copy: turn t takes frames base + kFrGroups t + q, q = 0..kFrGroups-1, kFrLanes lanes each
        for (uint32_t t = 0; t < kFrTurns; ++t) {
            const uint32_t from = kFrGroups * t + q;
            const uint32_t f_off = __shfl(off, from, kFrWave), f_bytes = __shfl(bytes, from, kFrWave);
            const uint32_t f_peer = __shfl(peer, from, kFrWave);
            const bool f_valid = __shfl((int)valid, from, kFrWave);
            if (!f_valid) continue;  // (also every frame at or past n)
            uint8_t *slot = a.arena + (base + from) * a.stride;
            if (kWide)
                copy_frame16(slot, a.packed + f_off, f_bytes, f_peer != QGCM_NO_PEER, a.own_ip, g);
            else
                copy_frame4(slot, a.packed + f_off, f_bytes, f_peer != QGCM_NO_PEER, a.own_ip, g);
        }
    }
}

}  // namespace

hipError_t launch_frames_resolve(const FramesArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)a.n + kFrThreads - 1) / kFrThreads;
    const dim3 grid((uint32_t)(blocks < kFrMaxBlocks ? blocks : kFrMaxBlocks));
    if ((a.stride & 15) == 0 && ((uintptr_t)a.arena & 15) == 0)
        hipLaunchKernelGGL(frames_resolve_kernel<true>, grid, dim3(kFrThreads), 0, s, a);
    else
        hipLaunchKernelGGL(frames_resolve_kernel<false>, grid, dim3(kFrThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
