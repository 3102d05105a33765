// gro_copy.h -- the copy of one datagram from an arbitrarily aligned source into its aligned slot, by the
// kGroLanes lanes of that slot: the code gro_unpack_kernel (gro_kernels.hip) and gro_resolve_kernel
// (gro_resolve_kernels.hip) share.  Device code only.
//
// 16-byte path (stride and arena 16-B aligned): per piece two aligned 16-byte loads that straddle the
// source bytes, realigned in registers -- a dword select for bits 2-3 of the source address, the byte-align
// funnel shift (v_alignbyte_b32) for bits 0-1 -- and one aligned 16-byte store.  The second load is the next
// lane's first, so it is served on chip.  It is issued only when a byte of it is needed, which keeps every
// read below the 16-byte boundary behind the buffer's end.  The last piece of a datagram stores its whole
// dwords and then at most three single bytes, so the slot's tail keeps its bytes.  No byte loads.
// Dword path (a stride that is only a multiple of 4): the same with aligned dword loads and stores.
#pragma once
#include "gcm_internal.h"

namespace qgcm {
namespace {

constexpr uint32_t kGroLanes = 16;                          // lanes of one slot

// ({hi, lo} >> 8 * (shift & 3)) & 0xffffffff
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t shift) {
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
}

// the last `nb` (1..3) bytes of a piece, from the low end of w
__device__ __forceinline__ void store_tail_bytes(uint8_t *dst, uint32_t w, uint32_t nb) {
    dst[0] = (uint8_t)w;
    if (nb > 1) dst[1] = (uint8_t)(w >> 8);
    if (nb > 2) dst[2] = (uint8_t)(w >> 16);
}

// bytes [0, bytes) of dst (16-B aligned) from src (any alignment; src - (src & 15) is 16-B aligned), by the
// kGroLanes lanes of a slot, lane g of them
__device__ __forceinline__ void copy_slot16(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes,
                                            uint32_t g) {
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15u);
    const uint4 *__restrict__ s16 = reinterpret_cast<const uint4 *>(src - sh);
    const bool q2 = sh & 8u, q1 = sh & 4u;
    const uint32_t r = sh & 3u;
    for (uint32_t at = 16 * g; at < bytes; at += 16 * kGroLanes) {
        const uint32_t nb = bytes - at < 16 ? bytes - at : 16;
        const uint4 lo = s16[at >> 4];
        uint4 hi = make_uint4(0, 0, 0, 0);
        if (sh + nb > 16) hi = s16[(at >> 4) + 1];
        // dwords q .. q + 4 of {lo, hi}, q = sh >> 2
        const uint32_t a0 = q2 ? lo.z : lo.x, a1 = q2 ? lo.w : lo.y, a2 = q2 ? hi.x : lo.z, a3 = q2 ? hi.y : lo.w,
                       a4 = q2 ? hi.z : hi.x, a5 = q2 ? hi.w : hi.y;
        const uint32_t b0 = q1 ? a1 : a0, b1 = q1 ? a2 : a1, b2 = q1 ? a3 : a2, b3 = q1 ? a4 : a3, b4 = q1 ? a5 : a4;
        const uint4 out = make_uint4(funnel(b1, b0, r), funnel(b2, b1, r), funnel(b3, b2, r), funnel(b4, b3, r));
        uint8_t *d = dst + at;
        if (nb == 16) {
            *reinterpret_cast<uint4 *>(d) = out;
        } else {
            uint32_t *d32 = reinterpret_cast<uint32_t *>(d);
            const uint32_t whole = nb >> 2;
            if (whole > 0) d32[0] = out.x;
            if (whole > 1) d32[1] = out.y;
            if (whole > 2) d32[2] = out.z;
            if (nb & 3u) store_tail_bytes(d + 4 * whole, whole == 0 ? out.x : whole == 1 ? out.y : whole == 2 ? out.z : out.w, nb & 3u);
        }
    }
}

// the same in dwords, for a dst that is only 4-B aligned
__device__ __forceinline__ void copy_slot4(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes,
                                           uint32_t g) {
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(src - sh);
    for (uint32_t at = 4 * g; at < bytes; at += 4 * kGroLanes) {
        const uint32_t nb = bytes - at < 4 ? bytes - at : 4;
        const uint32_t lo = s4[at >> 2];
        uint32_t hi = 0;
        if (sh + nb > 4) hi = s4[(at >> 2) + 1];
        const uint32_t out = funnel(hi, lo, sh);
        if (nb == 4)
            *reinterpret_cast<uint32_t *>(dst + at) = out;
        else
            store_tail_bytes(dst + at, out, nb);
    }
}

}  // namespace
}  // namespace qgcm
