// x25519_kernels.hip -- peer secrets computed on the GPU: out = X25519(scalar, point) (x25519_core.h), one
// Montgomery ladder per lane.
//
// A ladder is a serial chain of 255 steps of five field multiplications, four squarings and one
// multiplication by 121665 on ten 26/25-bit limbs, then an inversion (254 squarings, 11 multiplications),
// with no memory traffic between the 64 B it loads and the 32 B it stores: pure VALU work in registers,
// no LDS and no scratch.  The arithmetic is x25519_core.h's as the host compiles it; every product term is
// one v_mad_u64_u32.  The ladder loop and the inversion's runs of squarings stay rolled (one step is about
// 11 KiB of code), everything inside a step is straight-line code on constant limb indices.
//
// Constant time per lane as in x25519_core.h; across a wave there is nothing to diverge on, since every
// lane runs the same 255 steps.
#include <hip/hip_runtime.h>

#include "gcm_internal.h"
#include "x25519_core.h"

namespace qgcm {

namespace {

// out[i] = X25519(scalar of lane i, points[i]): 32 B each, 4-B aligned.  scalar_stride 32: lane i's scalar
// is scalars + 32 i; scalar_stride 0: scalars for lanes below `split`, scalars + 32 from there on (split >=
// count: one scalar for all -- a peer table's secrets and salts are one launch over both private values).
// out may be points: a lane loads its point before it stores, and no lane reads another's.
__global__ void __launch_bounds__(64) x25519_ladder_kernel(const uint8_t *scalars, uint32_t scalar_stride,
                                                           const uint8_t *points, uint32_t count, uint8_t *out,
                                                           uint32_t split) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= count) return;  // before any load
    const uint32_t *ps = (const uint32_t *)(scalars + (scalar_stride ? (uint64_t)scalar_stride * i : i >= split ? 32u : 0u));
    const uint32_t *pp = (const uint32_t *)(points + 32ull * i);
    uint32_t k[8], u[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        k[j] = ps[j];
        u[j] = pp[j];
    }
    x25519_words(r, k, u);
    uint32_t *po = (uint32_t *)(out + 32ull * i);
#pragma unroll
    for (int j = 0; j < 8; ++j) po[j] = r[j];
}

}  // namespace

hipError_t launch_x25519(const uint8_t *d_scalars, uint32_t scalar_stride, const uint8_t *d_points, uint32_t count,
                         uint8_t *d_out, uint32_t split, hipStream_t s, uint32_t *launches) {
    if (launches) *launches = 0;
    if (count == 0) return hipSuccess;
    if (!d_scalars || !d_points || !d_out || (scalar_stride != 0 && scalar_stride != 32)) return hipErrorInvalidValue;
    for (uint32_t off = 0; off < count; off += kX25519LaunchLanes) {
        const uint32_t n = count - off < kX25519LaunchLanes ? count - off : kX25519LaunchLanes;
        hipLaunchKernelGGL(x25519_ladder_kernel, dim3((n + 63) / 64), dim3(64), 0, s,
                           d_scalars + (uint64_t)scalar_stride * off, scalar_stride, d_points + 32ull * off, n,
                           d_out + 32ull * off, split > off ? split - off : 0u);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (launches) ++*launches;
    }
    return hipSuccess;
}

}  // namespace qgcm
