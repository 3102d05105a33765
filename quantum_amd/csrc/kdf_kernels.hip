// kdf_kernels.hip -- peer keys derived on the GPU: PBKDF2-HMAC-SHA512(secret, salt, iters, 32) for
// 32-byte secrets and salts (kdf_core.h), one key per lane.
//
// A key is a serial chain of 2 * iters SHA-512 compressions on 64-bit words with no memory traffic, so
// the kernel is pure VALU work in registers: no LDS, no scratch.  The key states and U1 come from
// kdf_core.h as the host computes them (four generic compressions); the loop's two compressions per
// iteration are written out here for the one block shape they see -- an 8-word digest, then the fixed
// padding W[8] = 2^63, W[9..14] = 0, W[15] = 1536:
//   * rounds 0..31 are straight-line code in which the padding words are constants: K[t] + W[t] of rounds
//     8..15 is one literal, and the schedule steps 16..30 lose the terms that are zero or constant;
//   * rounds 32..79 are three passes of one 16-round body whose K comes by scalar loads from the constant
//     table (a uniform index), so the loop body stays a few KiB of code;
//   * a 64-bit rotate is two v_alignbit_b32 on the halves (halves swapped first for 32 or more), a shift
//     one v_alignbit_b32 and one v_lshrrev_b32; Ch and Maj are v_bfi_b32 per half (Maj(a, b, c) =
//     bfi(a ^ b, c, b)); the adds stay 64-bit (v_lshl_add_u64).  gfx950 has no three-input xor
//     (v_xor3_b32 is refused by its assembler), so a sigma costs two v_xor_b32 per half.
#include <hip/hip_runtime.h>

#include "gcm_internal.h"
#include "kdf_core.h"

namespace qgcm {

namespace {

// constant address space: a compile-time index folds to a literal, a uniform run-time index is a scalar load
constexpr uint64_t kKdfK[80] = {QGCM_KDF_SHA512_K};

__device__ __forceinline__ uint32_t lo32(uint64_t x) { return (uint32_t)x; }
__device__ __forceinline__ uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
// a register pair, not arithmetic: (uint64_t)hi << 32 | lo invites the compiler to fold the shift into the
// next 64-bit add and to add the low half separately
typedef uint32_t kdf_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint64_t pack64(uint32_t lo, uint32_t hi) {
    return __builtin_bit_cast(uint64_t, kdf_u32x2{lo, hi});
}
// low 32 bits of {hi:lo} >> s, s in [0, 32)
__device__ __forceinline__ uint32_t align32(uint32_t hi, uint32_t lo, uint32_t s) {
    return __builtin_amdgcn_alignbit(hi, lo, s);
}
// (sel & one) | (~sel & zero); as an instruction, because the compiler rewrites the C form of Maj into
// two ands, an xor and an or
__device__ __forceinline__ uint32_t bfi32(uint32_t sel, uint32_t one, uint32_t zero) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(sel), "v"(one), "v"(zero));
    return r;
}

// the halves of x rotated right by N: lo, hi
template <int N>
__device__ __forceinline__ uint32_t ror_lo(uint32_t l, uint32_t h) {
    if constexpr (N < 32) return align32(h, l, N);
    else if constexpr (N == 32) return h;
    else return align32(l, h, N - 32);
}
template <int N>
__device__ __forceinline__ uint32_t ror_hi(uint32_t l, uint32_t h) {
    if constexpr (N < 32) return align32(l, h, N);
    else if constexpr (N == 32) return l;
    else return align32(h, l, N - 32);
}

// ror(x, A) ^ ror(x, B) ^ ror(x, C)
template <int A, int B, int C>
__device__ __forceinline__ uint64_t big_sigma(uint64_t x) {
    const uint32_t l = lo32(x), h = hi32(x);
    return pack64(ror_lo<A>(l, h) ^ ror_lo<B>(l, h) ^ ror_lo<C>(l, h), ror_hi<A>(l, h) ^ ror_hi<B>(l, h) ^ ror_hi<C>(l, h));
}
// ror(x, A) ^ ror(x, B) ^ (x >> S), S < 32
template <int A, int B, int S>
__device__ __forceinline__ uint64_t small_sigma(uint64_t x) {
    const uint32_t l = lo32(x), h = hi32(x);
    return pack64(ror_lo<A>(l, h) ^ ror_lo<B>(l, h) ^ align32(h, l, S), ror_hi<A>(l, h) ^ ror_hi<B>(l, h) ^ (h >> S));
}
__device__ __forceinline__ uint64_t ch64(uint64_t e, uint64_t f, uint64_t g) {
    return pack64(bfi32(lo32(e), lo32(f), lo32(g)), bfi32(hi32(e), hi32(f), hi32(g)));
}
__device__ __forceinline__ uint64_t maj64(uint64_t a, uint64_t b, uint64_t c) {
    const uint64_t x = a ^ b;
    return pack64(bfi32(lo32(x), lo32(c), lo32(b)), bfi32(hi32(x), hi32(c), hi32(b)));
}

#define KDF_ROUND(a, b, c, d, e, f, g, h, kw)                        \
    h += big_sigma<14, 18, 41>(e) + ch64(e, f, g) + (kw);            \
    d += h;                                                          \
    h += big_sigma<28, 34, 39>(a) + maj64(a, b, c);
// word t of the schedule into w[t & 15] (t >= 16; i = t & 15)
#define KDF_SCHED(i) \
    (w[i] += small_sigma<1, 8, 7>(w[((i) + 1) & 15]) + w[((i) + 9) & 15] + small_sigma<19, 61, 6>(w[((i) + 14) & 15]))
#define KDF_16_ROUNDS(KW)                                                                             \
    KDF_ROUND(a, b, c, d, e, f, g, h, KW(0)) KDF_ROUND(h, a, b, c, d, e, f, g, KW(1))                 \
    KDF_ROUND(g, h, a, b, c, d, e, f, KW(2)) KDF_ROUND(f, g, h, a, b, c, d, e, KW(3))                 \
    KDF_ROUND(e, f, g, h, a, b, c, d, KW(4)) KDF_ROUND(d, e, f, g, h, a, b, c, KW(5))                 \
    KDF_ROUND(c, d, e, f, g, h, a, b, KW(6)) KDF_ROUND(b, c, d, e, f, g, h, a, KW(7))                 \
    KDF_ROUND(a, b, c, d, e, f, g, h, KW(8)) KDF_ROUND(h, a, b, c, d, e, f, g, KW(9))                 \
    KDF_ROUND(g, h, a, b, c, d, e, f, KW(10)) KDF_ROUND(f, g, h, a, b, c, d, e, KW(11))               \
    KDF_ROUND(e, f, g, h, a, b, c, d, KW(12)) KDF_ROUND(d, e, f, g, h, a, b, c, KW(13))               \
    KDF_ROUND(c, d, e, f, g, h, a, b, KW(14)) KDF_ROUND(b, c, d, e, f, g, h, a, KW(15))

// out = init + F(init, m || 80 00.. || 1536) for the 64-byte message m = w[0..8).  w[8..16) is set here.
__device__ __forceinline__ void compress_digest_block(const uint64_t init[8], uint64_t w[16], uint64_t out[8]) {
    uint64_t a = init[0], b = init[1], c = init[2], d = init[3], e = init[4], f = init[5], g = init[6], h = init[7];
    // the padding as constants: the compiler folds them through rounds 8..15 and schedule steps 16..30
    w[8] = kKdfPad80;
    w[9] = w[10] = w[11] = w[12] = w[13] = w[14] = 0;
    w[15] = kKdfLenDigest;
#define KDF_KW_FIRST(i) (kKdfK[i] + w[i])
    KDF_16_ROUNDS(KDF_KW_FIRST)
#define KDF_KW_SECOND(i) (KDF_SCHED(i), kKdfK[16 + (i)] + w[i])
    KDF_16_ROUNDS(KDF_KW_SECOND)
#pragma nounroll
    for (int p = 32; p < 80; p += 16) {
#define KDF_KW_LOOP(i) (KDF_SCHED(i), kKdfK[p + (i)] + w[i])
        KDF_16_ROUNDS(KDF_KW_LOOP)
    }
    out[0] = init[0] + a; out[1] = init[1] + b; out[2] = init[2] + c; out[3] = init[3] + d;
    out[4] = init[4] + e; out[5] = init[5] + f; out[6] = init[6] + g; out[7] = init[7] + h;
}

__device__ __forceinline__ uint64_t load_be64(const uint32_t *p) {
    return pack64(__builtin_bswap32(p[1]), __builtin_bswap32(p[0]));
}

// keys[i] = PBKDF2-HMAC-SHA512(secrets[i], salts[i], iters, 32): 32 B each, 4-B aligned; iters >= 1.
__global__ void __launch_bounds__(64) kdf_pbkdf2_kernel(const uint8_t *secrets, const uint8_t *salts, uint32_t count,
                                                        uint32_t iters, uint8_t *keys) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= count) return;  // before any load
    const uint32_t *ps = (const uint32_t *)(secrets + 32ull * i);
    const uint32_t *pc = (const uint32_t *)(salts + 32ull * i);
    uint64_t secret[4], salt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        secret[k] = load_be64(ps + 2 * k);
        salt[k] = load_be64(pc + 2 * k);
    }
    uint64_t ipad[8], opad[8], u[8], t[4];
    kdf_pads(secret, ipad, opad, kKdfK);
    kdf_u1(ipad, opad, salt, u, kKdfK);
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = u[k];
#pragma nounroll
    for (uint32_t it = 1; it < iters; ++it) {
        uint64_t w[16], dg[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = u[k];
        compress_digest_block(ipad, w, dg);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = dg[k];
        compress_digest_block(opad, w, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] ^= u[k];
    }
    uint32_t *pk = (uint32_t *)(keys + 32ull * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pk[2 * k] = __builtin_bswap32(hi32(t[k]));
        pk[2 * k + 1] = __builtin_bswap32(lo32(t[k]));
    }
}

}  // namespace

hipError_t launch_kdf(const uint8_t *d_secrets, const uint8_t *d_salts, uint32_t count, uint32_t iters, uint8_t *d_keys,
                      hipStream_t s, uint32_t *launches) {
    if (launches) *launches = 0;
    if (count == 0) return hipSuccess;
    if (!d_secrets || !d_salts || !d_keys || iters == 0 || iters > kKdfMaxIters) return hipErrorInvalidValue;
    for (uint32_t off = 0; off < count; off += kKdfLaunchKeys) {
        const uint32_t n = count - off < kKdfLaunchKeys ? count - off : kKdfLaunchKeys;
        hipLaunchKernelGGL(kdf_pbkdf2_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_secrets + 32ull * off,
                           d_salts + 32ull * off, n, iters, d_keys + 32ull * off);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (launches) ++*launches;
    }
    return hipSuccess;
}

}  // namespace qgcm
