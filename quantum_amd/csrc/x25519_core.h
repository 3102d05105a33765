// x25519_core.h -- the arithmetic of a peer's shared secret, shared by host and device:
//   secret = X25519(scalar, u)                                   (crypto/ecdh.go:13-31, RFC 7748 s5)
// with the semantics of keymath.cpp's x25519 (curve25519.ScalarMult of the reference's vintage): the
// scalar is clamped, bit 255 of u is ignored, a non-canonical u is taken as it is (reduced mod p), and
// nothing is refused -- a small-order u gives the all-zero secret.
//
// Header-only and free of HIP includes, so a stand-alone host program can check it under the sanitizers
// (tools/x25519_core_check.cpp); x25519_kernels.hip compiles the same functions for gfx950, one ladder
// per lane.
//
// GF(2^255 - 19) elements are ten unsigned 32-bit limbs of 26, 25, 26, 25, ... bits (limb i starts at bit
// ceil(25.5 i)); products accumulate in 64 bits, which on gfx950 is one v_mad_u64_u32 per term.  Bounds:
//   reduced (what mul, sq, mul121665 and frombytes give):  even limbs < 2^26, odd limbs < 2^25 + 2^18
//   add of two reduced elements:                            even < 2^27,      odd < 2^26 + 2^19
//   sub of two reduced elements (f + 2p - g, no borrow):    even < 3 * 2^26,  odd < 3 * 2^25 + 2^18
// mul and sq take limbs up to 3 * 2^26 (even) and 3 * 2^25 + 2^19 (odd): a pre-multiplied operand 19 g
// stays below 2^32 (19 * 3 * 2^26 = 0.89 * 2^32), and a column of ten terms stays below 2^64 (column 0 is
// the largest: one plain product and four times 19 of two even limbs, five times 38 of two odd limbs, in
// all less than 124.5 * (3 * 2^26)^2 = 2^62.2).  The ladder only ever multiplies sums and differences of
// reduced elements, so add and sub need no carry.  mul and sq read their operands before they write the
// result, so the result may be one of the operands.
//
// Constant time: no branch, loop bound or memory index depends on a scalar bit or on a field value; the
// conditional swap is a mask, the scalar's bits come off the top of a shifted copy, and every loop below
// has a fixed trip count.  Every array index is a constant once the marked loops are unrolled, so on the
// device the limbs live in registers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QGCM_X_FN __host__ __device__ inline
#else
#define QGCM_X_FN inline
#endif
#if defined(__clang__)
#define QGCM_X_UNROLLED _Pragma("unroll")
#define QGCM_X_ROLLED _Pragma("nounroll")
#else
#define QGCM_X_UNROLLED
#define QGCM_X_ROLLED
#endif

namespace qgcm {

struct fe25519 {
    uint32_t v[10];
};

constexpr uint32_t kXMask26 = (1u << 26) - 1, kXMask25 = (1u << 25) - 1;
// bits of limb i and its first bit
QGCM_X_FN constexpr int x_bits(int i) { return (i & 1) ? 25 : 26; }
QGCM_X_FN constexpr int x_off(int i) { return 26 * ((i + 1) / 2) + 25 * (i / 2); }

QGCM_X_FN void fe_set_small(fe25519 &h, uint32_t x) {
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) h.v[i] = i ? 0 : x;
}

// h = f + g, no carry (operands reduced)
QGCM_X_FN void fe_add(fe25519 &h, const fe25519 &f, const fe25519 &g) {
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) h.v[i] = f.v[i] + g.v[i];
}

// h = f + 2p - g, no carry and no borrow (operands reduced: every limb of g is at most that of 2p)
QGCM_X_FN void fe_sub(fe25519 &h, const fe25519 &f, const fe25519 &g) {
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) {
        const uint32_t twop = i == 0 ? 2 * (kXMask26 - 18) : (i & 1) ? 2 * kXMask25 : 2 * kXMask26;
        h.v[i] = f.v[i] + twop - g.v[i];
    }
}

// ten 64-bit columns to a reduced element: one carry pass, the top carry times 19 into limb 0, and
// limb 0's carry into limb 1
QGCM_X_FN void fe_carry_columns(fe25519 &h, uint64_t c[10]) {
    QGCM_X_UNROLLED
    for (int i = 0; i < 9; ++i) {
        c[i + 1] += c[i] >> x_bits(i);
        h.v[i] = (uint32_t)c[i] & ((i & 1) ? kXMask25 : kXMask26);
    }
    const uint64_t t = (uint64_t)h.v[0] + 19 * (c[9] >> 25);  // c[9] >> 25 < 2^39
    h.v[9] = (uint32_t)c[9] & kXMask25;
    h.v[0] = (uint32_t)t & kXMask26;
    h.v[1] += (uint32_t)(t >> 26);  // < 2^18
}

// h = f g.  The term f_i g_j belongs to column (i + j) mod 10, times 19 when i + j >= 10 (2^255 = 19) and
// times 2 when i and j are both odd (their limbs start half a bit early).
QGCM_X_FN void fe_mul(fe25519 &h, const fe25519 &f, const fe25519 &g) {
    uint32_t f2[10], g19[10];
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) {
        f2[i] = 2 * f.v[i];
        g19[i] = 19 * g.v[i];
    }
    uint64_t c[10];
    QGCM_X_UNROLLED
    for (int k = 0; k < 10; ++k) {
        uint64_t acc = 0;
        QGCM_X_UNROLLED
        for (int i = 0; i < 10; ++i) {
            const int j = (k - i + 10) % 10;
            const uint32_t a = ((i & 1) && (j & 1)) ? f2[i] : f.v[i];
            const uint32_t b = i > k ? g19[j] : g.v[j];
            acc += (uint64_t)a * b;
        }
        c[k] = acc;
    }
    fe_carry_columns(h, c);
}

// h = f f: the terms i < j once, doubled
QGCM_X_FN void fe_sq(fe25519 &h, const fe25519 &f) {
    uint32_t f19[10];
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) f19[i] = 19 * f.v[i];
    uint64_t c[10];
    QGCM_X_UNROLLED
    for (int k = 0; k < 10; ++k) {
        uint64_t acc = 0;
        QGCM_X_UNROLLED
        for (int i = 0; i < 10; ++i) {
            const int j = (k - i + 10) % 10;
            if (i > j) continue;
            const int shift = (i != j ? 1 : 0) + (((i & 1) && (j & 1)) ? 1 : 0);
            const uint32_t b = i + j >= 10 ? f19[j] : f.v[j];
            acc += (uint64_t)(f.v[i] << shift) * b;  // 4 * 3 * 2^25 < 2^32
        }
        c[k] = acc;
    }
    fe_carry_columns(h, c);
}

// h = 121665 f  ((A - 2) / 4 of curve25519)
QGCM_X_FN void fe_mul121665(fe25519 &h, const fe25519 &f) {
    uint64_t c[10];
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) c[i] = (uint64_t)f.v[i] * 121665u;
    fe_carry_columns(h, c);
}

// swap f and g where mask is all ones, leave them where it is zero
QGCM_X_FN void fe_cswap(fe25519 &f, fe25519 &g, uint32_t mask) {
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) {
        const uint32_t t = mask & (f.v[i] ^ g.v[i]);
        f.v[i] ^= t;
        g.v[i] ^= t;
    }
}

// the low 255 bits of eight little-endian words; bit 255 is ignored (RFC 7748 s5), values of p and above
// are kept as they are
QGCM_X_FN void fe_frombytes(fe25519 &h, const uint32_t w[8]) {
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) {
        const int o = x_off(i), q = o >> 5, s = o & 31;
        const uint64_t pair = (uint64_t)w[q] | (q < 7 ? (uint64_t)w[q < 7 ? q + 1 : 7] << 32 : 0);
        h.v[i] = (uint32_t)(pair >> s) & ((i & 1) ? kXMask25 : kXMask26);
    }
}

// the canonical value (in [0, p)) of a reduced element or of a sum or difference of two, as eight words
QGCM_X_FN void fe_tobytes(uint32_t w[8], const fe25519 &f) {
    uint32_t h[10];
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) h[i] = f.v[i];
    // two carry passes leave every limb within its width: the first may wrap up to 19 * 2^7 into limb 0,
    // the second wraps only after a carry that rippled through nine full limbs, which leaves them zero
    QGCM_X_UNROLLED
    for (int pass = 0; pass < 2; ++pass) {
        QGCM_X_UNROLLED
        for (int i = 0; i < 9; ++i) {
            h[i + 1] += h[i] >> x_bits(i);
            h[i] &= (i & 1) ? kXMask25 : kXMask26;
        }
        h[0] += 19 * (h[9] >> 25);
        h[9] &= kXMask25;
    }
    // q = 1 exactly when h >= p: the carry out of bit 255 of h + 19
    uint32_t q = (h[0] + 19) >> 26;
    QGCM_X_UNROLLED
    for (int i = 1; i < 10; ++i) q = (h[i] + q) >> x_bits(i);
    // h - q p = h + 19 q - q 2^255
    h[0] += 19 * q;
    QGCM_X_UNROLLED
    for (int i = 0; i < 9; ++i) {
        h[i + 1] += h[i] >> x_bits(i);
        h[i] &= (i & 1) ? kXMask25 : kXMask26;
    }
    h[9] &= kXMask25;
    QGCM_X_UNROLLED
    for (int k = 0; k < 8; ++k) w[k] = 0;
    QGCM_X_UNROLLED
    for (int i = 0; i < 10; ++i) {
        const int o = x_off(i), q0 = o >> 5, s = o & 31;
        w[q0] |= h[i] << s;
        if (s + x_bits(i) > 32) w[q0 < 7 ? q0 + 1 : 7] |= h[i] >> (32 - s);
    }
}

// h = f^(2^n), n >= 1, in a rolled loop
QGCM_X_FN void fe_sq_times(fe25519 &h, const fe25519 &f, int n) {
    fe_sq(h, f);
    QGCM_X_ROLLED
    for (int i = 1; i < n; ++i) {
        const fe25519 t = h;
        fe_sq(h, t);
    }
}

// out = z^(p - 2) = z^(2^255 - 21) by the fixed addition chain (254 squarings, 11 multiplications);
// z = 0 gives 0
QGCM_X_FN void fe_invert(fe25519 &out, const fe25519 &z) {
    fe25519 t0, t1, t2, t3;
    fe_sq(t0, z);             // 2
    fe_sq_times(t1, t0, 2);   // 8
    fe_mul(t1, z, t1);        // 9
    fe_mul(t0, t0, t1);       // 11
    fe_sq(t2, t0);            // 22
    fe_mul(t1, t1, t2);       // 31 = 2^5 - 1
    fe_sq_times(t2, t1, 5);
    fe_mul(t1, t2, t1);       // 2^10 - 1
    fe_sq_times(t2, t1, 10);
    fe_mul(t2, t2, t1);       // 2^20 - 1
    fe_sq_times(t3, t2, 20);
    fe_mul(t2, t3, t2);       // 2^40 - 1
    fe_sq_times(t2, t2, 10);
    fe_mul(t1, t2, t1);       // 2^50 - 1
    fe_sq_times(t2, t1, 50);
    fe_mul(t2, t2, t1);       // 2^100 - 1
    fe_sq_times(t3, t2, 100);
    fe_mul(t2, t3, t2);       // 2^200 - 1
    fe_sq_times(t2, t2, 50);
    fe_mul(t1, t2, t1);       // 2^250 - 1
    fe_sq_times(t1, t1, 5);
    fe_mul(out, t1, t0);      // 2^255 - 32 + 11
}

// out = X25519(scalar, u), all three as eight little-endian words (RFC 7748 s5: the Montgomery ladder on
// x-only coordinates, with keymath.cpp's step formulas)
QGCM_X_FN void x25519_words(uint32_t out[8], const uint32_t scalar[8], const uint32_t u[8]) {
    uint32_t k[8];
    QGCM_X_UNROLLED
    for (int i = 0; i < 8; ++i) k[i] = scalar[i];
    k[0] &= ~7u;
    k[7] = (k[7] & 0x7fffffffu) | 0x40000000u;
    // bit 254 to the top: each step takes the top bit and shifts the scalar up by one
    QGCM_X_UNROLLED
    for (int i = 7; i > 0; --i) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
    k[0] <<= 1;
    fe25519 x1, x2, z2, x3, z3;
    fe_frombytes(x1, u);
    fe_set_small(x2, 1);
    fe_set_small(z2, 0);
    x3 = x1;
    fe_set_small(z3, 1);
    uint32_t swap = 0;
    QGCM_X_ROLLED
    for (int t = 254; t >= 0; --t) {
        const uint32_t kt = 0u - (k[7] >> 31);
        QGCM_X_UNROLLED
        for (int i = 7; i > 0; --i) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
        k[0] <<= 1;
        swap ^= kt;
        fe_cswap(x2, x3, swap);
        fe_cswap(z2, z3, swap);
        swap = kt;
        fe25519 a, aa, b, bb, e, c, d, da, cb, t0, t1;
        fe_add(a, x2, z2);
        fe_sq(aa, a);
        fe_sub(b, x2, z2);
        fe_sq(bb, b);
        fe_sub(e, aa, bb);
        fe_add(c, x3, z3);
        fe_sub(d, x3, z3);
        fe_mul(da, d, a);
        fe_mul(cb, c, b);
        fe_add(t0, da, cb);
        fe_sq(x3, t0);
        fe_sub(t1, da, cb);
        fe_sq(t0, t1);
        fe_mul(z3, x1, t0);
        fe_mul(x2, aa, bb);
        fe_mul121665(t0, e);
        fe_add(t1, aa, t0);
        fe_mul(z2, e, t1);
    }
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    fe25519 zi, r;
    fe_invert(zi, z2);
    fe_mul(r, x2, zi);
    fe_tobytes(out, r);
}

// the same on byte strings (host callers; the kernel loads and stores words)
QGCM_X_FN void x25519_bytes(uint8_t out[32], const uint8_t scalar[32], const uint8_t u[32]) {
    uint32_t k[8], p[8], r[8];
    for (int i = 0; i < 8; ++i) {
        k[i] = (uint32_t)scalar[4 * i] | (uint32_t)scalar[4 * i + 1] << 8 | (uint32_t)scalar[4 * i + 2] << 16 |
               (uint32_t)scalar[4 * i + 3] << 24;
        p[i] = (uint32_t)u[4 * i] | (uint32_t)u[4 * i + 1] << 8 | (uint32_t)u[4 * i + 2] << 16 | (uint32_t)u[4 * i + 3] << 24;
    }
    x25519_words(r, k, p);
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(r[i] >> (8 * j));
}

}  // namespace qgcm
