// kdf_core.h -- the arithmetic of a peer key, shared by host and device:
//   key = PBKDF2-HMAC-SHA512(secret, salt, iters, 32)           (crypto/aes.go:66, iters = 10000)
// for the one shape common/mapping.go:90-99 produces: a 32-byte secret and a 32-byte salt (two X25519
// outputs).  From FIPS 180-4 (SHA-512), RFC 2104 (HMAC) and RFC 8018 s5.2 (PBKDF2).
//
// Header-only and free of HIP includes, so a stand-alone host program can check it under the sanitizers
// (tools/kdf_core_check.cpp); kdf_kernels.hip compiles the same functions for gfx950 and replaces only
// the loop's two compressions by its hand-written form.  The shape is fixed, so there is no buffering
// and no variable-length path:
//   ipad / opad states: one compression each of (secret || 0^96) xor 0x36.. / 0x5c..
//   U1   = HMAC(salt || 00000001): inner block 2 = salt || 00000001 || 80 || 0.. || len (128 + 36) * 8,
//          outer block 2 = digest || 80 || 0.. || len (128 + 64) * 8
//   Uk+1 = HMAC(Uk): both blocks are digest || 80 || 0.. || len (128 + 64) * 8
//   T    = U1 xor ... xor Uiters; the key is the first 32 bytes of T, big-endian words.
// Words are the 64-bit big-endian words of FIPS 180-4 throughout; bytes appear only at the two ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QGCM_KDF_FN __host__ __device__ inline
#else
#define QGCM_KDF_FN inline
#endif
#if defined(__clang__)
#define QGCM_KDF_UNROLLED _Pragma("unroll")
#define QGCM_KDF_ROLLED _Pragma("nounroll")
#else
#define QGCM_KDF_UNROLLED
#define QGCM_KDF_ROLLED
#endif

namespace qgcm {

// SHA-512 round constants and initial value (FIPS 180-4 s4.2.3, s5.3.5).  Each side declares its own table
// from this list (the kernel in constant memory, where a uniform index is a scalar load) and passes it in.
#define QGCM_KDF_SHA512_K                                                                               \
    0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL,         \
    0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL,         \
    0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,         \
    0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL,         \
    0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,         \
    0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,         \
    0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL,         \
    0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL, 0x06ca6351e003826fULL, 0x142929670a0e6e70ULL,         \
    0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,         \
    0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,         \
    0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL,         \
    0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,         \
    0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL,         \
    0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL,         \
    0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,         \
    0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL,         \
    0xca273eceea26619cULL, 0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL,         \
    0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,         \
    0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL,         \
    0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL

constexpr uint64_t kKdfPad80 = 0x8000000000000000ULL;    // the 0x80 byte behind a message that ends on a word
constexpr uint64_t kKdfLenU1 = (128 + 36) * 8;           // bits hashed by the inner HMAC pass of U1
constexpr uint64_t kKdfLenDigest = (128 + 64) * 8;       // bits hashed by every other second block (1536)
constexpr uint32_t kKdfMaxIters = 1u << 20;

QGCM_KDF_FN uint64_t kdf_ror(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

QGCM_KDF_FN void kdf_h0(uint64_t h[8]) {
    h[0] = 0x6a09e667f3bcc908ULL; h[1] = 0xbb67ae8584caa73bULL; h[2] = 0x3c6ef372fe94f82bULL;
    h[3] = 0xa54ff53a5f1d36f1ULL; h[4] = 0x510e527fade682d1ULL; h[5] = 0x9b05688c2b3e6c1fULL;
    h[6] = 0x1f83d9abfb41bd6bULL; h[7] = 0x5be0cd19137e2179ULL;
}

// Rounds [p, p + 16) of a compression; the schedule rolls through w: word t lives in w[t & 15].  Inside a pass every index into w and v is a constant once the pass is unrolled, so
// on the device both arrays stay in registers.
template <bool kSchedule>
QGCM_KDF_FN void kdf_pass(uint64_t v[8], uint64_t w[16], const uint64_t *K, int p) {
    QGCM_KDF_UNROLLED
    for (int r = 0; r < 16; ++r) {
        if (kSchedule) {
            const uint64_t w15 = w[(r + 1) & 15], w2 = w[(r + 14) & 15];
            const uint64_t s0 = kdf_ror(w15, 1) ^ kdf_ror(w15, 8) ^ (w15 >> 7);
            const uint64_t s1 = kdf_ror(w2, 19) ^ kdf_ror(w2, 61) ^ (w2 >> 6);
            w[r] += s0 + w[(r + 9) & 15] + s1;
        }
        const uint64_t a = v[0], b = v[1], c = v[2], e = v[4], f = v[5], g = v[6];
        const uint64_t S1 = kdf_ror(e, 14) ^ kdf_ror(e, 18) ^ kdf_ror(e, 41);
        const uint64_t ch = (e & f) ^ (~e & g);
        const uint64_t t1 = v[7] + S1 + ch + K[p + r] + w[r];
        const uint64_t S0 = kdf_ror(a, 28) ^ kdf_ror(a, 34) ^ kdf_ror(a, 39);
        const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
        v[7] = g; v[6] = f; v[5] = e; v[4] = v[3] + t1; v[3] = c; v[2] = b; v[1] = a; v[0] = t1 + S0 + mj;
    }
}

// One SHA-512 compression: st += F(st, w).  w is the block's 16 words and is overwritten.
QGCM_KDF_FN void kdf_compress(uint64_t st[8], uint64_t w[16], const uint64_t *K) {
    uint64_t v[8];
    for (int i = 0; i < 8; ++i) v[i] = st[i];
    kdf_pass<false>(v, w, K, 0);
    QGCM_KDF_ROLLED
    for (int p = 16; p < 80; p += 16) kdf_pass<true>(v, w, K, p);
    for (int i = 0; i < 8; ++i) st[i] += v[i];
}

// big-endian word i of a 32-byte string
QGCM_KDF_FN uint64_t kdf_load_be64(const uint8_t *p) {
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v = (v << 8) | p[j];
    return v;
}

// HMAC key states of a 32-byte secret (4 words): ipad = F(H0, (secret || 0) ^ 0x36..), opad likewise 0x5c.
QGCM_KDF_FN void kdf_pads(const uint64_t secret[4], uint64_t ipad[8], uint64_t opad[8], const uint64_t *K) {
    uint64_t w[16];
    for (int i = 0; i < 16; ++i) w[i] = (i < 4 ? secret[i] : 0) ^ 0x3636363636363636ULL;
    kdf_h0(ipad);
    kdf_compress(ipad, w, K);
    for (int i = 0; i < 16; ++i) w[i] = (i < 4 ? secret[i] : 0) ^ 0x5c5c5c5c5c5c5c5cULL;
    kdf_h0(opad);
    kdf_compress(opad, w, K);
}

// u = F(opad, F(ipad, block) || pad): the second half of every HMAC here.  `w` holds the inner block.
QGCM_KDF_FN void kdf_hmac_tail(const uint64_t ipad[8], const uint64_t opad[8], uint64_t w[16], uint64_t u[8],
                               const uint64_t *K) {
    uint64_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = ipad[i];
    kdf_compress(st, w, K);
    for (int i = 0; i < 8; ++i) w[i] = st[i];
    w[8] = kKdfPad80;
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = kKdfLenDigest;
    for (int i = 0; i < 8; ++i) u[i] = opad[i];
    kdf_compress(u, w, K);
}

// U1 = HMAC(secret, salt || 00000001) from the key states; salt as 4 words.
QGCM_KDF_FN void kdf_u1(const uint64_t ipad[8], const uint64_t opad[8], const uint64_t salt[4], uint64_t u[8],
                        const uint64_t *K) {
    uint64_t w[16];
    for (int i = 0; i < 4; ++i) w[i] = salt[i];
    w[4] = 0x0000000180000000ULL;  // block index 1, then the 0x80 pad byte
    for (int i = 5; i < 15; ++i) w[i] = 0;
    w[15] = kKdfLenU1;
    kdf_hmac_tail(ipad, opad, w, u, K);
}

// Uk+1 = HMAC(secret, Uk) in place: two compressions on one padded 64-byte block each.
QGCM_KDF_FN void kdf_next(const uint64_t ipad[8], const uint64_t opad[8], uint64_t u[8], const uint64_t *K) {
    uint64_t w[16];
    for (int i = 0; i < 8; ++i) w[i] = u[i];
    w[8] = kKdfPad80;
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = kKdfLenDigest;
    kdf_hmac_tail(ipad, opad, w, u, K);
}

// The whole derivation, words in and out: t[0..4) are the key's four big-endian words.  iters >= 1.
QGCM_KDF_FN void kdf_pbkdf2_words(const uint64_t secret[4], const uint64_t salt[4], uint32_t iters, uint64_t t[4],
                                  const uint64_t *K) {
    uint64_t ipad[8], opad[8], u[8];
    kdf_pads(secret, ipad, opad, K);
    kdf_u1(ipad, opad, salt, u, K);
    for (int i = 0; i < 4; ++i) t[i] = u[i];
    for (uint32_t k = 1; k < iters; ++k) {
        kdf_next(ipad, opad, u, K);
        for (int i = 0; i < 4; ++i) t[i] ^= u[i];
    }
}

// Bytes in and out (32-byte secret, 32-byte salt, 32-byte key).
QGCM_KDF_FN void kdf_pbkdf2_32(const uint8_t secret[32], const uint8_t salt[32], uint32_t iters, uint8_t key[32],
                               const uint64_t *K) {
    uint64_t s[4], c[4], t[4];
    for (int i = 0; i < 4; ++i) {
        s[i] = kdf_load_be64(secret + 8 * i);
        c[i] = kdf_load_be64(salt + 8 * i);
    }
    kdf_pbkdf2_words(s, c, iters, t, K);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 8; ++j) key[8 * i + j] = (uint8_t)(t[i] >> (56 - 8 * j));
}

}  // namespace qgcm
