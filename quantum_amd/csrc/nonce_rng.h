// The nonce generator's host state (qgcm_nonce_fill, QGCM_NONCES_GENERATE): an AES-256-CTR stream whose
// blocks are computed on the GPU (gcm_kernels.hip nonce_kernel) and whose key and counter live here.
// Header-only and free of HIP, so a stand-alone host program can sweep the key expansion, the counter
// arithmetic and the reseed rule under the sanitizers (tools/nonce_rng_check.cpp).
//
// Construction (SP 800-38A 6.5, counter mode): a context holds a key K (32 B) and a 128-bit counter V.
// Nonce number j of the stream is the first 12 bytes of AES-256_K(BE128(V0 + j)), the counter a
// big-endian 128-bit integer that carries through all 16 bytes and wraps at 2^128.  A call that needs
// n nonces reserves [V, V + n) under the generator's mutex and takes a copy of the round keys with it
// (a NonceLease), so a later reseed never changes what a launch in flight computes.
// Reseed rule: before reserving, when at least one nonce was drawn since the last (re)seed and that
// count plus n exceeds the interval (QGCM_NONCE_RESEED, default 2^32), K and V are drawn anew from the
// entropy source (getrandom) first; one call always uses one key.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <mutex>

namespace qgcm {

// Round keys in the layout Keys{rk, rr} of the kernels: rk[i] = FIPS-197 word i as an LE column word
// (byte 4 i of the schedule in bits 0..7), rr[i] = rot16(rk[i]).  480 B: travels in the kernel arguments.
struct NonceKeys {
    uint32_t rk[60];
    uint32_t rr[60];
};

// 128-bit counter as four 32-bit limbs, v[0] least significant; BE128(v) = the 16 bytes of the block.
inline void ctr128_from_be(const uint8_t be[16], uint32_t v[4]) {
    for (int i = 0; i < 4; ++i) {
        const uint8_t *p = be + 12 - 4 * i;
        v[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
    }
}
inline void ctr128_to_be(const uint32_t v[4], uint8_t be[16]) {
    for (int i = 0; i < 4; ++i) {
        uint8_t *p = be + 12 - 4 * i;
        p[0] = (uint8_t)(v[i] >> 24);
        p[1] = (uint8_t)(v[i] >> 16);
        p[2] = (uint8_t)(v[i] >> 8);
        p[3] = (uint8_t)v[i];
    }
}
// v += n mod 2^128
inline void ctr128_add(uint32_t v[4], uint64_t n) {
    const uint64_t lo = (uint64_t)v[0] | (uint64_t)v[1] << 32;
    uint64_t hi = (uint64_t)v[2] | (uint64_t)v[3] << 32;
    const uint64_t s = lo + n;
    hi += s < lo ? 1u : 0u;
    v[0] = (uint32_t)s;
    v[1] = (uint32_t)(s >> 32);
    v[2] = (uint32_t)hi;
    v[3] = (uint32_t)(hi >> 32);
}

namespace nonce_detail {
inline uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
// FIPS-197 S-box: affine map of the inverse in GF(2^8), generated (3 is a generator, 0xf6 its inverse)
inline const uint8_t *sbox() {
    static const struct Table {
        uint8_t s[256];
        Table() {
            uint8_t p = 1, q = 1;
            do {
                p = (uint8_t)(p ^ xtime(p));  // p *= 3
                q ^= (uint8_t)(q << 1);       // q /= 3
                q ^= (uint8_t)(q << 2);
                q ^= (uint8_t)(q << 4);
                if (q & 0x80) q ^= 0x09;
                const uint8_t x = (uint8_t)(q ^ (q << 1 | q >> 7) ^ (q << 2 | q >> 6) ^ (q << 3 | q >> 5) ^ (q << 4 | q >> 4));
                s[p] = (uint8_t)(x ^ 0x63);
            } while (p != 1);
            s[0] = 0x63;
        }
    } t;
    return t.s;
}
}  // namespace nonce_detail

// FIPS-197 5.2 key expansion, Nk = 8: 240 schedule bytes
inline void aes256_schedule(const uint8_t key[32], uint8_t out[240]) {
    const uint8_t *sb = nonce_detail::sbox();
    memcpy(out, key, 32);
    uint8_t rcon = 1;
    for (int i = 8; i < 60; ++i) {
        uint8_t t[4] = {out[4 * i - 4], out[4 * i - 3], out[4 * i - 2], out[4 * i - 1]};
        if (i % 8 == 0) {
            const uint8_t t0 = t[0];
            t[0] = (uint8_t)(sb[t[1]] ^ rcon);
            t[1] = sb[t[2]];
            t[2] = sb[t[3]];
            t[3] = sb[t0];
            rcon = nonce_detail::xtime(rcon);
        } else if (i % 8 == 4) {
            for (int j = 0; j < 4; ++j) t[j] = sb[t[j]];
        }
        for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(out[4 * i - 32 + j] ^ t[j]);
    }
}
inline void nonce_expand_key(const uint8_t key[32], NonceKeys &k) {
    uint8_t b[240];
    aes256_schedule(key, b);
    for (int i = 0; i < 60; ++i) {
        const uint32_t w = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
                           (uint32_t)b[4 * i + 3] << 24;
        k.rk[i] = w;
        k.rr[i] = (w << 16) | (w >> 16);
    }
}

// What a call takes away from a reservation: the round keys and the counter of its first nonce.
struct NonceLease {
    NonceKeys keys;
    uint32_t v[4];
};
// the lease of a call's packets [first, ...): same key, counter advanced
inline NonceLease lease_at(const NonceLease &l, uint64_t first) {
    NonceLease r = l;
    ctr128_add(r.v, first);
    return r;
}

// fills buf with n bytes of entropy; false on failure
typedef bool (*NonceEntropy)(void *buf, size_t n);
inline bool nonce_getrandom(void *buf, size_t n) {
    uint8_t *p = static_cast<uint8_t *>(buf);
    while (n) {
        const ssize_t r = getrandom(p, n, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        p += r;
        n -= (size_t)r;
    }
    return true;
}

constexpr uint64_t kNonceReseedDefault = 1ull << 32;

class NonceRng {
  public:
    explicit NonceRng(NonceEntropy e = nonce_getrandom, uint64_t interval = kNonceReseedDefault)
        : entropy_(e), interval_(interval ? interval : 1) {}
    // before the first reservation only (qgcm_create)
    void set_interval(uint64_t interval) { interval_ = interval ? interval : 1; }
    uint64_t interval() const { return interval_; }
    // K and V set explicitly (known answers, reproducible runs), or both drawn from the entropy source
    // when key is NULL; restarts the reseed count either way
    bool seed(const uint8_t key[32], const uint8_t counter[16]) {
        std::lock_guard<std::mutex> g(mu_);
        if (!key) return draw();
        nonce_expand_key(key, keys_);
        ctr128_from_be(counter, v_);
        since_ = 0;
        seeded_ = true;
        return true;
    }
    // reserves stream positions [V, V + n) for one call; false when the entropy source failed (nothing
    // is reserved then)
    bool reserve(uint64_t n, NonceLease &out) {
        std::lock_guard<std::mutex> g(mu_);
        if (!seeded_ || (since_ > 0 && (since_ + n < since_ || since_ + n > interval_))) {
            if (!draw()) return false;
        }
        out.keys = keys_;
        memcpy(out.v, v_, sizeof v_);
        ctr128_add(v_, n);
        since_ += n;
        return true;
    }
    // (tests) draws from the entropy source so far, nonces reserved since the last of them or seed()
    uint64_t draws() const { return draws_; }
    uint64_t since_seed() const { return since_; }

  private:
    bool draw() {
        uint8_t kv[48];
        if (!entropy_(kv, sizeof kv)) return false;
        nonce_expand_key(kv, keys_);
        ctr128_from_be(kv + 32, v_);
        volatile uint8_t *w = kv;  // the key does not stay on the stack
        for (size_t i = 0; i < sizeof kv; ++i) w[i] = 0;
        since_ = 0;
        seeded_ = true;
        ++draws_;
        return true;
    }
    std::mutex mu_;
    NonceEntropy entropy_;
    uint64_t interval_;
    NonceKeys keys_{};
    uint32_t v_[4] = {};
    uint64_t since_ = 0, draws_ = 0;
    bool seeded_ = false;
};

}  // namespace qgcm
