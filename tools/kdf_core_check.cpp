// Checks the peer-key arithmetic shared by host and device (quantum_amd/csrc/kdf_core.h): the SHA-512
// compression on its rolling schedule and the fixed-shape PBKDF2-HMAC-SHA512 for a 32-byte secret and a
// 32-byte salt.  Stand-alone host program with no HIP, meant for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/kdf_core_check.cpp -o kdf_core_check && ./kdf_core_check [vector file]
// The vector file holds lines of `secret salt iters expected` (hex, hex, decimal, hex; 32-byte secret and
// salt, 32-byte key; blank lines and lines starting with # are skipped); each is derived and compared.
// Then it sweeps edge inputs by itself -- all-00 and all-ff secrets and salts, every single-bit secret
// and salt, at 1, 2 and 3 iterations, the all-00 / all-ff pairs at 10000 too -- against a byte-wise PBKDF2
// written below from FIPS 180-4, RFC 2104 and RFC 8018 with none of the header's shortcuts (buffered
// updates, a full 80-word schedule, padding built byte by byte).  It ends with
// "kdf_core_check: <checks> checks, <failures> failures" and exits 1 if any failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../quantum_amd/csrc/kdf_core.h"

using namespace qgcm;

static const uint64_t kK[80] = {QGCM_KDF_SHA512_K};

static int checks = 0, failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        ++checks;                        \
        if (!(cond)) {                   \
            ++failures;                  \
            printf("FAIL %s: ", #cond);  \
            printf(__VA_ARGS__);         \
            printf("\n");                \
        }                                \
    } while (0)

static std::string hex(const uint8_t *p, size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

static bool unhex(const std::string &s, std::vector<uint8_t> &out) {
    if (s.size() % 2) return false;
    out.clear();
    for (size_t i = 0; i < s.size(); i += 2) {
        int v = 0;
        for (int k = 0; k < 2; ++k) {
            const char c = s[i + k];
            int d;
            if (c >= '0' && c <= '9') d = c - '0';
            else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
            else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
            else return false;
            v = v * 16 + d;
        }
        out.push_back((uint8_t)v);
    }
    return true;
}

// ---- byte-wise reference ----
namespace ref {

struct Sha512 {
    uint64_t h[8];
    std::vector<uint8_t> buf;
    uint64_t total = 0;
    Sha512() { kdf_h0(h); }
    static uint64_t rotr(uint64_t x, unsigned n) { return (x >> n) | (x << (64 - n)); }
    void block(const uint8_t *p) {
        uint64_t w[80];
        for (int i = 0; i < 16; ++i) {
            w[i] = 0;
            for (int j = 0; j < 8; ++j) w[i] = (w[i] << 8) | p[8 * i + j];
        }
        for (int i = 16; i < 80; ++i)
            w[i] = w[i - 16] + (rotr(w[i - 15], 1) ^ rotr(w[i - 15], 8) ^ (w[i - 15] >> 7)) + w[i - 7] +
                   (rotr(w[i - 2], 19) ^ rotr(w[i - 2], 61) ^ (w[i - 2] >> 6));
        uint64_t v[8];
        memcpy(v, h, sizeof v);
        for (int i = 0; i < 80; ++i) {
            const uint64_t t1 = v[7] + (rotr(v[4], 14) ^ rotr(v[4], 18) ^ rotr(v[4], 41)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) +
                                kK[i] + w[i];
            const uint64_t t2 = (rotr(v[0], 28) ^ rotr(v[0], 34) ^ rotr(v[0], 39)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
            for (int k = 7; k > 0; --k) v[k] = v[k - 1];
            v[4] += t1;
            v[0] = t1 + t2;
        }
        for (int i = 0; i < 8; ++i) h[i] += v[i];
    }
    void update(const uint8_t *p, size_t n) {
        total += n;
        buf.insert(buf.end(), p, p + n);
        size_t off = 0;
        for (; buf.size() - off >= 128; off += 128) block(buf.data() + off);
        buf.erase(buf.begin(), buf.begin() + (long)off);
    }
    void final(uint8_t out[64]) {
        const uint64_t bits = total * 8;
        std::vector<uint8_t> pad(1, 0x80);
        while ((buf.size() + pad.size()) % 128 != 112) pad.push_back(0);
        for (int j = 15; j >= 0; --j) pad.push_back(j < 8 ? (uint8_t)(bits >> (8 * j)) : 0);
        update(pad.data(), pad.size());
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(h[i] >> (56 - 8 * j));
    }
};

static void hmac(const uint8_t *key, size_t klen, const uint8_t *m, size_t n, uint8_t out[64]) {
    uint8_t k[128] = {0}, pad[128], inner[64];
    memcpy(k, key, klen);  // klen <= 128 here
    Sha512 in, ou;
    for (int i = 0; i < 128; ++i) pad[i] = k[i] ^ 0x36;
    in.update(pad, 128);
    in.update(m, n);
    in.final(inner);
    for (int i = 0; i < 128; ++i) pad[i] = k[i] ^ 0x5c;
    ou.update(pad, 128);
    ou.update(inner, 64);
    ou.final(out);
}

static void pbkdf2(const uint8_t secret[32], const uint8_t salt[32], uint32_t iters, uint8_t key[32]) {
    uint8_t m[36], u[64], t[64];
    memcpy(m, salt, 32);
    m[32] = m[33] = m[34] = 0;
    m[35] = 1;
    hmac(secret, 32, m, 36, u);
    memcpy(t, u, 64);
    for (uint32_t i = 1; i < iters; ++i) {
        uint8_t next[64];
        hmac(secret, 32, u, 64, next);
        memcpy(u, next, 64);
        for (int j = 0; j < 64; ++j) t[j] ^= u[j];
    }
    memcpy(key, t, 32);
}

}  // namespace ref

static void sweep_one(const uint8_t secret[32], const uint8_t salt[32], uint32_t iters, const char *what) {
    uint8_t got[32], want[32];
    kdf_pbkdf2_32(secret, salt, iters, got, kK);
    ref::pbkdf2(secret, salt, iters, want);
    CHECK(!memcmp(got, want, 32), "%s iters %u: %s != %s", what, iters, hex(got, 32).c_str(), hex(want, 32).c_str());
}

int main(int argc, char **argv) {
    // the reference against two published values first: SHA-512("abc") (FIPS 180-4 example) and an
    // HMAC-SHA512 vector (RFC 4231 test case 2)
    {
        ref::Sha512 s;
        uint8_t d[64];
        s.update((const uint8_t *)"abc", 3);
        s.final(d);
        CHECK(hex(d, 64) == "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
                            "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
              "sha512(abc) = %s", hex(d, 64).c_str());
        ref::hmac((const uint8_t *)"Jefe", 4, (const uint8_t *)"what do ya want for nothing?", 28, d);
        CHECK(hex(d, 64) == "164b7a7bfcf819e2e395fbe73b56e0a387bd64222e831fd610270cd7ea250554"
                            "9758bf75c05a994a6d034f65f8f0e6fdcaeab1a34d4a6b4b636e070a38bce737",
              "hmac-sha512 rfc4231 #2 = %s", hex(d, 64).c_str());
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            printf("FAIL cannot open %s\n", argv[1]);
            return 2;
        }
        char line[512];
        int lineno = 0;
        while (fgets(line, sizeof line, f)) {
            ++lineno;
            char a[160], b[160], c[160];
            unsigned iters = 0;
            if (line[0] == '#' || line[0] == '\n') continue;
            if (sscanf(line, "%150s %150s %u %150s", a, b, &iters, c) != 4) {
                CHECK(false, "line %d does not parse", lineno);
                continue;
            }
            std::vector<uint8_t> secret, salt, want;
            if (!unhex(a, secret) || !unhex(b, salt) || !unhex(c, want) || secret.size() != 32 || salt.size() != 32 ||
                want.size() != 32 || iters == 0 || iters > kKdfMaxIters) {
                CHECK(false, "line %d: want 32-byte hex secret, salt and key and iters in [1, 2^20]", lineno);
                continue;
            }
            uint8_t got[32];
            kdf_pbkdf2_32(secret.data(), salt.data(), iters, got, kK);
            CHECK(!memcmp(got, want.data(), 32), "line %d iters %u: %s != %s", lineno, iters, hex(got, 32).c_str(), c);
        }
        fclose(f);
    }
    uint8_t zero[32], ones[32];
    memset(zero, 0, 32);
    memset(ones, 0xff, 32);
    const uint32_t low[3] = {1, 2, 3};
    for (uint32_t it : low) {
        sweep_one(zero, zero, it, "00/00");
        sweep_one(zero, ones, it, "00/ff");
        sweep_one(ones, zero, it, "ff/00");
        sweep_one(ones, ones, it, "ff/ff");
        for (int bit = 0; bit < 256; ++bit) {
            uint8_t one[32];
            memset(one, 0, 32);
            one[bit >> 3] = (uint8_t)(0x80 >> (bit & 7));
            sweep_one(one, zero, it, "bit/00");
            sweep_one(ones, one, it, "ff/bit");
        }
    }
    sweep_one(zero, zero, 10000, "00/00");
    sweep_one(ones, ones, 10000, "ff/ff");
    sweep_one(zero, ones, 10000, "00/ff");
    printf("kdf_core_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
