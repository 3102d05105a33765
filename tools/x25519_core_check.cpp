// Checks the shared-secret arithmetic shared by host and device (quantum_amd/csrc/x25519_core.h): the
// GF(2^255 - 19) field on ten 26/25-bit limbs and the RFC 7748 X25519 ladder.  Stand-alone host program
// with no HIP, meant for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/x25519_core_check.cpp -o x25519_core_check && ./x25519_core_check [vector file]
// The vector file holds lines of `scalar point expected` (hex, 32 bytes each; blank lines and lines
// starting with # are skipped); each is computed and compared.  Then it checks by itself
//   * tobytes(frombytes(x)) for x in {0, 1, 18, 19, p-1, p, p+1, 2^255-20, 2^255-1, 2^256-1} against
//     (x mod 2^255) mod p worked out byte by byte (10 checks);
//   * for 64 field elements (the ten above and pseudo-random ones, also as sums and differences, the
//     widest operands the ladder multiplies): sq(a) = mul(a, a), mul(a, b) = mul(b, a), and a * a^-1 = 1
//     or, for a = 0 mod p, 0 (3 x 64 checks);
//   * the ladder on every pair of 8 edge scalars and 16 edge points, and on 32 pseudo-random pairs,
//     against a second ladder written below on sixteen 16-bit limbs in 64-bit signed words, which shares
//     nothing with the header (160 checks).
// It ends with "x25519_core_check: <checks> checks, <failures> failures" and exits 1 if any failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../quantum_amd/csrc/x25519_core.h"

using namespace qgcm;

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

// ---- second implementation: sixteen 16-bit limbs in int64 ----
namespace ref {

typedef int64_t gf[16];

static void carry(gf o) {
    for (int i = 0; i < 16; ++i) {
        o[i] += 1LL << 16;
        const int64_t c = o[i] >> 16;
        o[(i + 1) * (i < 15)] += c - 1 + 37 * (c - 1) * (i == 15);
        o[i] -= c * 65536;  // (not c << 16: c may be negative)
    }
}
static void sel(gf p, gf q, int b) {
    const int64_t c = ~(int64_t)(b - 1);
    for (int i = 0; i < 16; ++i) {
        const int64_t t = c & (p[i] ^ q[i]);
        p[i] ^= t;
        q[i] ^= t;
    }
}
static void pack(uint8_t o[32], const gf n) {
    gf m, t;
    for (int i = 0; i < 16; ++i) t[i] = n[i];
    carry(t);
    carry(t);
    carry(t);
    for (int j = 0; j < 2; ++j) {
        m[0] = t[0] - 0xffed;
        for (int i = 1; i < 15; ++i) {
            m[i] = t[i] - 0xffff - ((m[i - 1] >> 16) & 1);
            m[i - 1] &= 0xffff;
        }
        m[15] = t[15] - 0x7fff - ((m[14] >> 16) & 1);
        const int b = (int)((m[15] >> 16) & 1);
        m[14] &= 0xffff;
        sel(t, m, 1 - b);
    }
    for (int i = 0; i < 16; ++i) {
        o[2 * i] = (uint8_t)(t[i] & 0xff);
        o[2 * i + 1] = (uint8_t)(t[i] >> 8);
    }
}
static void unpack(gf o, const uint8_t n[32]) {
    for (int i = 0; i < 16; ++i) o[i] = n[2 * i] + ((int64_t)n[2 * i + 1] << 8);
    o[15] &= 0x7fff;
}
static void add(gf o, const gf a, const gf b) { for (int i = 0; i < 16; ++i) o[i] = a[i] + b[i]; }
static void sub(gf o, const gf a, const gf b) { for (int i = 0; i < 16; ++i) o[i] = a[i] - b[i]; }
static void mul(gf o, const gf a, const gf b) {
    int64_t t[31];
    for (int i = 0; i < 31; ++i) t[i] = 0;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) t[i + j] += a[i] * b[j];
    for (int i = 0; i < 15; ++i) t[i] += 38 * t[i + 16];
    for (int i = 0; i < 16; ++i) o[i] = t[i];
    carry(o);
    carry(o);
}
static void inv(gf o, const gf a) {
    gf c;
    for (int i = 0; i < 16; ++i) c[i] = a[i];
    for (int e = 253; e >= 0; --e) {
        mul(c, c, c);
        if (e != 2 && e != 4) mul(c, c, a);
    }
    for (int i = 0; i < 16; ++i) o[i] = c[i];
}
static void x25519(uint8_t q[32], const uint8_t n[32], const uint8_t p[32]) {
    static const gf k121665 = {0xDB41, 1};
    uint8_t z[32];
    gf x, a, b, c, d, e, f;
    memcpy(z, n, 32);
    z[31] = (uint8_t)((n[31] & 127) | 64);
    z[0] &= 248;
    unpack(x, p);
    for (int i = 0; i < 16; ++i) {
        b[i] = x[i];
        d[i] = a[i] = c[i] = 0;
    }
    a[0] = d[0] = 1;
    for (int i = 254; i >= 0; --i) {
        const int r = (z[i >> 3] >> (i & 7)) & 1;
        sel(a, b, r);
        sel(c, d, r);
        add(e, a, c);
        sub(a, a, c);
        add(c, b, d);
        sub(b, b, d);
        mul(d, e, e);
        mul(f, a, a);
        mul(a, c, a);
        mul(c, b, e);
        add(e, a, c);
        sub(a, a, c);
        mul(b, a, a);
        sub(c, d, f);
        mul(a, c, k121665);
        add(a, a, d);
        mul(c, c, a);
        mul(a, d, f);
        mul(d, b, x);
        mul(b, e, e);
        sel(a, b, r);
        sel(c, d, r);
    }
    inv(c, c);
    mul(a, a, c);
    pack(q, a);
}

// (x mod 2^255) mod p on bytes: clear bit 255, then subtract p once if the value is p or more
static void canonical(uint8_t out[32], const uint8_t x[32]) {
    uint8_t v[32], p[32], d[32];
    memcpy(v, x, 32);
    v[31] &= 127;
    memset(p, 0xff, 32);
    p[0] = 0xed;
    p[31] = 0x7f;
    int borrow = 0;
    for (int i = 0; i < 32; ++i) {
        const int t = (int)v[i] - p[i] - borrow;
        d[i] = (uint8_t)(t & 0xff);
        borrow = t < 0;
    }
    memcpy(out, borrow ? v : d, 32);
}

}  // namespace ref

static uint64_t rng_state = 0x5832353531394bULL;
static uint8_t rnd_byte() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return (uint8_t)((z ^ (z >> 31)) >> 24);
}
struct Bytes32 {
    uint8_t b[32];
};
static Bytes32 rnd32() {
    Bytes32 r;
    for (int i = 0; i < 32; ++i) r.b[i] = rnd_byte();
    return r;
}
static Bytes32 filled(uint8_t v) {
    Bytes32 r;
    memset(r.b, v, 32);
    return r;
}
// `fill` in every byte, with byte 0 and byte 31 replaced
static Bytes32 shaped(uint8_t fill, uint8_t b0, uint8_t b31) {
    Bytes32 r = filled(fill);
    r.b[0] = b0;
    r.b[31] = b31;
    return r;
}

static void words_of(uint32_t w[8], const uint8_t b[32]) {
    for (int i = 0; i < 8; ++i)
        w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
}
static void bytes_of(uint8_t b[32], const uint32_t w[8]) {
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[i] >> (8 * j));
}
static void fe_of(fe25519 &f, const Bytes32 &x) {
    uint32_t w[8];
    words_of(w, x.b);
    fe_frombytes(f, w);
}
static Bytes32 bytes_of_fe(const fe25519 &f) {
    uint32_t w[8];
    Bytes32 r;
    fe_tobytes(w, f);
    bytes_of(r.b, w);
    return r;
}

// 0, 1, 18, 19, p-1, p, p+1, 2^255-20, 2^255-1, 2^256-1
static std::vector<Bytes32> field_edges() {
    return {shaped(0, 0, 0),          shaped(0, 1, 0),          shaped(0, 18, 0),         shaped(0, 19, 0),
            shaped(0xff, 0xec, 0x7f), shaped(0xff, 0xed, 0x7f), shaped(0xff, 0xee, 0x7f), shaped(0xff, 0xec, 0x7f),
            shaped(0xff, 0xff, 0x7f), shaped(0xff, 0xff, 0xff)};
}

static void check_field() {
    std::vector<Bytes32> edges = field_edges();
    for (const Bytes32 &x : edges) {
        fe25519 f;
        fe_of(f, x);
        uint8_t want[32];
        ref::canonical(want, x.b);
        const Bytes32 got = bytes_of_fe(f);
        CHECK(memcmp(got.b, want, 32) == 0, "tobytes(frombytes(%s)) = %s, want %s", hex(x.b, 32).c_str(),
              hex(got.b, 32).c_str(), hex(want, 32).c_str());
    }
    // 64 operands: the edges, pseudo-random elements, and sums and differences of two (the widest limbs the
    // ladder hands to mul and sq)
    std::vector<fe25519> ops;
    for (const Bytes32 &x : edges) {
        fe25519 f;
        fe_of(f, x);
        ops.push_back(f);
    }
    while (ops.size() < 30) {
        fe25519 f;
        fe_of(f, rnd32());
        ops.push_back(f);
    }
    for (size_t i = 0; ops.size() < 64; ++i) {
        fe25519 f;
        if (i & 1) fe_add(f, ops[i % 30], ops[(7 * i + 3) % 30]);
        else fe_sub(f, ops[i % 30], ops[(7 * i + 3) % 30]);
        ops.push_back(f);
    }
    const Bytes32 one = shaped(0, 1, 0), zero = shaped(0, 0, 0);
    for (size_t i = 0; i < ops.size(); ++i) {
        const fe25519 &a = ops[i], &b = ops[(i * 5 + 11) % ops.size()];
        fe25519 s, m, ab, ba, ai, r;
        fe_sq(s, a);
        fe_mul(m, a, a);
        CHECK(memcmp(bytes_of_fe(s).b, bytes_of_fe(m).b, 32) == 0, "sq != mul for operand %zu", i);
        fe_mul(ab, a, b);
        fe_mul(ba, b, a);
        CHECK(memcmp(bytes_of_fe(ab).b, bytes_of_fe(ba).b, 32) == 0, "mul not commutative for operand %zu", i);
        fe25519 ared, unit;  // a reduced copy for the inversion (the ladder inverts a product)
        fe_set_small(unit, 1);
        fe_mul(ared, a, unit);
        fe_invert(ai, ared);
        fe_mul(r, ared, ai);
        const bool is_zero = memcmp(bytes_of_fe(a).b, zero.b, 32) == 0;
        CHECK(memcmp(bytes_of_fe(r).b, is_zero ? zero.b : one.b, 32) == 0, "a * a^-1 = %s for operand %zu",
              hex(bytes_of_fe(r).b, 32).c_str(), i);
    }
}

static void check_pair(const Bytes32 &k, const Bytes32 &u) {
    uint8_t got[32], want[32];
    x25519_bytes(got, k.b, u.b);
    ref::x25519(want, k.b, u.b);
    CHECK(memcmp(got, want, 32) == 0, "X25519(%s, %s) = %s, want %s", hex(k.b, 32).c_str(), hex(u.b, 32).c_str(),
          hex(got, 32).c_str(), hex(want, 32).c_str());
}

static void check_ladder() {
    // scalars: all-00, all-ff, only bit 0, only bit 254, only bit 255, bits 0..2 (cleared by the clamp), two random
    std::vector<Bytes32> ks = {filled(0), filled(0xff), shaped(0, 1, 0), shaped(0, 0, 0x40), shaped(0, 0, 0x80),
                               shaped(0, 7, 0), rnd32(), rnd32()};
    // points: 0, 1, 9, p-1, p, p+1, 2^255-1, 2^256-1, p-1 and p with bit 255 set, the rest of the list in RFC
    // 7748 s6.1's note (2p-1, 2p, 2p+1, the two points of order 8), and a random one
    static const char *order8[] = {"e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800",
                                   "5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157"};
    std::vector<Bytes32> us = {shaped(0, 0, 0),          shaped(0, 1, 0),          shaped(0, 9, 0),
                               shaped(0xff, 0xec, 0x7f), shaped(0xff, 0xed, 0x7f), shaped(0xff, 0xee, 0x7f),
                               shaped(0xff, 0xff, 0x7f), shaped(0xff, 0xff, 0xff), shaped(0xff, 0xec, 0xff),
                               shaped(0xff, 0xed, 0xff), shaped(0xff, 0xd9, 0xff), shaped(0xff, 0xda, 0xff),
                               shaped(0xff, 0xdb, 0xff)};
    for (const char *h : order8) {
        std::vector<uint8_t> v;
        unhex(h, v);
        Bytes32 b;
        memcpy(b.b, v.data(), 32);
        us.push_back(b);
    }
    while (us.size() < 16) us.push_back(rnd32());
    for (const Bytes32 &k : ks)
        for (const Bytes32 &u : us) check_pair(k, u);
    for (int i = 0; i < 32; ++i) check_pair(rnd32(), rnd32());
}

static void check_vectors(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) {
        CHECK(false, "cannot open %s", path);
        return;
    }
    char line[512];
    int lineno = 0;
    while (fgets(line, sizeof line, f)) {
        ++lineno;
        char a[200], b[200], c[200];
        if (line[0] == '#' || line[0] == '\n') continue;
        if (sscanf(line, "%199s %199s %199s", a, b, c) != 3) {
            CHECK(false, "%s:%d: not `scalar point expected`", path, lineno);
            continue;
        }
        std::vector<uint8_t> k, u, want;
        if (!unhex(a, k) || !unhex(b, u) || !unhex(c, want) || k.size() != 32 || u.size() != 32 || want.size() != 32) {
            CHECK(false, "%s:%d: three 32-byte hex strings expected", path, lineno);
            continue;
        }
        uint8_t got[32];
        x25519_bytes(got, k.data(), u.data());
        CHECK(memcmp(got, want.data(), 32) == 0, "%s:%d: got %s, want %s", path, lineno, hex(got, 32).c_str(), c);
    }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc > 1) check_vectors(argv[1]);
    check_field();
    check_ladder();
    printf("x25519_core_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
