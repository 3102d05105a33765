// Checks the nonce generator's host logic (quantum_amd/csrc/nonce_rng.h): key expansion, 128-bit counter
// arithmetic, reservation and the reseed rule.  Stand-alone host program with no HIP, meant for the
// sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/nonce_rng_check.cpp -o nonce_rng_check && ./nonce_rng_check [key as 64 hex digits]...
// For each key on the command line (default: the all-zero key) it prints one line
//   rk <key hex> <the 240 schedule bytes as hex>
// taken from NonceKeys::rk (LE column words, so the bytes are the FIPS-197 schedule in order) after checking
// rr = rot16(rk); tests/test_nonce_host.py compares those lines with the oracle's expansion.  Then it sweeps
// the counter arithmetic against a byte-wise big-endian add and the reseed rule against its statement in
// include/qgcm.h, and ends with "nonce_rng_check: <checks> checks, <failures> failures".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../quantum_amd/csrc/nonce_rng.h"

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

// reference: schoolbook big-endian add of a 64-bit value to 16 bytes, mod 2^128
static void be_add(uint8_t be[16], uint64_t n) {
    unsigned carry = 0;
    for (int i = 15; i >= 0; --i) {
        const unsigned add = (i >= 8 ? (unsigned)((n >> (8 * (15 - i))) & 0xff) : 0u) + carry;
        const unsigned s = be[i] + add;
        be[i] = (uint8_t)s;
        carry = s >> 8;
    }
}

static std::string hex(const uint8_t *p, size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

// deterministic entropy for the reseed sweep: every draw differs from the one before
static uint64_t g_entropy_calls = 0;
static bool fake_entropy(void *buf, size_t n) {
    ++g_entropy_calls;
    uint8_t *p = static_cast<uint8_t *>(buf);
    for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)(0x5a + 31 * i + 7 * g_entropy_calls);
    return true;
}
static bool no_entropy(void *, size_t) { return false; }

static void print_keys(const char *keyhex) {
    uint8_t key[32] = {};
    if (strlen(keyhex) != 64) {
        printf("FAIL key '%s' is not 64 hex digits\n", keyhex);
        ++failures;
        return;
    }
    for (int i = 0; i < 32; ++i) {
        unsigned b = 0;
        if (sscanf(keyhex + 2 * i, "%2x", &b) != 1) {
            printf("FAIL key '%s' is not hex\n", keyhex);
            ++failures;
            return;
        }
        key[i] = (uint8_t)b;
    }
    NonceKeys k;
    nonce_expand_key(key, k);
    uint8_t bytes[240];
    for (int i = 0; i < 60; ++i) {
        for (int j = 0; j < 4; ++j) bytes[4 * i + j] = (uint8_t)(k.rk[i] >> (8 * j));
        CHECK(k.rr[i] == ((k.rk[i] << 16) | (k.rk[i] >> 16)), "rr[%d] is not rot16(rk[%d])", i, i);
    }
    CHECK(memcmp(bytes, key, 32) == 0, "the schedule does not start with the key");
    printf("rk %s %s\n", hex(key, 32).c_str(), hex(bytes, 240).c_str());
}

static void counter_sweep() {
    // starts just below the 32-bit, 64-bit and 128-bit carries; reservations of 1, 7 and 2^31
    uint8_t starts[3][16];
    memset(starts, 0, sizeof starts);
    memset(starts[0] + 12, 0xff, 4);   // 2^32 - 3
    starts[0][15] = 0xfd;
    memset(starts[1] + 8, 0xff, 8);    // 2^64 - 3
    starts[1][15] = 0xfd;
    memset(starts[2], 0xff, 16);       // 2^128 - 3
    starts[2][15] = 0xfd;
    const uint64_t sizes[] = {1, 7, 1ull << 31};
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)i;
    for (auto &st : starts) {
        // the conversion round-trips, and single steps carry through every byte
        uint32_t v[4];
        uint8_t back[16], want[16];
        ctr128_from_be(st, v);
        ctr128_to_be(v, back);
        CHECK(memcmp(back, st, 16) == 0, "BE128 round trip of %s", hex(st, 16).c_str());
        memcpy(want, st, 16);
        for (int j = 0; j < 8; ++j) {
            ctr128_add(v, 1);
            be_add(want, 1);
            ctr128_to_be(v, back);
            CHECK(memcmp(back, want, 16) == 0, "%s + %d: %s, want %s", hex(st, 16).c_str(), j + 1,
                  hex(back, 16).c_str(), hex(want, 16).c_str());
        }
        for (uint64_t a : sizes)
            for (uint64_t b : sizes) {
                // two reservations in a row: the first starts at the seed, the second where the first ended,
                // and a lease's part for packet p starts p further on
                NonceRng rng(fake_entropy, 1ull << 40);
                CHECK(rng.seed(key, st), "seed");
                NonceLease l1, l2;
                CHECK(rng.reserve(a, l1) && rng.reserve(b, l2), "reserve");
                uint8_t got[16];
                memcpy(want, st, 16);
                ctr128_to_be(l1.v, got);
                CHECK(memcmp(got, want, 16) == 0, "first lease starts at %s, want %s", hex(got, 16).c_str(),
                      hex(want, 16).c_str());
                be_add(want, a);
                ctr128_to_be(l2.v, got);
                CHECK(memcmp(got, want, 16) == 0, "lease after %llu starts at %s, want %s", (unsigned long long)a,
                      hex(got, 16).c_str(), hex(want, 16).c_str());
                const NonceLease part = lease_at(l2, b - 1);
                be_add(want, b - 1);
                ctr128_to_be(part.v, got);
                CHECK(memcmp(got, want, 16) == 0, "lease_at(%llu) is %s, want %s", (unsigned long long)(b - 1),
                      hex(got, 16).c_str(), hex(want, 16).c_str());
                CHECK(memcmp(&part.keys, &l1.keys, sizeof(NonceKeys)) == 0, "one key across reservations");
                CHECK(rng.since_seed() == a + b && rng.draws() == 0, "count since seed");
            }
    }
}

// the rule as include/qgcm.h states it
static bool want_reseed(uint64_t since, uint64_t n, uint64_t interval) { return since > 0 && since + n > interval; }

static void reseed_sweep() {
    const uint64_t interval = 64, sizes[] = {1, 63, 64, 65, 200};
    uint8_t key[32], ctr[16];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)(0xa0 + i);
    memset(ctr, 0, sizeof ctr);
    ctr[15] = 9;
    for (uint64_t a : sizes)
        for (uint64_t b : sizes)
            for (uint64_t c : sizes) {
                NonceRng rng(fake_entropy, interval);
                CHECK(rng.seed(key, ctr), "seed");
                uint64_t since = 0, draws = 0, prev_n = 0;
                NonceLease prev{};
                bool have_prev = false;
                for (uint64_t n : {a, b, c}) {
                    const bool reseed = want_reseed(since, n, interval);
                    NonceLease l;
                    CHECK(rng.reserve(n, l), "reserve");
                    if (reseed) {
                        ++draws;
                        since = 0;
                    }
                    CHECK(rng.draws() == draws, "calls %llu %llu %llu: %llu draws before/at a call of %llu, want %llu",
                          (unsigned long long)a, (unsigned long long)b, (unsigned long long)c,
                          (unsigned long long)rng.draws(), (unsigned long long)n, (unsigned long long)draws);
                    if (have_prev) {
                        const bool same_key = memcmp(&l.keys, &prev.keys, sizeof(NonceKeys)) == 0;
                        CHECK(same_key == !reseed, "key %s across a call that %s", same_key ? "kept" : "changed",
                              reseed ? "reseeds" : "does not reseed");
                        if (!reseed) {  // the stream continues where the previous call ended
                            const NonceLease cont = lease_at(prev, prev_n);
                            CHECK(memcmp(cont.v, l.v, sizeof l.v) == 0, "the stream continues after %llu",
                                  (unsigned long long)prev_n);
                        }
                    }
                    prev_n = n;
                    since += n;
                    CHECK(rng.since_seed() == since, "since-seed count %llu, want %llu",
                          (unsigned long long)rng.since_seed(), (unsigned long long)since);
                    prev = l;
                    have_prev = true;
                }
            }
    // a call larger than the interval right after a seed still uses one key and no draw
    {
        NonceRng rng(fake_entropy, interval);
        rng.seed(key, ctr);
        NonceLease l;
        CHECK(rng.reserve(200, l) && rng.draws() == 0, "a first call past the interval draws nothing");
        CHECK(rng.reserve(1, l) && rng.draws() == 1, "the call after it reseeds");
    }
    // first use without a seed draws K and V; seed(NULL) draws again and restarts the count
    {
        NonceRng rng(fake_entropy, interval);
        NonceLease l1, l2;
        CHECK(rng.reserve(5, l1) && rng.draws() == 1 && rng.since_seed() == 5, "first use seeds from the entropy source");
        CHECK(rng.seed(nullptr, nullptr) && rng.draws() == 2 && rng.since_seed() == 0, "seed(NULL) reseeds");
        CHECK(rng.reserve(5, l2) && memcmp(&l1.keys, &l2.keys, sizeof(NonceKeys)) != 0, "a reseed changes the key");
    }
    // a failing entropy source reserves nothing
    {
        NonceRng rng(no_entropy, interval);
        NonceLease l;
        CHECK(!rng.reserve(1, l) && rng.since_seed() == 0, "no entropy, no reservation");
        CHECK(rng.seed(key, ctr) && rng.reserve(1, l), "an explicit seed needs none");
    }
    // interval 0 is read as 1; the default is 2^32
    CHECK(NonceRng(fake_entropy, 0).interval() == 1 && NonceRng().interval() == (1ull << 32), "interval bounds");
    // the real source fills what it is asked for
    {
        uint8_t a[48] = {}, z[48] = {};
        CHECK(nonce_getrandom(a, sizeof a) && memcmp(a, z, sizeof a) != 0, "getrandom");
    }
}

int main(int argc, char **argv) {
    if (argc < 2) print_keys("0000000000000000000000000000000000000000000000000000000000000000");
    for (int i = 1; i < argc; ++i) print_keys(argv[i]);
    counter_sweep();
    reseed_sweep();
    printf("nonce_rng_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
