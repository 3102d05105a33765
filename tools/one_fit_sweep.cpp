// Sweeps the per-packet calls' size arithmetic (quantum_amd/csrc/one_fit.h) across its boundaries and
// checks it against the rule as qgcm.h states it.  Stand-alone host program, meant for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/one_fit_sweep.cpp -o one_fit_sweep && ./one_fit_sweep
// It also lays each fitting call out in a heap buffer of exactly the size the host asks for, the way
// qgcm_seal_one / qgcm_open_one and resident_call write it (record, tail, zeroed padding, the
// announced nonce's row), so an off-by-one in the arithmetic is an out-of-bounds write the address
// sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../quantum_amd/csrc/one_fit.h"

using namespace qgcm;

static int failures = 0;
#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            if (++failures < 20) fprintf(stderr, "%s:%d: L=%llu aad=%u seal=%d: %s\n", __FILE__, __LINE__, \
                                         (unsigned long long)L, aad, (int)seal, #c);               \
        }                                                                                          \
    } while (0)

static void one(uint64_t L, uint32_t aad, bool seal) {
    const uint64_t len = seal ? L : L + QGCM_OVERHEAD;  // what the call passes
    // the rule as the header states it
    const uint64_t rec = (4 + L + 28 + 15) & ~15ull;
    const uint64_t tail = aad > 4 ? (aad + 15ull) & ~15ull : 0;
    const bool fits = aad <= QGCM_MAX_AAD && rec + tail <= 32752;
    CHECK(one_record_bytes(len, seal) == rec);
    CHECK(one_tail_bytes(aad) == tail);
    CHECK(one_tail_rows(aad) * 16ull == tail);
    CHECK(one_aad_blocks(aad) == (aad <= 4 ? 1u : (uint32_t)(tail / 16)));
    CHECK(one_fits_launch(len, seal, aad) == fits);
    const bool res = fits && rec + tail <= kResSlotBytes, res_ann = fits && rec + tail + 16 <= kResSlotBytes;
    CHECK(one_fits_resident(len, seal, aad, false) == res);
    CHECK(one_fits_resident(len, seal, aad, true) == res_ann);
    CHECK(!res_ann || res);
    if (one_fits_launch(len, seal, aad)) {  // the launch path's staging: record, tail, 16 B of status
        std::vector<uint8_t> a(aad, 0xA5), d(len, 0x5A);
        const uint64_t sb = one_record_bytes(len, seal) + one_tail_bytes(aad);
        CHECK(sb + 16 <= kOneCap + 4096);  // a pooled staging slot holds it
        uint8_t *h = (uint8_t *)malloc(sb + 16);
        memset(h, 0, sb);
        if (aad) memcpy(tail ? h + rec : h, a.data(), aad);
        if (len) memcpy(h + 4, d.data(), len);  // (the calls' data pointer is never NULL)
        if (seal) memset(h + 4 + L + 16, 1, 12);
        h[sb] = 0;
        h[sb + 1] = 0;
        free(h);
    }
    for (int ann = 0; ann < 2; ++ann) {
        if (!one_fits_resident(len, seal, aad, ann != 0)) continue;
        std::vector<uint8_t> a(aad, 0xA5), d(len, 0x5A);
        uint8_t *slot = (uint8_t *)malloc(kResSlotBytes);
        const uint64_t stage = one_record_bytes(len, seal), t = one_tail_bytes(aad);
        memset(slot, 0, 4);
        if (aad && !t) memcpy(slot, a.data(), aad);
        if (len) memcpy(slot + 4, d.data(), len);
        if (seal) memset(slot + 4 + L + 16, 1, 12);
        if (t) {
            memcpy(slot + stage, a.data(), aad);
            memset(slot + stage + aad, 0, t - aad);
        }
        if (ann) {
            CHECK(stage + t <= kResSlotBytes - 16);  // the tail stops short of the announced nonce
            memset(slot + kResSlotBytes - 16, 2, 12);
        }
        free(slot);
    }
}

int main() {
    std::vector<uint32_t> aads = {0, 1, 3, 4, 5, 13, 15, 16, 17, 31, 32, 33, 64, 672, 673, 976, 992, 1000, 1008, 1009, 1024,
                                  8000, 16383, 16384, 16385, 65536, 0x7fffffffu, 0xfffffff0u, 0xffffffffu};
    std::vector<uint64_t> Ls = {0, 1, 15, 16, 17, 100, 1350, 2016, 2032, 2033, 9000, 16000, 20000, 32000};
    // every L around the resident slot and the staging cap, for every listed AAD length's row count
    for (uint64_t base : {(uint64_t)kResSlotBytes, (uint64_t)kOneCap, (uint64_t)kOneCap / 2})
        for (uint32_t aad : {0u, 5u, 16u, 17u, 1000u, 8000u, 16384u}) {
            const uint64_t t = aad > 4 ? (aad + 15ull) & ~15ull : 0;
            if (base < t + 128) continue;
            for (uint64_t L = base - t - 128; L <= base - t + 64; ++L) Ls.push_back(L);
        }
    size_t cases = 0;
    for (uint64_t L : Ls)
        for (uint32_t aad : aads)
            for (int seal = 0; seal < 2; ++seal, ++cases) one(L, aad, seal != 0);
    // the largest lengths the API lets through
    one((uint64_t)QGCM_MAX_PAYLOAD - 1, 5, true);
    one((uint64_t)QGCM_MAX_PAYLOAD - 1, 16384, false);
    printf("one_fit_sweep: %zu cases, %d failures\n", cases + 2, failures);
    return failures ? 1 : 0;
}
