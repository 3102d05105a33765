// frames_san_driver.cpp -- the packed frames' host code (frames_core.h: the table checks and
// qgcm_frames_unpack_cpu's body) under the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program, no HIP, no Python.
//
//   1. the unpack from arrays of exactly the size the contract names (the packed area exactly packed_len bytes,
//      the table exactly n entries, the arena exactly n * stride, lens exactly n) against a byte-by-byte
//      restatement: every length around the 4- and 16-byte pieces, the slot's end and past it, frames that end
//      exactly at packed_len, empty frames
//   2. every class of table that is not valid, and the argument checks: QGCM_E_ARG, nothing written
//   3. the pipeline's table check: ascending without overlap
//
// Prints "frames_san_driver ok" and exits 0, or says what differed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/frames_core.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED00F4ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

constexpr uint8_t kSentinel = 0xA5;
constexpr uint32_t kLenSentinel = 0xDEADBEEFu;

struct Case {
    std::vector<uint8_t> packed;     // exactly packed_len bytes
    std::vector<qgcm_frame> frames;  // exactly n entries
};

// the lengths back to back, each frame on the next 16-byte boundary, a gap now and then; the area ends with the
// last frame
Case layout(const std::vector<uint32_t> &lens) {
    Case c;
    uint64_t at = 0, end = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
        if (i % 5 == 3) at += 16 * (1 + i % 3);
        c.frames.push_back(qgcm_frame{(uint32_t)at, lens[i]});
        end = at + lens[i];
        at = (end + 15) & ~(uint64_t)15;
    }
    c.packed.resize(end);
    for (auto &b : c.packed) b = (uint8_t)rnd();
    return c;
}

void run(const Case &c, uint64_t stride) {
    const uint32_t n = (uint32_t)c.frames.size();
    std::vector<uint8_t> arena(n * stride, kSentinel), want(n * stride, kSentinel);
    std::vector<uint32_t> lens(n, kLenSentinel);
    CHECK(qgcm::frames_unpack_checked(c.packed.data(), c.packed.size(), c.frames.data(), n, arena.data(), stride, lens.data()) ==
          QGCM_OK);
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(lens[i] == c.frames[i].len);
        for (uint64_t k = 0; k < c.frames[i].len && 4 + k < stride; ++k) want[i * stride + 4 + k] = c.packed[c.frames[i].off + k];
    }
    CHECK(arena == want);
}

void unpack_cases() {
    for (uint64_t stride : {1536ull, 1388ull, 64ull, 8ull}) {
        std::vector<uint32_t> lens = {0, 1, 3, 4, 11, 12, 13, 15, 16, 19, 20, 21, 27, 28, 29, 31, 32, 33, 255, 256, 257, 1350};
        for (uint64_t l : {stride - 4, stride - 3, 2 * stride, stride}) lens.push_back((uint32_t)l);
        if (stride > 32) lens.push_back((uint32_t)stride - 32), lens.push_back((uint32_t)stride - 31);
        lens.push_back(77);  // the area ends off the 16-byte grid
        run(layout(lens), stride);
        std::vector<uint32_t> seeded;
        for (int i = 0; i < 200; ++i) seeded.push_back(rnd() % 3 == 0 ? rnd() % 40 : rnd() % 3000);
        run(layout(seeded), stride);
    }
    run(layout({}), 64);  // n == 0: empty vectors, NULL data
}

void refusals() {
    const Case good = layout({64, 100, 64, 100, 64, 100, 64, 100, 77});
    const uint32_t n = (uint32_t)good.frames.size();
    const uint64_t packed_len = good.packed.size();
    CHECK(qgcm::frames_table_ok(good.frames.data(), n, packed_len) && qgcm::frames_table_ascends(good.frames.data(), n, packed_len));
    struct Bad {
        uint32_t i;
        qgcm_frame f;
    };
    const Bad bad[] = {
        {4, {good.frames[4].off + 4, 8}},                                   // off not on a 16-byte boundary
        {8, {good.frames[8].off, good.frames[8].len + 1}},                  // one past the end
        {2, {(uint32_t)((packed_len + 15) & ~(uint64_t)15), 1}},            // off past the end
        {5, {0xFFFFFFF0u, 0x20u}},                                          // off + len wraps 32 bits
        {0, {0, 0xFFFFFFFFu}},
    };
    for (const Bad &b : bad) {
        std::vector<qgcm_frame> t = good.frames;
        t[b.i] = b.f;
        std::vector<uint8_t> arena(n * 256, kSentinel);
        std::vector<uint32_t> lens(n, kLenSentinel);
        CHECK(!qgcm::frames_table_ok(t.data(), n, packed_len) && !qgcm::frames_table_ascends(t.data(), n, packed_len));
        CHECK(qgcm::frames_unpack_checked(good.packed.data(), packed_len, t.data(), n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
        for (uint8_t v : arena) CHECK(v == kSentinel);
        for (uint32_t v : lens) CHECK(v == kLenSentinel);
    }
    std::vector<uint8_t> arena(n * 256, kSentinel);
    std::vector<uint32_t> lens(n, kLenSentinel);
    const uint8_t *p = good.packed.data();
    const qgcm_frame *f = good.frames.data();
    CHECK(qgcm::frames_unpack_checked(nullptr, packed_len, f, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::frames_unpack_checked(p, packed_len, nullptr, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::frames_unpack_checked(p, packed_len, f, n, nullptr, 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::frames_unpack_checked(p, packed_len, f, n, arena.data(), 256, nullptr) == QGCM_E_ARG);
    for (uint64_t stride : {0ull, 4ull, 258ull})
        CHECK(qgcm::frames_unpack_checked(p, packed_len, f, n, arena.data(), stride, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::frames_unpack_checked(p, packed_len, f, QGCM_MAX_BATCH + 1, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    for (uint8_t v : arena) CHECK(v == kSentinel);
    CHECK(qgcm::frames_unpack_checked(nullptr, 0, nullptr, 0, nullptr, 256, nullptr) == QGCM_OK);
}

void ascending() {
    const Case good = layout({64, 100, 0, 100, 64});
    const uint32_t n = (uint32_t)good.frames.size();
    const uint64_t packed_len = good.packed.size();
    std::vector<qgcm_frame> t = good.frames;
    std::swap(t[1], t[3]);  // unsorted
    CHECK(qgcm::frames_table_ok(t.data(), n, packed_len) && !qgcm::frames_table_ascends(t.data(), n, packed_len));
    t = good.frames;
    t[0].len = t[1].off + 1;  // one byte into the next frame
    CHECK(qgcm::frames_table_ok(t.data(), n, packed_len) && !qgcm::frames_table_ascends(t.data(), n, packed_len));
    t[0].len = t[1].off;  // touching is no overlap
    CHECK(qgcm::frames_table_ascends(t.data(), n, packed_len));
    t = good.frames;
    t[3] = t[2];  // an empty frame twice at one offset
    t[3].len = 0;
    CHECK(qgcm::frames_table_ascends(t.data(), n, packed_len));
    CHECK(qgcm::frames_table_ascends(nullptr, 0, 0));
}

}  // namespace

int main() {
    unpack_cases();
    refusals();
    ascending();
    if (failures) {
        fprintf(stderr, "frames_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("frames_san_driver ok");
    return 0;
}
