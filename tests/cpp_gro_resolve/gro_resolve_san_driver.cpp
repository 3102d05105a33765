// gro_resolve_san_driver.cpp -- gro_find (gro_core.h), the search by which every slot of gro_unpack_kernel and
// gro_resolve_kernel finds its buffer, under the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer:
// a stand-alone program, no HIP, no Python.  Every table is a vector of exactly n_bufs entries, so a read at or
// past n_bufs is the sanitizer's to find.
//
//   1. ascending tables: for every slot i < n the index returned is the one a linear scan gives -- the last
//      buffer whose first is at or below i, 0 when none is.  Tables of equal counts (where the first guess is
//      exact), of mixed counts, all-lone tables, one 64-segment buffer first and one last (where the guess is far
//      off in either direction), tables with gaps in `first`, n_bufs of 1 and 2
//   2. tables whose `first` values do not ascend: every returned index is below n_bufs
//
// Prints "gro_resolve_san_driver ok" and exits 0, or says what differed and exits 1.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/gro_core.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED0F1Dull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// a table of these datagram counts, 100 bytes a datagram; gaps[b] slots are left unnamed before buffer b
struct Table {
    std::vector<qgcm_gro_buf> bufs;  // exactly n_bufs entries
    uint32_t n = 0;
};

Table table_of(const std::vector<uint32_t> &counts, const std::vector<uint32_t> &gaps = {}) {
    Table t;
    uint32_t off = 0;
    for (size_t b = 0; b < counts.size(); ++b) {
        if (b < gaps.size()) t.n += gaps[b];
        t.bufs.push_back(qgcm_gro_buf{off, 100 * counts[b], counts[b] > 1 ? 100u : 0u, t.n});
        CHECK(qgcm::gro_count(t.bufs.back().len, t.bufs.back().seg_len) == counts[b]);
        t.n += counts[b];
        off += 100 * counts[b];
    }
    return t;
}

uint32_t linear(const Table &t, uint64_t i) {
    uint32_t last = 0;
    for (uint32_t b = 0; b < t.bufs.size(); ++b)
        if (t.bufs[b].first <= i) last = b;
    return last;
}

void check_ascending(const Table &t, uint32_t extra_slots = 0) {
    const uint32_t n = t.n + extra_slots, nb = (uint32_t)t.bufs.size();
    CHECK(nb >= 1 && nb <= n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t got = qgcm::gro_find(t.bufs.data(), nb, n, i);
        if (got != linear(t, i)) {
            fprintf(stderr, "n_bufs %u n %u slot %llu: buffer %u, the scan says %u\n", nb, n, (unsigned long long)i, got, linear(t, i));
            ++failures;
            return;
        }
    }
}

void check_in_range(const std::vector<qgcm_gro_buf> &bufs, uint32_t n) {
    for (uint64_t i = 0; i < n; ++i) CHECK(qgcm::gro_find(bufs.data(), (uint32_t)bufs.size(), n, i) < bufs.size());
}

void test_ascending() {
    for (uint32_t nb : {1u, 2u, 3u, 7u, 64u, 65u, 1000u}) {
        for (uint32_t c : {1u, 2u, 45u, 64u}) check_ascending(table_of(std::vector<uint32_t>(nb, c)));  // equal counts; c == 1: all lone
        std::vector<uint32_t> mixed(nb), gaps(nb);
        for (uint32_t b = 0; b < nb; ++b) mixed[b] = 1 + rnd() % 64, gaps[b] = rnd() % 4 == 0 ? rnd() % 70 : 0;
        check_ascending(table_of(mixed));
        check_ascending(table_of(mixed, gaps));      // gaps in `first`, slot 0 unnamed now and then
        check_ascending(table_of(mixed, gaps), 77);  // and unnamed slots behind the last buffer
        std::vector<uint32_t> head(nb, 1), tail(nb, 1);
        head.front() = 64;  // the guess points far behind the buffer
        tail.back() = 64;   // ... and far in front of it
        check_ascending(table_of(head));
        check_ascending(table_of(tail));
        gaps.assign(nb, 0);
        gaps.front() = 500;
        check_ascending(table_of(head, gaps));  // every slot below the first `first`: buffer 0
    }
    check_ascending(table_of({64}));
    check_ascending(table_of({1}));
    check_ascending(table_of({64, 1}));
    check_ascending(table_of({1, 64}));
}

void test_not_ascending() {
    for (uint32_t nb : {1u, 2u, 3u, 16u, 333u}) {
        std::vector<uint32_t> counts(nb);
        for (auto &c : counts) c = 1 + rnd() % 64;
        Table t = table_of(counts);
        std::vector<qgcm_gro_buf> rev(t.bufs.rbegin(), t.bufs.rend());
        check_in_range(rev, t.n);  // descending
        std::vector<qgcm_gro_buf> junk = t.bufs;
        for (auto &b : junk) b.first = rnd();  // anything, most of it past n
        check_in_range(junk, t.n);
        for (auto &b : junk) b.first = rnd() % t.n;
        check_in_range(junk, t.n);
        for (auto &b : junk) b.first = 0xffffffffu;
        check_in_range(junk, t.n);
        for (auto &b : junk) b.first = 0;
        check_in_range(junk, t.n);
        check_in_range(junk, t.n + 1000);
    }
}

}  // namespace

int main() {
    test_ascending();
    test_not_ascending();
    if (failures) {
        fprintf(stderr, "gro_resolve_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("gro_resolve_san_driver ok");
    return 0;
}
