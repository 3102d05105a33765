// gro_san_driver.cpp -- the host unpack (gro_core.h) and the coalesced receive (udp_batch.cpp) under the host
// compiler's AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no HIP, no Python.
//
//   1. the unpack into arrays of exactly the size the contract names (the packed area exactly packed_len
//      bytes, the arena n * stride, the lengths n), against a byte-by-byte restatement: lone and coalesced
//      buffers at every source residue, a stride shorter than the datagrams, skipped buffers
//   2. the table check: prefix sums, totals, counts that would overflow 32 bits
//   3. trains from qgcm_udp_send_plan and plain datagrams over loopback into a packed area of exactly
//      packed_cap bytes and a table of exactly max_bufs entries: everything arrives in order, with the
//      UDP_GRO option on and off, across calls that stop for slots, room and entries
//
// Prints "gro_san_driver ok" and exits 0, or says what differed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
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

uint64_t rng_state = 0x5EED0061ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Spec {
    uint32_t len, seg_len, mod;
};

// the contract, byte by byte
void contract(const std::vector<uint8_t> &packed, uint64_t packed_len, const std::vector<qgcm_gro_buf> &bufs, uint32_t n,
              std::vector<uint8_t> &arena, uint64_t stride, std::vector<uint32_t> &lens) {
    for (const qgcm_gro_buf &b : bufs) {
        const uint64_t count = (b.seg_len == 0 || b.seg_len >= b.len) ? 1 : ((uint64_t)b.len + b.seg_len - 1) / b.seg_len;
        if ((uint64_t)b.off + b.len > packed_len || b.first + count > n) continue;
        for (uint64_t k = 0; k < count; ++k) {
            const uint64_t L = count == 1 ? b.len : std::min<uint64_t>(b.seg_len, b.len - k * b.seg_len);
            lens[b.first + k] = (uint32_t)L;
            for (uint64_t j = 0; j < std::min(L, stride); ++j) arena[(b.first + k) * stride + j] = packed[b.off + k * b.seg_len + j];
        }
    }
}

void unpack_case(const std::vector<Spec> &specs, uint64_t stride, uint64_t cut_packed, uint32_t cut_n) {
    std::vector<qgcm_gro_buf> bufs;
    uint64_t at = 0;
    uint32_t first = 0;
    for (const Spec &s : specs) {
        const uint64_t off = at + ((s.mod + 16 - at % 16) % 16);
        bufs.push_back(qgcm_gro_buf{(uint32_t)off, s.len, s.seg_len, first});
        first += (uint32_t)qgcm::gro_count(s.len, s.seg_len);
        at = off + s.len;
    }
    CHECK(qgcm::gro_table_ok(bufs.data(), (uint32_t)bufs.size(), first));
    const uint64_t packed_len = at - cut_packed;
    const uint32_t n = first - cut_n;
    std::vector<uint8_t> packed(packed_len);  // exactly: a read past it is the sanitizer's to find
    for (auto &b : packed) b = (uint8_t)rnd();
    std::vector<uint8_t> got(n * stride, 0xA5), want(n * stride, 0xA5);
    std::vector<uint32_t> got_lens(n, 0xDEADBEEFu), want_lens(n, 0xDEADBEEFu);
    contract(packed, packed_len, bufs, n, want, stride, want_lens);
    qgcm::gro_unpack_cpu(packed.data(), packed_len, bufs.data(), (uint32_t)bufs.size(), n, got.data(), stride, got_lens.data());
    CHECK(got == want);
    CHECK(got_lens == want_lens);
}

void test_unpack() {
    std::vector<Spec> specs;
    const uint32_t lengths[] = {0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 1382, 1471, 1472, 1473};
    for (uint32_t mod = 0; mod < 16; ++mod)
        for (uint32_t L : lengths) {
            specs.push_back({L, (mod & 1) ? L + 1 + mod : 0, mod});
            if (L) specs.push_back({3 * L + (L > 1 ? L - 1 : 1), L, (mod + 7) % 16});
            if (L > 1) specs.push_back({2 * L + 1, L, (mod + 3) % 16});
        }
    specs.push_back({64 * 1000, 1000, 5});
    specs.push_back({65535, 1024, 9});
    specs.push_back({1382, 0, 3});
    for (uint64_t stride : {1472ull, 1388ull, 64ull, 4ull}) {
        unpack_case(specs, stride, 0, 0);
        unpack_case(specs, stride, 1, 0);     // the last buffer reaches one byte past the packed area
        unpack_case(specs, stride, 70000, 0); // the last three lie past it, one of them partly
        unpack_case(specs, stride, 0, 1);     // the last buffer names a slot past n
    }
}

void test_table() {
    const qgcm_gro_buf ok[3] = {{0, 300, 100, 0}, {304, 77, 0, 3}, {384, 200, 300, 4}};
    CHECK(qgcm::gro_table_ok(ok, 3, 5));
    CHECK(!qgcm::gro_table_ok(ok, 3, 4) && !qgcm::gro_table_ok(ok, 3, 6) && !qgcm::gro_table_ok(ok, 2, 5));
    CHECK(qgcm::gro_table_ok(ok, 0, 0) && !qgcm::gro_table_ok(ok, 0, 1));
    qgcm_gro_buf bad[3] = {ok[0], ok[1], ok[2]};
    bad[1].first = 2;
    CHECK(!qgcm::gro_table_ok(bad, 3, 5));
    // counts of 2^32 - 1 each: the sum is kept in 64 bits
    const qgcm_gro_buf huge[2] = {{0, 0xffffffffu, 1, 0}, {0, 0xffffffffu, 1, 0xffffffffu}};
    CHECK(!qgcm::gro_table_ok(huge, 2, 0xfffffffeu));
    CHECK(qgcm::gro_count(0, 0) == 1 && qgcm::gro_count(0, 7) == 1 && qgcm::gro_count(7, 7) == 1 && qgcm::gro_count(8, 7) == 2 &&
          qgcm::gro_count(0xffffffffu, 0xfffffffeu) == 2);
}

struct Wire {
    int tx = -1, plain = -1, rx = -1;
    qgcm_peer_addr addr{};
    Wire() {
        tx = qgcm_udp_socket("127.0.0.1", 0, 1 << 22);
        plain = qgcm_udp_socket("127.0.0.1", 0, 1 << 22);
        rx = qgcm_udp_socket("127.0.0.1", 0, 1 << 22);
        CHECK(tx >= 0 && plain >= 0 && rx >= 0);
        const uint8_t ip[4] = {127, 0, 0, 1};
        memcpy(&addr.ip, ip, 4);
        const int port = qgcm_udp_port(rx);
        const uint8_t pb[2] = {(uint8_t)(port >> 8), (uint8_t)port};
        memcpy(&addr.port, pb, 2);
    }
    ~Wire() {
        qgcm_udp_close(tx);
        qgcm_udp_close(plain);
        qgcm_udp_close(rx);
    }
};

constexpr uint64_t kStride = 1472;

// trains of (count, seg_len) through the planned sender, the datagrams appended to `sent`
void send_trains(Wire &w, const std::vector<std::pair<uint32_t, uint32_t>> &shape, std::vector<std::vector<uint8_t>> &sent) {
    uint32_t n = 0;
    for (auto &s : shape) n += s.first;
    std::vector<uint8_t> arena(n * kStride);
    for (auto &b : arena) b = (uint8_t)rnd();
    std::vector<uint32_t> lens(n), order(n);
    std::vector<qgcm_train> trains;
    uint32_t at = 0;
    for (auto &s : shape) {
        trains.push_back(qgcm_train{at, s.first, 0, s.second});
        for (uint32_t k = 0; k < s.first; ++k, ++at) {
            lens[at] = s.second;
            order[at] = at;
            sent.emplace_back(arena.begin() + at * kStride, arena.begin() + at * kStride + s.second);
        }
    }
    CHECK(qgcm_udp_send_plan(w.tx, arena.data(), kStride, n, lens.data(), order.data(), n, trains.data(), (uint32_t)trains.size(),
                             &w.addr, 1, nullptr) == (int)n);
}

// calls of the given shape until `want` datagrams have come; every array exactly as large as the call is told
std::vector<std::vector<uint8_t>> drain(Wire &w, size_t want, uint64_t packed_cap, uint32_t max_bufs, uint32_t max_n) {
    std::vector<std::vector<uint8_t>> got;
    while (got.size() < want) {
        std::vector<uint8_t> packed(packed_cap);
        std::vector<qgcm_gro_buf> bufs(max_bufs);
        uint64_t out[3];
        const int n = qgcm_udp_recv_gro(w.rx, packed.data(), packed_cap, bufs.data(), max_bufs, max_n, 1000, out);
        CHECK(n > 0);
        if (n <= 0) break;
        CHECK((uint32_t)n <= max_n && out[0] >= 1 && out[0] <= max_bufs && out[1] <= packed_cap && out[2] == 0);
        CHECK(qgcm::gro_table_ok(bufs.data(), (uint32_t)out[0], (uint32_t)n));
        CHECK(out[1] == (uint64_t)bufs[out[0] - 1].off + bufs[out[0] - 1].len);
        for (uint64_t b = 0; b < out[0]; ++b) CHECK(bufs[b].off % 16 == 0);
        std::vector<uint8_t> arena((size_t)n * kStride);
        std::vector<uint32_t> lens((size_t)n, 0xDEADBEEFu);
        qgcm::gro_unpack_cpu(packed.data(), out[1], bufs.data(), (uint32_t)out[0], (uint32_t)n, arena.data(), kStride, lens.data());
        for (int i = 0; i < n; ++i) {
            CHECK(lens[i] <= kStride);
            if (lens[i] <= kStride) got.emplace_back(arena.begin() + i * kStride, arena.begin() + i * kStride + lens[i]);
        }
    }
    uint8_t none[65536];
    qgcm_gro_buf nb[1];
    uint64_t out[3] = {9, 9, 9};
    CHECK(qgcm_udp_recv_gro(w.rx, none, sizeof none, nb, 1, 64, 10, out) == 0 && out[0] == 0 && out[1] == 0 && out[2] == 0);
    return got;
}

void test_receive() {
    for (int gro = 0; gro < 2; ++gro) {
        struct Shape {
            uint64_t packed_cap;
            uint32_t max_bufs, max_n;
        };
        for (const Shape &sh : {Shape{1u << 20, 256, 1024}, Shape{65536 + 15, 4, 64}, Shape{1u << 18, 2, 100}}) {
            Wire w;
            CHECK(qgcm_udp_gro(w.rx, gro) == 0);
            std::vector<std::vector<uint8_t>> sent, plain;
            send_trains(w, {{45, 1382}, {1, 300}}, sent);
            // plain datagrams of lengths no train has, from a sender of their own
            for (uint32_t L : {0u, 1u, 77u}) {
                plain.emplace_back(L, (uint8_t)(L + 1));
                const uint8_t none = 0;
                CHECK(qgcm_udp_send_slots(w.plain, L ? plain.back().data() : &none, kStride, 1, &L, "127.0.0.1", qgcm_udp_port(w.rx)) == 1);
            }
            send_trains(w, {{64, 100}, {2, 200}}, sent);
            const auto got = drain(w, sent.size() + plain.size(), sh.packed_cap, sh.max_bufs, sh.max_n);
            std::vector<std::vector<uint8_t>> got_trains, got_plain;
            for (const auto &d : got) (d.size() == 0 || d.size() == 1 || d.size() == 77 ? got_plain : got_trains).push_back(d);
            CHECK(got_trains == sent);  // in order per sender
            CHECK(got_plain == plain);
        }
    }
    uint8_t buf[65536];
    qgcm_gro_buf nb[1];
    CHECK(qgcm_udp_recv_gro(-1, buf, sizeof buf, nb, 1, 64, 0, nullptr) == -1);
    CHECK(qgcm_udp_recv_gro(0, buf, sizeof buf - 1, nb, 1, 64, 0, nullptr) == -1);
    CHECK(qgcm_udp_recv_gro(0, buf, sizeof buf, nb, 0, 64, 0, nullptr) == -1);
    CHECK(qgcm_udp_recv_gro(0, buf, sizeof buf, nb, 1, 63, 0, nullptr) == -1);
    CHECK(qgcm_udp_recv_gro(0, nullptr, sizeof buf, nb, 1, 64, 0, nullptr) == -1);
    CHECK(qgcm_udp_gro(-1, 1) < 0);
}

}  // namespace

int main() {
    test_unpack();
    test_table();
    test_receive();
    if (failures) {
        fprintf(stderr, "gro_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("gro_san_driver ok");
    return 0;
}
