// pack_san_driver.cpp -- the host pack (pack_core.h, qgcm_deliver_pack_cpu) and the packed TUN write
// (qgcm_tun_write_packed) under the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program, no HIP, no Python.
//
//   1. the pack from arrays of exactly the size the contract names (the arena n * stride, the packed area
//      exactly packed_cap bytes, the table exactly m entries) against a byte-by-byte restatement: every length
//      around the pieces and the slot's end, dropped packets with garbage lengths, lengths that wrap, status
//      NULL, caps that cut at a record's start, inside it and at its end
//   2. the argument checks of qgcm_deliver_pack_cpu
//   3. qgcm_tun_write_packed over a datagram socket pair: order and bytes, a zero-length packet, tables that
//      reach past packed_len (nothing written), a write the kernel refuses
//
// Prints "pack_san_driver ok" and exits 0, or says what differed and exits 1.
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/pack_core.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED0071ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Batch {
    uint64_t stride;
    std::vector<uint8_t> arena, status;
    std::vector<uint32_t> lens, peer;
};

Batch edge_batch(uint64_t stride) {
    Batch b;
    b.stride = stride;
    const uint32_t s = (uint32_t)stride;
    const uint32_t lengths[] = {0, 1, 11, 12, 13, 27, 28, 29, 60, s - 5, s - 4};
    auto add = [&](uint8_t st, uint32_t L) {
        b.status.push_back(st);
        b.lens.push_back(L);
        b.peer.push_back(rnd());
    };
    add(0, 0xDEAD0000u);
    for (uint32_t L : lengths)
        if (L <= s - 4) add(1, L);
    add(1, s - 3);
    add(1, 0xffffffffu);
    add(1, 0xfffffffcu);
    add(2, 7);
    for (uint32_t L : lengths)
        if (L <= s - 4) {
            add(1, L);
            add(0, s * 3);
        }
    add(1, 5);
    add(0, 0);
    b.arena.resize(b.lens.size() * stride);  // exactly: a read past the last slot is the sanitizer's to find
    for (auto &x : b.arena) x = (uint8_t)rnd();
    return b;
}

// the contract, byte by byte
void contract(const Batch &b, bool with_status, uint64_t cap, std::vector<uint8_t> &packed, std::vector<qgcm_pack_rec> &recs,
              uint64_t counts[2]) {
    uint64_t at = 0;
    recs.clear();
    for (uint32_t i = 0; i < b.lens.size(); ++i) {
        const uint64_t L = b.lens[i];
        if ((with_status && b.status[i] != 1) || 4 + L > b.stride) continue;
        const uint64_t R = (4 + L + 15) / 16 * 16;
        const bool fits = at + R <= cap;
        recs.push_back(qgcm_pack_rec{fits ? (uint32_t)at : 0xffffffffu, (uint32_t)L, i, b.peer[i]});
        if (fits)
            for (uint64_t j = 0; j < R; ++j) packed[at + j] = j < 4 + L ? b.arena[i * b.stride + j] : 0;
        at += R;
    }
    counts[0] = recs.size();
    counts[1] = at;
}

bool same(const std::vector<qgcm_pack_rec> &a, const std::vector<qgcm_pack_rec> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), 16 * a.size()));
}

void pack_case(const Batch &b, bool with_status, uint64_t cap) {
    std::vector<uint8_t> want(cap, 0x5A), got(cap, 0x5A);  // exactly packed_cap bytes
    std::vector<qgcm_pack_rec> want_recs;
    uint64_t want_counts[2], counts[2] = {~0ull, ~0ull};
    contract(b, with_status, cap, want, want_recs, want_counts);
    std::vector<qgcm_pack_rec> recs(want_recs.size() ? want_recs.size() : 1);  // exactly m entries
    uint8_t none = 0;
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), b.stride, (uint32_t)b.lens.size(), b.lens.data(), b.peer.data(),
                                with_status ? b.status.data() : nullptr, cap ? got.data() : &none, cap, recs.data(),
                                counts) == QGCM_OK);
    recs.resize(want_recs.size());
    CHECK(counts[0] == want_counts[0] && counts[1] == want_counts[1]);
    CHECK(same(recs, want_recs));
    CHECK(got == want);
}

void test_pack() {
    for (uint64_t stride : {1536ull, 1388ull, 64ull, 16ull, 4ull}) {
        const Batch b = edge_batch(stride);
        std::vector<uint8_t> whole(b.arena.size() + 64);
        std::vector<qgcm_pack_rec> recs;
        uint64_t counts[2];
        contract(b, true, whole.size(), whole, recs, counts);
        CHECK(counts[0] >= 3 || stride == 4);
        pack_case(b, true, counts[1]);
        pack_case(b, true, counts[1] + 48);
        pack_case(b, false, b.arena.size() + 64);
        pack_case(b, true, 0);
        if (recs.size() >= 3) {
            const qgcm_pack_rec &r = recs[recs.size() / 2];
            const uint64_t R = qgcm::pack_rec_bytes(r.len);
            for (uint64_t cap : {(uint64_t)r.off, r.off + R - 1, r.off + R, (uint64_t)r.off + 1}) pack_case(b, true, cap);
        }
    }
}

void test_args() {
    const Batch b = edge_batch(64);
    std::vector<uint8_t> packed(4096);
    std::vector<qgcm_pack_rec> recs(b.lens.size());
    uint64_t counts[2] = {7, 7};
    const uint32_t n = (uint32_t)b.lens.size();
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 66, n, b.lens.data(), b.peer.data(), nullptr, packed.data(), 4096, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 0, n, b.lens.data(), b.peer.data(), nullptr, packed.data(), 4096, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 64, n, b.lens.data(), b.peer.data(), nullptr, packed.data(), 0xfffffff1ull, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(nullptr, 64, n, b.lens.data(), b.peer.data(), nullptr, packed.data(), 4096, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 64, n, nullptr, b.peer.data(), nullptr, packed.data(), 4096, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 64, n, b.lens.data(), nullptr, nullptr, packed.data(), 4096, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 64, n, b.lens.data(), b.peer.data(), nullptr, nullptr, 4096, recs.data(), counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 64, n, b.lens.data(), b.peer.data(), nullptr, packed.data(), 4096, nullptr, counts) == QGCM_E_ARG);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 64, n, b.lens.data(), b.peer.data(), nullptr, packed.data(), 4096, recs.data(), nullptr) == QGCM_E_ARG);
    CHECK(counts[0] == 7 && counts[1] == 7);
    CHECK(qgcm_deliver_pack_cpu(nullptr, 64, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, counts) == QGCM_OK);
    CHECK(counts[0] == 0 && counts[1] == 0);
}

// every datagram queued on fd, without blocking
std::vector<std::vector<uint8_t>> drain(int fd) {
    std::vector<std::vector<uint8_t>> got;
    uint8_t buf[4096];
    for (;;) {
        const ssize_t r = recv(fd, buf, sizeof buf, MSG_DONTWAIT);
        if (r < 0) break;
        got.emplace_back(buf, buf + r);
    }
    return got;
}

void test_tun_write() {
    const Batch b = edge_batch(1536);
    const uint32_t n = (uint32_t)b.lens.size();
    uint64_t counts[2];
    std::vector<uint8_t> probe(n * 1536);
    std::vector<qgcm_pack_rec> all(n);
    CHECK(qgcm_deliver_pack_cpu(b.arena.data(), 1536, n, b.lens.data(), b.peer.data(), b.status.data(), probe.data(), probe.size(),
                                all.data(), counts) == QGCM_OK);
    const uint32_t m = (uint32_t)counts[0];
    std::vector<uint8_t> packed(probe.begin(), probe.begin() + counts[1]);  // exactly packed_len bytes
    std::vector<qgcm_pack_rec> recs(all.begin(), all.begin() + m);          // exactly m entries
    std::vector<std::vector<uint8_t>> want;
    for (const qgcm_pack_rec &r : recs) want.emplace_back(b.arena.begin() + r.slot * 1536 + 4, b.arena.begin() + r.slot * 1536 + 4 + r.len);
    int sv[2];
    CHECK(socketpair(AF_UNIX, SOCK_DGRAM, 0, sv) == 0);
    std::vector<std::vector<uint8_t>> got;
    for (uint32_t k = 0; k < m; k += 8) {  // a datagram socket queues about ten: eight records a call
        const uint32_t c = m - k < 8 ? m - k : 8;
        CHECK(qgcm_tun_write_packed(sv[0], packed.data(), packed.size(), recs.data() + k, c) == (int)c);
        for (auto &d : drain(sv[1])) got.push_back(d);
    }
    CHECK(got == want);
    // tables that reach past packed_len: -1, nothing written
    std::vector<qgcm_pack_rec> bad = recs;
    bad[m / 2].off = (uint32_t)packed.size();
    CHECK(qgcm_tun_write_packed(sv[0], packed.data(), packed.size(), bad.data(), m) == -1);
    bad = recs;
    bad[m - 1].off = 0xffffffffu;
    CHECK(qgcm_tun_write_packed(sv[0], packed.data(), packed.size(), bad.data(), m) == -1);
    bad = recs;
    bad[0].len = 0xfffffffcu;
    CHECK(qgcm_tun_write_packed(sv[0], packed.data(), packed.size(), bad.data(), m) == -1);
    CHECK(qgcm_tun_write_packed(sv[0], packed.data(), recs[m - 1].off + 4 + recs[m - 1].len - 1, recs.data(), m) == -1);
    CHECK(qgcm_tun_write_packed(-1, packed.data(), packed.size(), recs.data(), m) == -1);
    CHECK(qgcm_tun_write_packed(sv[0], nullptr, packed.size(), recs.data(), m) == -1);
    CHECK(qgcm_tun_write_packed(sv[0], packed.data(), packed.size(), nullptr, 0) == 0);
    CHECK(drain(sv[1]).empty());
    // a write the kernel refuses ends the batch there: the queue of a socket nobody reads fills up
    CHECK(fcntl(sv[0], F_SETFL, O_NONBLOCK) == 0);
    const int done = qgcm_tun_write_packed(sv[0], packed.data(), packed.size(), recs.data(), m);
    CHECK(done > 0 && done <= (int)m);
    got = drain(sv[1]);
    CHECK((int)got.size() == done && std::vector<std::vector<uint8_t>>(want.begin(), want.begin() + done) == got);
    close(sv[0]);
    close(sv[1]);
}

}  // namespace

int main() {
    test_pack();
    test_args();
    test_tun_write();
    if (failures) {
        fprintf(stderr, "pack_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("pack_san_driver ok");
    return 0;
}
