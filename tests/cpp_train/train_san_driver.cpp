// train_san_driver.cpp -- the train pack's host code (train_core.h, qgcm_train_pack_cpu) and the packed sender
// (qgcm_udp_send_packed) under the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program, no HIP, no Python.
//
//   1. the pack from arrays of exactly the size the contract names (the arena n * stride, order exactly m, the
//      tables exactly t, the packed area exactly packed_cap bytes) against a byte-by-byte restatement, over plans
//      the host planner makes: every segment length around the 4- and 16-byte pieces and the slot's end, caps
//      that cut at a train's start, inside it, at its end and off the 16-byte grid
//   2. every class of plan that is not well-formed, and the argument checks: QGCM_E_ARG, nothing written
//   3. qgcm_udp_send_packed over loopback: the datagrams arrive in table order (segmented, and again with
//      QGCM_UDP_GSO=0), and every table the check refuses sends nothing
//
// Prints "train_san_driver ok" and exits 0, or says what differed and exits 1.
#include <arpa/inet.h>
#include <netinet/in.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/send_plan_core.h"
#include "../../quantum_amd/csrc/train_core.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED0072ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Batch {
    uint64_t stride;
    uint32_t n, max_keys;
    std::vector<uint8_t> arena;
    std::vector<uint32_t> lens, peer, order;  // order exactly m entries
    std::vector<qgcm_train> trains;           // exactly t entries
};

// per segment length one peer with 1, 2, 3 and 17 datagrams of it (a peer each), interleaved; a few unsendable
Batch edge_batch(uint64_t stride, uint32_t max_segs) {
    Batch b;
    b.stride = stride;
    const uint32_t s = (uint32_t)stride;
    const uint32_t segs[] = {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, s - 1, s};
    const uint32_t counts[] = {1, 2, 3, 17};
    uint32_t key = 0;
    std::vector<uint32_t> lens, peer;
    for (uint32_t seg : segs)
        if (seg >= 1 && seg <= s)
            for (uint32_t c : counts) {
                for (uint32_t k = 0; k < c; ++k) {
                    lens.push_back(seg);
                    peer.push_back(key);
                }
                ++key;
            }
    lens.push_back(0);
    peer.push_back(0);
    lens.push_back(40);
    peer.push_back(QGCM_NO_PEER);
    b.n = (uint32_t)lens.size();
    b.max_keys = key;
    // a seeded shuffle: peers interleave
    std::vector<uint32_t> at(b.n);
    for (uint32_t i = 0; i < b.n; ++i) at[i] = i;
    for (uint32_t i = b.n - 1; i > 0; --i) {
        const uint32_t j = rnd() % (i + 1);
        const uint32_t x = at[i];
        at[i] = at[j];
        at[j] = x;
    }
    b.lens.resize(b.n);
    b.peer.resize(b.n);
    for (uint32_t i = 0; i < b.n; ++i) {
        b.lens[i] = lens[at[i]];
        b.peer[i] = peer[at[i]];
    }
    b.arena.resize((size_t)b.n * stride);  // exactly: a read past the last slot is the sanitizer's to find
    for (auto &x : b.arena) x = (uint8_t)rnd();
    std::vector<uint32_t> order(b.n);
    std::vector<qgcm_train> trains(b.n);
    uint32_t plan_counts[2];
    const qgcm_plan_limits asked{max_segs, 0, 0};
    qgcm_plan_limits lim;
    CHECK(qgcm::plan_limits_resolve(&asked, &lim));
    qgcm::send_plan_cpu(b.n, b.lens.data(), b.peer.data(), b.max_keys, lim, order.data(), trains.data(), plan_counts);
    b.order.assign(order.begin(), order.begin() + plan_counts[0]);
    b.trains.assign(trains.begin(), trains.begin() + plan_counts[1]);
    return b;
}

// the contract, byte by byte
void contract(const Batch &b, uint64_t cap, std::vector<uint8_t> &packed, std::vector<qgcm_ptrain> &pt, uint64_t pcounts[2]) {
    uint64_t at = 0;
    pt.clear();
    for (const qgcm_train &tr : b.trains) {
        const uint64_t used = (uint64_t)tr.count * tr.seg_len, R = (used + 15) / 16 * 16;
        const bool fits = at + R <= cap;
        pt.push_back(qgcm_ptrain{fits ? (uint32_t)at : 0xffffffffu, tr.count, tr.peer, tr.seg_len});
        if (fits)
            for (uint64_t j = 0; j < R; ++j)
                packed[at + j] = j < used ? b.arena[(uint64_t)b.order[tr.first + j / tr.seg_len] * b.stride + j % tr.seg_len] : 0;
        at += R;
    }
    pcounts[0] = pt.size();
    pcounts[1] = at;
}

bool same(const std::vector<qgcm_ptrain> &a, const std::vector<qgcm_ptrain> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), 16 * a.size()));
}

int pack(const Batch &b, const std::vector<uint32_t> &order, uint32_t m, const std::vector<qgcm_train> &trains, uint32_t t,
         std::vector<uint8_t> &packed, std::vector<qgcm_ptrain> &pt, uint64_t pcounts[2]) {
    uint8_t none = 0;
    return qgcm_train_pack_cpu(b.arena.data(), b.stride, b.n, order.data(), m, trains.data(), t,
                               packed.empty() ? &none : packed.data(), packed.size(), pt.data(), pcounts);
}

void pack_case(const Batch &b, uint64_t cap) {
    std::vector<uint8_t> want(cap, 0x5A), got(cap, 0x5A);  // exactly packed_cap bytes
    std::vector<qgcm_ptrain> want_pt;
    uint64_t want_counts[2], pcounts[2] = {~0ull, ~0ull};
    contract(b, cap, want, want_pt, want_counts);
    std::vector<qgcm_ptrain> pt(want_pt.size() ? want_pt.size() : 1);  // exactly t entries
    CHECK(pack(b, b.order, (uint32_t)b.order.size(), b.trains, (uint32_t)b.trains.size(), got, pt, pcounts) == QGCM_OK);
    pt.resize(want_pt.size());
    CHECK(pcounts[0] == want_counts[0] && pcounts[1] == want_counts[1]);
    CHECK(same(pt, want_pt));
    CHECK(got == want);
}

void test_pack() {
    for (uint64_t stride : {1536ull, 1388ull, 64ull, 16ull, 4ull})
        for (uint32_t max_segs : {64u, 2u}) {
            const Batch b = edge_batch(stride, max_segs);
            CHECK(qgcm::train_plan_ok(b.stride, b.n, b.order.data(), (uint32_t)b.order.size(), b.trains.data(), (uint32_t)b.trains.size()));
            std::vector<uint8_t> whole(b.arena.size() + 16 * b.n);  // a train of one byte is 16
            std::vector<qgcm_ptrain> pt;
            uint64_t pcounts[2];
            contract(b, whole.size(), whole, pt, pcounts);
            CHECK(pt.size() >= 8);
            pack_case(b, pcounts[1]);
            pack_case(b, pcounts[1] + 48);
            pack_case(b, 0);
            const qgcm_ptrain &r = pt[pt.size() / 2];
            const uint64_t R = qgcm::train_bytes(r.count, r.seg_len);
            for (uint64_t cap : {(uint64_t)r.off, r.off + R - 1, r.off + R, (uint64_t)r.off + 1, r.off + R + 7}) pack_case(b, cap);
        }
}

void test_refusals() {
    const Batch b = edge_batch(64, 64);
    const uint32_t m = (uint32_t)b.order.size(), t = (uint32_t)b.trains.size();
    uint32_t big = 0;
    while (b.trains[big].count < 3) ++big;
    auto refused = [&](std::vector<uint32_t> order, uint32_t mm, std::vector<qgcm_train> trains, uint32_t tt) {
        std::vector<uint8_t> packed(b.arena.size(), 0x5A);
        std::vector<qgcm_ptrain> pt(b.n, qgcm_ptrain{7, 7, 7, 7});
        uint64_t pcounts[2] = {7, 7};
        const int rc = pack(b, order, mm, trains, tt, packed, pt, pcounts);
        bool clean = pcounts[0] == 7 && pcounts[1] == 7;
        for (uint8_t x : packed) clean = clean && x == 0x5A;
        for (const qgcm_ptrain &p : pt) clean = clean && p.off == 7 && p.seg_len == 7;
        return rc == QGCM_E_ARG && clean;
    };
    auto with = [&](uint32_t j, uint32_t qgcm_train::*field, uint32_t v) {
        std::vector<qgcm_train> tr = b.trains;
        tr[j].*field = v;
        return tr;
    };
    CHECK(refused(b.order, m, with(big, &qgcm_train::count, 0), t));
    CHECK(refused(b.order, m, with(big, &qgcm_train::count, 1025), t));
    CHECK(refused(b.order, m, with(big, &qgcm_train::count, b.trains[big].count - 1), t));  // a gap
    CHECK(refused(b.order, m, with(big, &qgcm_train::seg_len, 0), t));
    CHECK(refused(b.order, m, with(big, &qgcm_train::seg_len, 68), t));
    CHECK(refused(b.order, m, with(big, &qgcm_train::first, 0xffffffffu), t));  // first + count wraps 32 bits
    CHECK(refused(b.order, m, with(t - 1, &qgcm_train::count, b.trains[t - 1].count + 1), t));
    CHECK(refused(b.order, m, std::vector<qgcm_train>(b.trains.begin(), b.trains.end() - 1), t - 1));  // short of m
    CHECK(refused(b.order, m - 1, b.trains, t));
    std::vector<uint32_t> order = b.order;
    order[b.trains[big].first + 1] = b.n;
    CHECK(refused(order, m, b.trains, t));
    order[b.trains[big].first + 1] = 0xffffffffu;
    CHECK(refused(order, m, b.trains, t));
    std::vector<uint32_t> long_order(b.n + 1, 0);
    CHECK(refused(long_order, b.n + 1, b.trains, t));  // m > n
    CHECK(refused(std::vector<uint32_t>(b.order.begin(), b.order.begin() + 1), 1,
                  std::vector<qgcm_train>(b.trains.begin(), b.trains.begin() + 2), 2));  // t > m
    // the argument checks
    std::vector<uint8_t> packed(4096);
    std::vector<qgcm_ptrain> pt(b.n);
    uint64_t pcounts[2] = {7, 7};
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 66, b.n, b.order.data(), m, b.trains.data(), t, packed.data(), 4096, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 0, b.n, b.order.data(), m, b.trains.data(), t, packed.data(), 4096, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 64, b.n, b.order.data(), m, b.trains.data(), t, packed.data(), 0xfffffff1ull, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(nullptr, 64, b.n, b.order.data(), m, b.trains.data(), t, packed.data(), 4096, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 64, b.n, nullptr, m, b.trains.data(), t, packed.data(), 4096, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 64, b.n, b.order.data(), m, nullptr, t, packed.data(), 4096, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 64, b.n, b.order.data(), m, b.trains.data(), t, nullptr, 4096, pt.data(), pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 64, b.n, b.order.data(), m, b.trains.data(), t, packed.data(), 4096, nullptr, pcounts) == QGCM_E_ARG);
    CHECK(qgcm_train_pack_cpu(b.arena.data(), 64, b.n, b.order.data(), m, b.trains.data(), t, packed.data(), 4096, pt.data(), nullptr) == QGCM_E_ARG);
    CHECK(pcounts[0] == 7 && pcounts[1] == 7);
    CHECK(qgcm_train_pack_cpu(nullptr, 64, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, pcounts) == QGCM_OK);
    CHECK(pcounts[0] == 0 && pcounts[1] == 0);
}

// every datagram queued on fd; the first may take a moment to cross loopback
std::vector<std::vector<uint8_t>> drain(int fd, size_t want) {
    std::vector<std::vector<uint8_t>> got;
    std::vector<uint8_t> buf(65536);
    timeval tv{want ? 1 : 0, want ? 0 : 20000};
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    while (got.size() < want + 4) {
        if (got.size() == want) {
            tv = timeval{0, 20000};
            setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
        }
        const ssize_t r = recv(fd, buf.data(), buf.size(), 0);
        if (r < 0) break;
        got.emplace_back(buf.begin(), buf.begin() + r);
    }
    return got;
}

void test_send() {
    const Batch b = edge_batch(256, 16);
    const uint32_t t = (uint32_t)b.trains.size();
    std::vector<uint8_t> probe(b.arena.size());
    std::vector<qgcm_ptrain> all(b.n);
    uint64_t pcounts[2];
    CHECK(pack(b, b.order, (uint32_t)b.order.size(), b.trains, t, probe, all, pcounts) == QGCM_OK);
    std::vector<uint8_t> packed(probe.begin(), probe.begin() + pcounts[1]);  // exactly packed_len bytes
    std::vector<qgcm_ptrain> pt(all.begin(), all.begin() + t);               // exactly t entries
    // one receiver; every peer's address is its
    const int rx = qgcm_udp_socket("127.0.0.1", 0, 1 << 22), tx = qgcm_udp_socket("127.0.0.1", 0, 1 << 22);
    CHECK(rx >= 0 && tx >= 0);
    qgcm_peer_addr addr{};
    addr.ip = inet_addr("127.0.0.1");
    addr.port = htons((uint16_t)qgcm_udp_port(rx));
    std::vector<qgcm_peer_addr> addrs(b.max_keys, addr);  // exactly n_addrs entries
    std::vector<std::vector<uint8_t>> want;
    for (uint32_t p = 0; p < b.order.size(); ++p)
        want.emplace_back(b.arena.begin() + (size_t)b.order[p] * b.stride, b.arena.begin() + (size_t)b.order[p] * b.stride + b.lens[b.order[p]]);
    uint64_t stats[3];
    for (int gso = 1; gso >= 0; --gso) {
        setenv("QGCM_UDP_GSO", gso ? "1" : "0", 1);
        CHECK(qgcm_udp_send_packed(tx, packed.data(), packed.size(), pt.data(), t, addrs.data(), b.max_keys, stats) == (int)want.size());
        CHECK(drain(rx, want.size()) == want);  // one sender, one receiver: table order
        if (!gso) CHECK(stats[0] == want.size() && stats[1] == 0 && stats[2] == 0);
    }
    unsetenv("QGCM_UDP_GSO");
    // tables the check refuses: -1, nothing sent
    auto refused = [&](uint32_t j, uint32_t qgcm_ptrain::*field, uint32_t v, uint64_t len, uint32_t n_addrs) {
        std::vector<qgcm_ptrain> bad = pt;
        bad[j].*field = v;
        return qgcm_udp_send_packed(tx, packed.data(), len, bad.data(), t, addrs.data(), n_addrs, stats) == -1 && stats[0] == 0;
    };
    uint32_t big = 0;
    while (pt[big].count < 3) ++big;
    CHECK(refused(big, &qgcm_ptrain::off, 0xffffffffu, packed.size(), b.max_keys));  // a train that did not fit
    CHECK(refused(t - 1, &qgcm_ptrain::off, pt[t - 1].off + 16, packed.size(), b.max_keys));
    CHECK(refused(0, &qgcm_ptrain::off, pt[0].off, pt[t - 1].off + pt[t - 1].count * pt[t - 1].seg_len - 1, b.max_keys));
    CHECK(refused(big, &qgcm_ptrain::count, 0, packed.size(), b.max_keys));
    CHECK(refused(big, &qgcm_ptrain::count, 1025, packed.size(), b.max_keys));
    CHECK(refused(big, &qgcm_ptrain::seg_len, 0, packed.size(), b.max_keys));
    CHECK(refused(big, &qgcm_ptrain::seg_len, 0xffffffffu, packed.size(), b.max_keys));  // count * seg_len in 64 bits
    CHECK(refused(big, &qgcm_ptrain::peer, b.max_keys, packed.size(), b.max_keys));
    CHECK(refused(0, &qgcm_ptrain::off, pt[0].off, packed.size(), pt[t - 1].peer));  // a peer at n_addrs
    // a segment size travels as 16 bits: no train of two 65536-byte datagrams, though one alone is a valid entry
    std::vector<uint8_t> wide(2 * 65536);
    qgcm_ptrain two{0, 2, 0, 65536}, one{0, 1, 0, 65536};
    CHECK(qgcm_udp_send_packed(tx, wide.data(), wide.size(), &two, 1, addrs.data(), 1, stats) == -1);
    CHECK(qgcm::train_table_ok(&one, 1, wide.size(), 1));
    CHECK(qgcm_udp_send_packed(-1, packed.data(), packed.size(), pt.data(), t, addrs.data(), b.max_keys, stats) == -1);
    CHECK(qgcm_udp_send_packed(tx, nullptr, packed.size(), pt.data(), t, addrs.data(), b.max_keys, stats) == -1);
    CHECK(qgcm_udp_send_packed(tx, packed.data(), packed.size(), nullptr, 0, addrs.data(), b.max_keys, stats) == 0);
    CHECK(drain(rx, 0).empty());
    qgcm_udp_close(rx);
    qgcm_udp_close(tx);
}

}  // namespace

int main() {
    test_pack();
    test_refusals();
    test_send();
    if (failures) {
        fprintf(stderr, "train_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("train_san_driver ok");
    return 0;
}
