// plan_san_driver.cpp -- the host planner (send_plan_core.h) and the planned sender (udp_batch.cpp) under the
// host compiler's AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no HIP, no Python.
//
//   1. the planner against a restatement of the contract with std::stable_sort, over seeded batches and
//      every number of sort passes (max_keys 200, 2048, 2^20 - 1)
//   2. a planned batch of three peers over loopback: each receiver gets its peer's datagrams in arena order
//   3. a train of 200 datagrams, which no kernel takes as one message, arrives as singles
//   4. plans that do not fit their batch return -1 and send nothing
//
// Prints "plan_san_driver ok" and exits 0, or says what differed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/send_plan_core.h"

namespace {

constexpr uint64_t kStride = 1472;
int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED0051ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Plan {
    std::vector<uint32_t> order;
    std::vector<qgcm_train> trains;
};

Plan contract(const std::vector<uint32_t> &lens, const std::vector<uint32_t> &peer, uint32_t max_keys,
              const qgcm_plan_limits &lim) {
    Plan p;
    for (uint32_t i = 0; i < lens.size(); ++i)
        if (peer[i] < max_keys && lens[i] != 0) p.order.push_back(i);
    std::stable_sort(p.order.begin(), p.order.end(), [&](uint32_t a, uint32_t b) { return peer[a] < peer[b]; });
    for (uint32_t at = 0; at < p.order.size();) {
        const uint32_t pr = peer[p.order[at]], len = lens[p.order[at]];
        uint32_t end = at;
        while (end < p.order.size() && peer[p.order[end]] == pr && lens[p.order[end]] == len) ++end;
        const uint32_t cap = len > lim.max_seg_len ? 1u : std::max(1u, std::min(lim.max_segs, lim.max_bytes / len));
        for (; at < end; at += std::min(cap, end - at)) p.trains.push_back(qgcm_train{at, std::min(cap, end - at), pr, len});
    }
    return p;
}

Plan planner(const std::vector<uint32_t> &lens, const std::vector<uint32_t> &peer, uint32_t max_keys,
             const qgcm_plan_limits &lim) {
    const uint32_t n = (uint32_t)lens.size();
    Plan p;
    // exactly n entries each: the sanitizer sees any write past them
    p.order.resize(n);
    p.trains.resize(n);
    uint32_t counts[2] = {7, 7};
    qgcm::send_plan_cpu(n, lens.data(), peer.data(), max_keys, lim, p.order.data(), p.trains.data(), counts);
    CHECK(counts[0] <= n && counts[1] <= counts[0]);
    p.order.resize(counts[0]);
    p.trains.resize(counts[1]);
    return p;
}

bool same(const Plan &a, const Plan &b) {
    return a.order == b.order && a.trains.size() == b.trains.size() &&
           (a.trains.empty() || !memcmp(a.trains.data(), b.trains.data(), a.trains.size() * sizeof(qgcm_train)));
}

void test_planner() {
    const uint32_t lengths[] = {36, 700, 1382, 0, 9000};
    const qgcm_plan_limits limits[] = {{0, 0, 0}, {7, 0, 0}, {0, 1000, 0}, {0, 0, 1000}, {1, 0, 0}, {1024, 0, 0}};
    for (uint32_t max_keys : {200u, 2048u, (1u << 20) - 1u})
        for (uint32_t n : {0u, 1u, 63u, 257u, 4099u})
            for (const qgcm_plan_limits &in : limits) {
                qgcm_plan_limits lim;
                CHECK(qgcm::plan_limits_resolve(&in, &lim));
                std::vector<uint32_t> lens(n), peer(n);
                const uint32_t spread = 1 + rnd() % 40;
                for (uint32_t i = 0; i < n; ++i) {
                    lens[i] = lengths[rnd() % 5];
                    const uint32_t r = rnd() % 16;
                    peer[i] = r == 0 ? QGCM_NO_PEER : r == 1 ? max_keys + rnd() % 3 : max_keys - 1 - (rnd() % spread) * (max_keys / 64);
                }
                CHECK(same(planner(lens, peer, max_keys, lim), contract(lens, peer, max_keys, lim)));
            }
    qgcm_plan_limits bad{1025, 0, 0}, out;
    CHECK(!qgcm::plan_limits_resolve(&bad, &out));
    bad = {0, 0, 65508};
    CHECK(!qgcm::plan_limits_resolve(&bad, &out));
    CHECK(qgcm::plan_limits_resolve(nullptr, &out) && out.max_segs == 64 && out.max_seg_len == 65507 && out.max_bytes == 65507);
}

struct Wire {
    int tx = -1, rx[3] = {-1, -1, -1};
    qgcm_peer_addr addrs[3];
    Wire() {
        tx = qgcm_udp_socket("127.0.0.1", 0, 1 << 22);
        for (int p = 0; p < 3; ++p) {
            rx[p] = qgcm_udp_socket("127.0.0.1", 0, 1 << 22);
            const uint8_t ip[4] = {127, 0, 0, 1};
            memcpy(&addrs[p].ip, ip, 4);
            const int port = qgcm_udp_port(rx[p]);
            const uint8_t pb[2] = {(uint8_t)(port >> 8), (uint8_t)port};
            memcpy(&addrs[p].port, pb, 2);
            addrs[p].pad = 0;
        }
        CHECK(tx >= 0 && rx[0] >= 0 && rx[1] >= 0 && rx[2] >= 0);
    }
    ~Wire() {
        qgcm_udp_close(tx);
        for (int fd : rx) qgcm_udp_close(fd);
    }
    // peer p's queue equals its datagrams of the batch, in arena order
    void expect(int p, const std::vector<uint8_t> &arena, const std::vector<uint32_t> &lens, const std::vector<uint32_t> &peer) {
        std::vector<uint32_t> want;
        for (uint32_t i = 0; i < lens.size(); ++i)
            if (peer[i] == (uint32_t)p && lens[i] != 0) want.push_back(i);
        std::vector<uint8_t> buf((want.size() + 4) * kStride);
        std::vector<uint32_t> got_lens(want.size() + 4);
        uint32_t got = 0;
        while (got < want.size() + 4) {
            const int r = qgcm_udp_recv_slots(rx[p], buf.data() + got * kStride, kStride, (uint32_t)want.size() + 4 - got,
                                              got_lens.data() + got, got < want.size() ? 1000 : 10);
            if (r <= 0) break;
            got += (uint32_t)r;
        }
        CHECK(got == want.size());
        for (uint32_t k = 0; k < std::min<size_t>(got, want.size()); ++k)
            CHECK(got_lens[k] == lens[want[k]] && !memcmp(buf.data() + k * kStride, arena.data() + want[k] * kStride, got_lens[k]));
    }
    bool quiet() {
        uint8_t buf[kStride];
        uint32_t len;
        for (int fd : rx)
            if (qgcm_udp_recv_slots(fd, buf, kStride, 1, &len, 10) != 0) return false;
        return true;
    }
};

void fill(std::vector<uint8_t> &arena) {
    for (auto &b : arena) b = (uint8_t)rnd();
}

void test_round_trip_and_validation() {
    const uint32_t n = 90;
    std::vector<uint8_t> arena(n * kStride);
    fill(arena);
    std::vector<uint32_t> lens(n), peer(n);
    const uint32_t mix[3] = {36, 700, 1382};
    for (uint32_t i = 0; i < n; ++i) {
        lens[i] = mix[(i / 12) % 3];
        peer[i] = i % 3;
    }
    lens[20] = 64;
    lens[7] = lens[40] = 0;
    peer[13] = peer[61] = QGCM_NO_PEER;
    qgcm_plan_limits lim;
    qgcm::plan_limits_resolve(nullptr, &lim);
    const Plan p = planner(lens, peer, 3, lim);
    const uint32_t m = (uint32_t)p.order.size(), t = (uint32_t)p.trains.size();
    Wire w;
    uint64_t stats[3];
    auto send = [&](const std::vector<uint32_t> &ln, const std::vector<uint32_t> &order, const std::vector<qgcm_train> &trains,
                    uint32_t n_addrs, uint64_t stride = kStride) {
        return qgcm_udp_send_plan(w.tx, arena.data(), stride, n, ln.data(), order.data(), (uint32_t)order.size(), trains.data(),
                                  (uint32_t)trains.size(), w.addrs, n_addrs, stats);
    };
    CHECK(send(lens, p.order, p.trains, 3) == (int)m);
    CHECK(stats[0] + stats[2] >= t);
    for (int q = 0; q < 3; ++q) w.expect(q, arena, lens, peer);
    setenv("QGCM_UDP_GSO", "0", 1);
    CHECK(send(lens, p.order, p.trains, 3) == (int)m);
    CHECK(stats[0] == m && stats[1] == 0 && stats[2] == 0);
    unsetenv("QGCM_UDP_GSO");
    for (int q = 0; q < 3; ++q) w.expect(q, arena, lens, peer);

    // validation: nothing leaves
    uint32_t big = 0;
    while (p.trains[big].count < 3) ++big;
    {
        auto ln = lens;
        ln[p.order[p.trains[big].first + 1]] -= 1;
        CHECK(send(ln, p.order, p.trains, 3) == -1);
    }
    {
        auto order = p.order;
        order[0] = n;
        CHECK(send(lens, order, p.trains, 3) == -1);
    }
    auto with_train = [&](uint32_t k, qgcm_train tr) {
        auto trains = p.trains;
        trains[k] = tr;
        return send(lens, p.order, trains, 3);
    };
    qgcm_train tr = p.trains[t - 1];
    tr.count += 1;
    CHECK(with_train(t - 1, tr) == -1);  // past m
    tr = p.trains[big];
    tr.first = 0xffffffffu;
    CHECK(with_train(big, tr) == -1);
    tr = p.trains[big];
    tr.peer = 3;
    CHECK(with_train(big, tr) == -1);
    CHECK(send(lens, p.order, p.trains, 2) == -1);
    tr = p.trains[big];
    tr.count = 0;
    CHECK(with_train(big, tr) == -1);
    tr.count = 1025;
    CHECK(with_train(big, tr) == -1);
    tr = p.trains[big];
    tr.seg_len += 1;
    CHECK(with_train(big, tr) == -1);
    CHECK(send(lens, p.order, p.trains, 3, 64) == -1);  // longer than the slot
    CHECK(w.quiet());
}

void test_fallback() {
    const uint32_t n = 220;
    std::vector<uint8_t> arena(n * kStride);
    fill(arena);
    std::vector<uint32_t> lens(n, 20), peer(n), order(n);
    std::iota(order.begin(), order.end(), 0u);
    for (uint32_t i = 0; i < n; ++i) peer[i] = i < 10 ? 0 : i < 210 ? 1 : 2;
    const qgcm_train trains[3] = {{0, 10, 0, 20}, {10, 200, 1, 20}, {210, 10, 2, 20}};
    Wire w;
    uint64_t stats[3];
    CHECK(qgcm_udp_send_plan(w.tx, arena.data(), kStride, n, lens.data(), order.data(), n, trains, 3, w.addrs, 3, stats) == (int)n);
    CHECK(stats[2] >= 1 && stats[0] >= 202);
    for (int q = 0; q < 3; ++q) w.expect(q, arena, lens, peer);
}

}  // namespace

int main() {
    test_planner();
    test_round_trip_and_validation();
    test_fallback();
    if (failures) {
        fprintf(stderr, "plan_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("plan_san_driver ok");
    return 0;
}
