// coalesce_san_driver.cpp -- the coalescing's host code (coalesce_core.h: the candidate and link rules, the frame
// arithmetic, the table check and qgcm_deliver_coalesce_cpu's body; tun_batch.cpp: qgcm_tun_write_gso and its
// fallback segmentation) under the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone
// program, no HIP, no Python.
//
//   1. the coalescing from heap arrays of exactly the size the contract names (the arena exactly n * stride with
//      the longest packets ending on their slot's last byte, lens, peer and status exactly n, the table exactly n
//      entries, the packed area exactly counts[1] bytes, and once more one byte short): segments that
//      gso_unpack_entry_cpu cut from super-frames come back as those super-frames; random bytes of every short length
//      between them are parsed inside their length
//   2. the table check of qgcm_tun_write_gso: every class of entry it refuses, nothing written
//   3. qgcm_tun_write_gso on a datagram socketpair: one message an entry, vnet header in front; and the fallback
//      segmentation: one message a segment behind ten zero bytes, the segments gso_unpack_entry_cpu makes
//
// Prints "coalesce_san_driver ok" and exits 0, or says what differed and exits 1.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/coalesce_core.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED0C0Aull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

struct Super {
    std::vector<uint8_t> packed;  // the lead and the packet, padded to 16
    qgcm_gso_frame f;
};

// a TCP4 super-frame of `count` segments (the last of `tail` bytes) with valid headers, as a coalesced entry is laid out
Super make_super(uint32_t ihl, uint32_t doff, uint32_t gso, uint32_t count, uint32_t tail, bool psh) {
    Super s;
    const uint32_t hdr = ihl + doff, len = hdr + (count - 1) * gso + tail;
    s.packed.assign(16 + ((len + 15) & ~15u), 0);
    uint8_t *p = s.packed.data() + 16;
    for (uint32_t i = 0; i < len; ++i) p[i] = (uint8_t)rnd();
    p[0] = (uint8_t)(0x40 | ihl >> 2);
    qgcm::gso_put16(p + 2, len);
    qgcm::gso_put16(p + 4, 0xfffe);  // the id wraps
    qgcm::gso_put16(p + 6, 0x4000);
    p[9] = 6;
    p[ihl + 4] = p[ihl + 5] = p[ihl + 6] = 0xff;  // the sequence number wraps
    p[ihl + 12] = (uint8_t)(doff >> 2 << 4);
    p[ihl + 13] = (uint8_t)(0x10 | (psh ? 8 : 0));
    s.f = qgcm_gso_frame{16, len, 0, count, (uint16_t)gso, (uint16_t)hdr, (uint16_t)ihl, 16, QGCM_GSO_TCP4, 0};
    return s;
}

void test_round_trip(uint64_t stride) {
    struct Spec { uint32_t ihl, doff, gso, count, tail; bool psh; };
    const Spec specs[] = {{20, 20, (uint32_t)stride - 44, 3, (uint32_t)stride - 44, false}, {24, 32, 17, 64, 17, true},
                          {20, 20, 31, 64, 5, false}, {60, 60, 1, 7, 1, true}, {20, 60, 33, 2, 32, false}, {20, 20, 5, 2, 5, false}};
    std::vector<Super> supers;
    uint32_t n = 0;
    std::vector<uint32_t> first;
    for (const Spec &sp : specs) {
        if (4 + sp.ihl + sp.doff + sp.gso > stride) continue;
        supers.push_back(make_super(sp.ihl, sp.doff, sp.gso, sp.count, sp.tail, sp.psh));
        first.push_back(n);
        n += sp.count + 5;  // five slots of random bytes behind every frame's segments
    }
    std::vector<uint8_t> arena((size_t)(n * stride));
    std::vector<uint32_t> lens(n), peer(n, 9);
    std::vector<uint8_t> status(n, 1);
    for (auto &b : arena) b = (uint8_t)rnd();
    const uint32_t odd[5] = {0, 1, 39, 40, (uint32_t)stride - 4};
    for (size_t k = 0; k < supers.size(); ++k) {
        qgcm_gso_frame f = supers[k].f;
        f.first = first[k];
        qgcm::gso_unpack_entry_cpu(supers[k].packed.data(), f, arena.data(), stride, lens.data());
        for (uint32_t j = 0; j < 5; ++j) {
            const uint32_t i = first[k] + f.count + j;
            lens[i] = odd[j];
            arena[(size_t)i * stride + 4] = (uint8_t)(0x4f);  // version 4, the longest header
            arena[(size_t)i * stride + 4 + 9] = 6;
        }
    }
    status[n - 1] = 0;
    std::vector<uint32_t> cls(n), head(n);
    std::vector<qgcm_gso_frame> frames(n);
    uint64_t counts[4], again[4];
    std::vector<uint8_t> big((size_t)n * (stride + 32), 0xA5);
    qgcm::deliver_coalesce_cpu(arena.data(), stride, n, lens.data(), peer.data(), status.data(), big.data(), big.size(),
                               frames.data(), counts, cls.data(), head.data());
    CHECK(counts[2] == supers.size() && counts[3] == n - 1 && counts[0] == supers.size() + 5 * supers.size() - 1);
    std::vector<uint8_t> exact((size_t)counts[1]);
    std::vector<qgcm_gso_frame> frames2(n);
    qgcm::deliver_coalesce_cpu(arena.data(), stride, n, lens.data(), peer.data(), status.data(), exact.data(), exact.size(),
                               frames2.data(), again, cls.data(), head.data());
    CHECK(memcmp(counts, again, sizeof counts) == 0 && memcmp(exact.data(), big.data(), exact.size()) == 0);
    CHECK(memcmp(frames.data(), frames2.data(), counts[0] * sizeof(qgcm_gso_frame)) == 0);
    for (size_t i = exact.size(); i < big.size(); ++i)
        if (big[i] != 0xA5) {
            CHECK(!"a byte behind the used part was written");
            break;
        }
    CHECK(qgcm::co_table_ok(frames.data(), (uint32_t)counts[0], exact.size()));
    uint32_t k = 0;
    for (uint32_t e = 0; e < counts[0]; ++e) {
        const qgcm_gso_frame &f = frames[e];
        if (f.kind != QGCM_GSO_TCP4) continue;
        const Super &s = supers[k];
        CHECK(f.first == first[k] && f.count == s.f.count && f.len == s.f.len && f.gso_size == s.f.gso_size && f.hdr_len == s.f.hdr_len &&
              f.l4_off == s.f.l4_off && f.reserved == 9);
        // the payload whole; the header but for the fields the coalescing patches
        CHECK(memcmp(exact.data() + f.off + f.hdr_len, s.packed.data() + 16 + f.hdr_len, f.len - f.hdr_len) == 0);
        CHECK(memcmp(exact.data() + f.off, s.packed.data() + 16, 10) == 0);
        CHECK(exact[f.off + f.l4_off + 13] == s.packed[16 + f.l4_off + 13]);
        CHECK(qgcm::gso_fold_not(qgcm::gso_sum_be(exact.data() + f.off, f.l4_off)) == 0);
        ++k;
    }
    CHECK(k == supers.size());
    // one byte short: the last entry does not fit and nothing of it is written
    std::vector<uint8_t> shorter((size_t)counts[1] - 1, 0xA5);
    qgcm::deliver_coalesce_cpu(arena.data(), stride, n, lens.data(), peer.data(), status.data(), shorter.data(), shorter.size(),
                               frames2.data(), again, cls.data(), head.data());
    CHECK(again[1] == counts[1] && frames2[counts[0] - 1].off == qgcm::kCoNoRoom && frames2[counts[0] - 2].off != qgcm::kCoNoRoom);
    const size_t last = frames[counts[0] - 1].off - 16;
    CHECK(memcmp(shorter.data(), exact.data(), last) == 0);
    for (size_t i = last; i < shorter.size(); ++i)
        if (shorter[i] != 0xA5) {
            CHECK(!"a byte of an entry that did not fit was written");
            break;
        }
    // the public entry's argument checks
    CHECK(qgcm_tun_write_gso(-1, exact.data(), exact.size(), frames.data(), 1, nullptr) == -1);
}

void test_table_check() {
    const qgcm_gso_frame good = {16, 100, 5, 2, 30, 40, 20, 16, QGCM_GSO_TCP4, 3};
    CHECK(qgcm::co_table_ok(&good, 1, 116));
    CHECK(!qgcm::co_table_ok(&good, 1, 115));
    qgcm_gso_frame b = good;
    b.off = 0;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    b.off = 20;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    b.off = qgcm::kCoNoRoom;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    for (uint32_t kind : {1u, 3u, 4u}) {
        b = good;
        b.kind = kind;
        CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    }
    b = good, b.count = 3;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    b = good, b.gso_size = 0;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    b = good, b.hdr_len = 38;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    b = good, b.l4_off = 16;
    CHECK(!qgcm::co_table_ok(&b, 1, 4096));
    b = good, b.first = 0xffffffffu;  // `first` is the caller's: not looked at
    CHECK(qgcm::co_table_ok(&b, 1, 4096));
}

void test_write_and_fallback() {
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_DGRAM, 0, sv) != 0) {
        CHECK(!"socketpair");
        return;
    }
    Super s = make_super(24, 32, 100, 7, 33, true);
    std::vector<uint8_t> area = s.packed;  // exactly the entry's region
    qgcm::co_put_lead(area.data(), s.f);
    uint64_t out[3];
    CHECK(qgcm_tun_write_gso(sv[0], area.data(), area.size(), &s.f, 1, out) == 1 && out[0] == 1 && out[1] == 7 && out[2] == 0);
    std::vector<uint8_t> msg(70000);
    ssize_t got = recv(sv[1], msg.data(), msg.size(), 0);
    CHECK(got == (ssize_t)(10 + s.f.len) && memcmp(msg.data(), area.data() + 6, (size_t)got) == 0);
    // a table the check refuses: nothing arrives
    qgcm_gso_frame bad = s.f;
    bad.count = 8;
    CHECK(qgcm_tun_write_gso(sv[0], area.data(), area.size(), &bad, 1, out) == -1 && out[0] == 0);
    CHECK(recv(sv[1], msg.data(), msg.size(), MSG_DONTWAIT) == -1 && (errno == EAGAIN || errno == EWOULDBLOCK));
    // the fallback: the segments of gso_unpack_entry_cpu, each behind ten zero bytes
    const uint64_t stride = 256;
    std::vector<uint8_t> arena((size_t)(stride * s.f.count));
    std::vector<uint32_t> lens(s.f.count);
    qgcm::gso_unpack_entry_cpu(area.data(), s.f, arena.data(), stride, lens.data());
    qgcm_gso_frame moved = s.f;
    moved.first = 12345;  // the caller's slot: the fallback does not index with it
    CHECK(qgcm::tun_write_gso_cut(sv[0], area.data(), moved) == (int)s.f.count);
    for (uint32_t k = 0; k < s.f.count; ++k) {
        got = recv(sv[1], msg.data(), msg.size(), MSG_DONTWAIT);
        CHECK(got == (ssize_t)(10 + lens[k]));
        bool zeros = true;
        for (int i = 0; i < 10; ++i) zeros &= msg[i] == 0;
        CHECK(zeros && memcmp(msg.data() + 10, arena.data() + k * stride + 4, lens[k]) == 0);
    }
    CHECK(recv(sv[1], msg.data(), msg.size(), MSG_DONTWAIT) == -1);
    close(sv[1]);
    // the peer gone: the write fails, -1 and no entry counted; the fallback stops at its first packet
    CHECK(qgcm_tun_write_gso(sv[0], area.data(), area.size(), &s.f, 1, out) == -1 && out[0] == 0 && out[1] == 0);
    CHECK(qgcm::tun_write_gso_cut(sv[0], area.data(), s.f) == 0);
    close(sv[0]);
}

}  // namespace

int main() {
    for (uint64_t stride : {1536ull, 1388ull, 128ull}) test_round_trip(stride);
    test_table_check();
    test_write_and_fallback();
    if (failures) {
        fprintf(stderr, "coalesce_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    printf("coalesce_san_driver ok\n");
    return 0;
}
