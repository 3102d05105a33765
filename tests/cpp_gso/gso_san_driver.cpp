// gso_san_driver.cpp -- the super-frames' host code (gso_core.h: the validity rule, the search, the table check and
// qgcm_gso_unpack_cpu's body; tun_batch.cpp: the argument paths of the TUN calls) under the host compiler's
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, no HIP, no Python.
//
//   1. the segmentation from arrays of exactly the size the contract names (the packed area exactly packed_len
//      bytes, the table exactly n_frames entries, the arena exactly n * stride, lens exactly n): every segment is a
//      packet whose IPv4 and L4 checksums a plain RFC 1071 loop accepts, the payloads give the frame's back, the
//      slots' tails keep their bytes; every gso_size residue, header length, clamp and kind
//   2. every class of table that is not well-formed, and the argument checks: QGCM_E_ARG, nothing written
//   3. gso_find against a linear search, on tables that ascend (with gaps) and on tables that do not (any index
//      below n_frames, every read inside the table)
//   4. qgcm_tun_open_offload and qgcm_tun_read_gso with arguments they refuse
//
// Prints "gso_san_driver ok" and exits 0, or says what differed and exits 1.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/gso_core.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x5EED0650ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

constexpr uint8_t kSentinel = 0xA5;
constexpr uint32_t kLenSentinel = 0xDEADBEEFu;

// RFC 1071, plainly: 0 when the checksum inside the bytes is right
uint16_t rfc1071(const std::vector<uint8_t> &b) {
    uint32_t s = 0;
    for (size_t i = 0; i < b.size(); i += 2) {
        s += (uint32_t)b[i] << 8 | (i + 1 < b.size() ? b[i + 1] : 0);
        s = (s & 0xffff) + (s >> 16);
    }
    return (uint16_t)~s;
}

bool packet_ok(const uint8_t *p, uint32_t len) {
    const uint32_t ihl = (p[0] & 15u) * 4;
    if (len < ihl + 8 || ((uint32_t)p[2] << 8 | p[3]) != len) return false;
    if (rfc1071(std::vector<uint8_t>(p, p + ihl)) != 0) return false;
    std::vector<uint8_t> l4(p + 12, p + 20);
    l4.push_back(0);
    l4.push_back(p[9]);
    l4.push_back((uint8_t)((len - ihl) >> 8));
    l4.push_back((uint8_t)(len - ihl));
    l4.insert(l4.end(), p + ihl, p + len);
    return rfc1071(l4) == 0;
}

struct Case {
    std::vector<uint8_t> packed;         // exactly packed_len bytes
    std::vector<qgcm_gso_frame> frames;  // exactly n_frames entries
    uint32_t n = 0;
};

// a frame of `kind` appended on the next 16-byte boundary that leaves ten bytes free: random bytes with an IPv4
// header of ihl bytes, the L4 header behind it, and the checksum field left as the stack leaves it (anything)
void add(Case &c, uint32_t kind, uint32_t ihl, uint32_t l4_hdr, uint32_t payload, uint32_t gso) {
    const uint32_t off = (uint32_t)((c.packed.size() + 10 + 15) & ~(size_t)15), hdr = ihl + l4_hdr, len = hdr + payload;
    c.packed.resize(off + len);
    for (size_t i = off - 10; i < c.packed.size(); ++i) c.packed[i] = (uint8_t)rnd();
    uint8_t *p = c.packed.data() + off;
    const bool tcp = l4_hdr != 8;
    if (len) p[0] = (uint8_t)(0x40 | ihl / 4);
    if (len > 9) p[9] = tcp ? 6 : 17;
    if (len > 3) p[2] = (uint8_t)(len >> 8), p[3] = (uint8_t)len;
    qgcm_gso_frame f{};
    f.off = off;
    f.len = len;
    f.first = c.n;
    f.kind = kind;
    f.count = 1;
    if (kind == QGCM_GSO_TCP4 || kind == QGCM_GSO_UDP4) {
        f.gso_size = (uint16_t)gso;
        f.hdr_len = (uint16_t)hdr;
        f.l4_off = (uint16_t)ihl;
        f.count = (payload + gso - 1) / gso;
        if (tcp) p[ihl + 13] |= 0x09;  // FIN, PSH
    } else if (kind == QGCM_GSO_CSUM) {
        f.l4_off = (uint16_t)ihl;
        f.csum_off = tcp ? 16 : 6;
        // a right packet but for the L4 checksum, which holds the pseudo-header's sum
        if (!tcp) p[ihl + 4] = (uint8_t)((len - ihl) >> 8), p[ihl + 5] = (uint8_t)(len - ihl);
        p[10] = p[11] = 0;
        const uint16_t ipc = rfc1071(std::vector<uint8_t>(p, p + ihl));
        p[10] = (uint8_t)(ipc >> 8), p[11] = (uint8_t)ipc;
        std::vector<uint8_t> pseudo(p + 12, p + 20);
        pseudo.push_back(0);
        pseudo.push_back(p[9]);
        pseudo.push_back((uint8_t)((len - ihl) >> 8));
        pseudo.push_back((uint8_t)(len - ihl));
        const uint16_t part = (uint16_t)~rfc1071(pseudo);
        p[ihl + f.csum_off] = (uint8_t)(part >> 8), p[ihl + f.csum_off + 1] = (uint8_t)part;
    }
    c.n += f.count;
    c.frames.push_back(f);
}

void run(const Case &c, uint64_t stride) {
    const uint32_t n = c.n, nf = (uint32_t)c.frames.size();
    std::vector<uint8_t> arena(n * stride, kSentinel);
    std::vector<uint32_t> lens(n, kLenSentinel);
    CHECK(qgcm::gso_table_ok(c.frames.data(), nf, n, c.packed.size()));
    CHECK(qgcm::gso_unpack_checked(c.packed.data(), c.packed.size(), c.frames.data(), nf, n, arena.data(), stride, lens.data()) ==
          QGCM_OK);
    for (const qgcm_gso_frame &f : c.frames) {
        const uint8_t *frame = c.packed.data() + f.off;
        std::vector<uint8_t> payload;
        for (uint32_t k = 0; k < f.count; ++k) {
            const uint32_t i = f.first + k, L = lens[i];
            const uint8_t *slot = arena.data() + (uint64_t)i * stride;
            const uint64_t held = L < stride - 4 ? L : stride - 4;
            for (uint64_t b = 4 + held; b < stride; ++b) CHECK(slot[b] == kSentinel);
            for (uint64_t b = 0; b < 4; ++b) CHECK(slot[b] == kSentinel);
            if (f.kind == QGCM_GSO_PLAIN) {
                CHECK(L == f.len && memcmp(slot + 4, frame, held) == 0);
                continue;
            }
            if (held == L) CHECK(packet_ok(slot + 4, L));
            if (f.kind == QGCM_GSO_CSUM) continue;
            CHECK(L == f.hdr_len + qgcm::gso_seg_payload(f, k));
            if (held == L) {
                payload.insert(payload.end(), slot + 4 + f.hdr_len, slot + 4 + L);
                const uint8_t flags = slot[4 + f.l4_off + 13];
                if (f.kind == QGCM_GSO_TCP4) CHECK((flags & 0x09) == (k + 1 == f.count ? 0x09 : 0));
            }
        }
        if (f.kind >= QGCM_GSO_TCP4 && payload.size() == f.len - f.hdr_len)
            CHECK(memcmp(payload.data(), frame + f.hdr_len, payload.size()) == 0);
    }
}

Case mixed() {
    Case c;
    for (uint32_t gso : {1u, 3u, 4u, 15u, 16u, 17u, 1347u, 1348u, 1448u})
        for (uint32_t tail : {1u, 2u, 3u, gso - 1, gso})
            if (tail >= 1 && tail <= gso) add(c, QGCM_GSO_TCP4, 20, 20, 2 * gso + tail, gso);
    for (uint32_t ihl : {20u, 24u, 60u})
        for (uint32_t th : {20u, 32u, 60u}) add(c, QGCM_GSO_TCP4, ihl, th, 4000, 1348);
    for (uint32_t gso : {1u, 31u, 1472u}) add(c, QGCM_GSO_UDP4, 24, 8, 3 * gso - 1, gso);
    add(c, QGCM_GSO_TCP4, 20, 20, QGCM_GSO_SEGS * 3, 3);
    for (uint32_t payload : {0u, 1u, 2u, 3u, 100u, 1349u}) {
        add(c, QGCM_GSO_CSUM, 20, 20, payload, 0);
        add(c, QGCM_GSO_CSUM, 24, 8, payload, 0);
    }
    for (uint32_t len : {0u, 1u, 19u, 20u, 1350u, 3000u}) add(c, QGCM_GSO_PLAIN, 0, 0, len, 0);
    add(c, QGCM_GSO_PLAIN, 0, 0, 77, 0);  // the area ends off the 16-byte grid
    return c;
}

void unpack_cases() {
    const Case c = mixed();
    for (uint64_t stride : {3104ull, 1536ull, 1388ull, 64ull, 8ull}) run(c, stride);
    Case none;
    run(none, 64);  // n == 0: empty vectors, NULL data
}

void refusals() {
    const Case good = mixed();
    const uint32_t n = good.n, nf = (uint32_t)good.frames.size();
    const uint64_t packed_len = good.packed.size();
    uint32_t tcp = 0, udp = 0, cs = 0, pl = 0;
    for (uint32_t e = 0; e < nf; ++e) {
        if (good.frames[e].kind == QGCM_GSO_TCP4 && !tcp) tcp = e + 1;
        if (good.frames[e].kind == QGCM_GSO_UDP4 && !udp) udp = e + 1;
        if (good.frames[e].kind == QGCM_GSO_CSUM && !cs) cs = e + 1;
        if (good.frames[e].kind == QGCM_GSO_PLAIN && !pl) pl = e + 1;
    }
    --tcp, --udp, --cs, --pl;
    std::vector<std::vector<qgcm_gso_frame>> bad;
    auto with = [&](uint32_t e, auto change) {
        std::vector<qgcm_gso_frame> t = good.frames;
        change(t[e]);
        bad.push_back(t);
    };
    with(tcp, [](qgcm_gso_frame &f) { f.off += 4; });
    with(nf - 1, [&](qgcm_gso_frame &f) { f.len += 1; });
    with(pl, [](qgcm_gso_frame &f) { f.off = 0xFFFFFFF0u, f.len = 0x20; });
    with(pl, [](qgcm_gso_frame &f) { f.kind = 4; });
    with(pl, [](qgcm_gso_frame &f) { f.count = 2; });
    with(cs, [](qgcm_gso_frame &f) { f.count = 0; });
    with(cs, [](qgcm_gso_frame &f) { f.l4_off += 1; });
    with(cs, [](qgcm_gso_frame &f) { f.csum_off += 1; });
    with(cs, [](qgcm_gso_frame &f) { f.csum_off = (uint16_t)((f.len - f.l4_off + 1) & ~1u); });
    with(tcp, [](qgcm_gso_frame &f) { f.l4_off = 16; });
    with(tcp, [](qgcm_gso_frame &f) { f.l4_off = 64, f.hdr_len = 84; });
    with(tcp, [](qgcm_gso_frame &f) { f.l4_off = 22, f.hdr_len = 42; });
    with(udp, [](qgcm_gso_frame &f) { f.hdr_len += 4; });
    with(tcp, [](qgcm_gso_frame &f) { f.hdr_len = f.l4_off + 16; });
    with(tcp, [](qgcm_gso_frame &f) { f.hdr_len = f.l4_off + 64; });
    with(tcp, [](qgcm_gso_frame &f) { f.hdr_len = f.l4_off + 22; });
    with(tcp, [](qgcm_gso_frame &f) { f.len = f.hdr_len; });
    with(tcp, [](qgcm_gso_frame &f) { f.gso_size = 0; });
    with(tcp, [](qgcm_gso_frame &f) { f.count -= 1; });
    with(udp, [](qgcm_gso_frame &f) { f.count += 1; });
    with(tcp, [](qgcm_gso_frame &f) { f.first += 1; });
    {
        std::vector<qgcm_gso_frame> t = good.frames;
        std::swap(t[tcp], t[tcp + 1]);
        bad.push_back(t);
    }
    for (const auto &t : bad) {
        std::vector<uint8_t> arena(n * 256ull, kSentinel);
        std::vector<uint32_t> lens(n, kLenSentinel);
        CHECK(!qgcm::gso_table_ok(t.data(), nf, n, packed_len));
        CHECK(qgcm::gso_unpack_checked(good.packed.data(), packed_len, t.data(), nf, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
        for (uint8_t v : arena) CHECK(v == kSentinel);
        for (uint32_t v : lens) CHECK(v == kLenSentinel);
    }
    // one segment more than QGCM_GSO_SEGS
    Case big;
    add(big, QGCM_GSO_TCP4, 20, 20, QGCM_GSO_SEGS + 1, 1);
    CHECK(big.n == QGCM_GSO_SEGS + 1 && !qgcm::gso_table_ok(big.frames.data(), 1, big.n, big.packed.size()));
    std::vector<uint8_t> arena(n * 256ull, kSentinel);
    std::vector<uint32_t> lens(n + 1, kLenSentinel);
    const uint8_t *p = good.packed.data();
    const qgcm_gso_frame *f = good.frames.data();
    CHECK(qgcm::gso_unpack_checked(p, packed_len, f, nf, n - 1, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(p, packed_len, f, nf - 1, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(nullptr, packed_len, f, nf, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(p, packed_len, nullptr, nf, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(p, packed_len, f, nf, n, nullptr, 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(p, packed_len, f, nf, n, arena.data(), 256, nullptr) == QGCM_E_ARG);
    for (uint64_t stride : {0ull, 4ull, 258ull})
        CHECK(qgcm::gso_unpack_checked(p, packed_len, f, nf, n, arena.data(), stride, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(p, packed_len, f, nf, QGCM_MAX_BATCH + 1, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    CHECK(qgcm::gso_unpack_checked(p, packed_len, f, n + 1, n, arena.data(), 256, lens.data()) == QGCM_E_ARG);
    for (uint8_t v : arena) CHECK(v == kSentinel);
    CHECK(qgcm::gso_unpack_checked(nullptr, 0, nullptr, 0, 0, nullptr, 256, nullptr) == QGCM_OK);
}

void search() {
    for (int round = 0; round < 60; ++round) {
        const uint32_t nf = 1 + rnd() % 70;
        std::vector<qgcm_gso_frame> t(nf);  // exactly nf entries: a read past the table is an ASan report
        uint32_t at = 0;
        for (auto &f : t) {
            at += rnd() % 3 == 0 ? rnd() % 5 : 0;  // a gap now and then
            f.first = at;
            f.count = 1 + rnd() % (round % 2 ? 2048 : 4);
            at += f.count;
        }
        const uint32_t n = at + rnd() % 4;
        for (uint32_t i = 0; i < n; i += 1 + (n > 4000 ? rnd() % 37 : 0)) {
            uint32_t want = 0;
            for (uint32_t e = 0; e < nf; ++e)
                if (t[e].first <= i) want = e;
            CHECK(qgcm::gso_find(t.data(), nf, n, i) == want);
        }
        for (auto &f : t) f.first = rnd();  // no order at all
        for (uint32_t i = 0; i < n; i += 1 + (n > 4000 ? rnd() % 37 : 0)) CHECK(qgcm::gso_find(t.data(), nf, n, i) < nf);
    }
}

void tun_arguments() {
    std::vector<uint8_t> packed(65536 + 16);
    std::vector<qgcm_gso_frame> frames(4);
    uint64_t out[3] = {7, 7, 7};
    int fds[1] = {-1};
    CHECK(qgcm_tun_open_offload("qgcmg%d", 1, fds, nullptr, 0, 4) == -EINVAL);
    CHECK(qgcm_tun_open_offload("qgcmg%d", 0, fds, nullptr, 0, QGCM_TUN_TSO4) == -EINVAL);
    CHECK(qgcm_tun_open_offload("qgcmg%d", 1, nullptr, nullptr, 0, QGCM_TUN_TSO4) == -EINVAL);
    CHECK(qgcm_tun_read_gso(-1, packed.data(), packed.size(), frames.data(), 4, 4096, 0, out) == -1);
    CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0);
    CHECK(qgcm_tun_read_gso(0, nullptr, packed.size(), frames.data(), 4, 4096, 0, out) == -1);
    CHECK(qgcm_tun_read_gso(0, packed.data(), packed.size(), nullptr, 4, 4096, 0, out) == -1);
    CHECK(qgcm_tun_read_gso(0, packed.data(), packed.size() - 1, frames.data(), 4, 4096, 0, out) == -1);
    CHECK(qgcm_tun_read_gso(0, packed.data(), packed.size(), frames.data(), 4, QGCM_GSO_SEGS - 1, 0, out) == -1);
    CHECK(qgcm_tun_read_gso(0, packed.data(), packed.size(), frames.data(), 0, 4096, 0, nullptr) == 0);
}

}  // namespace

int main() {
    unpack_cases();
    refusals();
    search();
    tun_arguments();
    if (failures) {
        fprintf(stderr, "gso_san_driver: %d check(s) failed\n", failures);
        return 1;
    }
    puts("gso_san_driver ok");
    return 0;
}
