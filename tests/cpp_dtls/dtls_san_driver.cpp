// dtls_san_driver.cpp -- the host code of the DTLS record layer under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_dtls_sanitizers.py builds it with the host compiler and runs it as a
// child process): dtls_core.h's rules through qgcm_dtls_number_cpu and qgcm_dtls_replay_cpu (parallel against
// packet by packet, the shifts at 63, 64 and beyond, numbers at the 48-bit end), qgcm_dtls_key_block, and
// qgcm_udp_send_dtls / qgcm_udp_recv_dtls over loopback.  Every array is a heap allocation of exactly the size the
// contract names, so a byte read or written past it is reported.
#include <arpa/inet.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "../../include/qgcm.h"
#include "../../quantum_amd/csrc/dtls_core.h"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #x); \
            exit(1);                                                   \
        }                                                              \
    } while (0)

using namespace qgcm;

template <class T>
static std::unique_ptr<T[]> exact(size_t n) {
    return std::unique_ptr<T[]>(new T[n ? n : 1]());
}

static void window_rules() {
    // the edge: 63 behind is inside the window, 64 is not; shifts of 63, 64, 65 and far more
    for (uint64_t sh : {1ull, 63ull, 64ull, 65ull, 1ull << 40}) {
        uint64_t R = 100, W = ~0ull;
        CHECK(dtls_window_step(R, W, 100 + sh));
        CHECK(R == 100 + sh && W == (sh >= 64 ? 1ull : ((~0ull << sh) | 1ull)));
        CHECK(dtls_window_carry(100, ~0ull, 100 + sh) == (sh >= 64 ? 0ull : ~0ull << sh));
    }
    CHECK(dtls_window_bit(100, 37) == 1ull << 63 && dtls_window_bit(100, 36) == 0);
    CHECK(dtls_window_accept(100, 1, 100, 37, false) && !dtls_window_accept(100, 1, 100, 36, false));
    CHECK(!dtls_window_accept(100, 1, 100, 37, true) && !dtls_window_accept(100, 1, 100, 100, false));
    // random batches: the parallel form and the packet-by-packet rule agree, state included
    std::mt19937_64 rng(0xD7151100);
    for (int round = 0; round < 300; ++round) {
        const uint32_t ns = 1 + rng() % 4, n = rng() % 90;
        auto sess = exact<uint32_t>(n);
        auto seq = exact<uint64_t>(n);
        auto auth = exact<uint8_t>(n);
        auto acc_s = exact<uint8_t>(n), acc_p = exact<uint8_t>(n);
        auto st_s = exact<uint64_t>(2 * ns), st_p = exact<uint64_t>(2 * ns);
        const bool top = round % 10 == 0;  // numbers at the end of the 48-bit range
        for (uint32_t p = 0; p < ns; ++p) {
            st_s[2 * p] = st_p[2 * p] = top ? kDtlsSeqEnd - 1 - rng() % 80 : rng() % 200;
            st_s[2 * p + 1] = st_p[2 * p + 1] = rng() | 1;
        }
        for (uint32_t i = 0; i < n; ++i) {
            sess[i] = rng() % (ns + 1);  // ns: out of range, counts for nothing
            const uint64_t base = st_s[2 * (sess[i] % ns)];
            const int64_t d = (int64_t)(rng() % 150) - 75;
            int64_t v = (int64_t)base + d;
            if (v < 0) v = 0;
            if ((uint64_t)v >= kDtlsSeqEnd) v = (int64_t)kDtlsSeqEnd - 1;
            seq[i] = (uint64_t)v;
            auth[i] = rng() % 5 != 0;
        }
        CHECK(qgcm_dtls_replay_cpu(n, sess.get(), seq.get(), auth.get(), ns, st_s.get(), acc_s.get(), 0) == QGCM_OK);
        CHECK(qgcm_dtls_replay_cpu(n, sess.get(), seq.get(), auth.get(), ns, st_p.get(), acc_p.get(), 1) == QGCM_OK);
        CHECK(memcmp(acc_s.get(), acc_p.get(), n) == 0);
        CHECK(memcmp(st_s.get(), st_p.get(), 16 * ns) == 0);
    }
}

static void numbering() {
    const uint32_t ns = 3, n = 9;
    auto keys = exact<qgcm_dtls_keys>(ns);
    auto wseq = exact<uint64_t>(ns);
    auto set = exact<uint8_t>(ns);
    for (uint32_t p = 0; p < ns; ++p) {
        keys[p].write_epoch = (uint16_t)(1 + p);
        set[p] = p != 2;
    }
    wseq[0] = kDtlsSeqEnd - 2;
    wseq[1] = 5;
    auto lens = exact<uint32_t>(n);
    auto peer = exact<uint32_t>(n);
    auto hdr = exact<qgcm_dtls_hdr>(n);
    auto status = exact<uint8_t>(n);
    auto reason = exact<uint8_t>(n);
    const uint32_t L[n] = {1, 16384, 0, 16385, 40, 49, 40, 40, 40}, P[n] = {0, 1, 1, 1, 2, 1, 0, 0, QGCM_NO_PEER};
    memcpy(lens.get(), L, sizeof L);
    memcpy(peer.get(), P, sizeof P);
    memset(hdr.get(), 0xA5, n * sizeof(qgcm_dtls_hdr));
    CHECK(qgcm_dtls_number_cpu(keys.get(), set.get(), wseq.get(), ns, 16400, n, lens.get(), peer.get(), hdr.get(),
                               status.get(), reason.get()) == QGCM_OK);
    const uint8_t want[n] = {0, 0, QGCM_DTLS_MALFORMED, QGCM_DTLS_MALFORMED, QGCM_DTLS_NO_SESSION, 0, 0,
                             QGCM_DTLS_SEQ_EXHAUSTED, QGCM_DTLS_NO_SESSION};
    CHECK(memcmp(reason.get(), want, n) == 0);
    CHECK(wseq[0] == kDtlsSeqEnd && wseq[1] == 7 && lens[1] == 16400 && lens[2] == 0 && lens[7] == 40);
    CHECK(dtls_hdr_seq(hdr[6].b) == kDtlsSeqEnd - 1 && hdr[6].b[3] == 0 && hdr[6].b[4] == 1 && hdr[6].b[31] == 0);
    CHECK(hdr[5].b[11] == ((8 + 49 + 16) >> 8) && hdr[5].b[12] == ((8 + 49 + 16) & 0xff) && hdr[7].b[0] == 0xA5);
    // the open's checks, on an exact 13-byte header
    auto h = exact<uint8_t>(13);
    memcpy(h.get(), hdr[5].b, 13);
    CHECK(dtls_open_check(h.get(), 65, 68, 2) == QGCM_DTLS_OK && dtls_open_check(h.get(), 65, 64, 2) == QGCM_DTLS_MALFORMED);
    CHECK(dtls_open_check(h.get(), 65, 68, 1) == QGCM_DTLS_MALFORMED && dtls_open_check(h.get(), 64, 68, 2) == QGCM_DTLS_MALFORMED);
    h[0] = 22;
    CHECK(dtls_open_check(h.get(), 65, 68, 1) == QGCM_DTLS_NOT_APPDATA);
}

static void key_block() {
    auto m = exact<uint8_t>(48);
    auto cr = exact<uint8_t>(32), sr = exact<uint8_t>(32);
    auto out = exact<uint8_t>(72), again = exact<uint8_t>(72);
    for (int i = 0; i < 48; ++i) m[i] = (uint8_t)i;
    for (int i = 0; i < 32; ++i) {
        cr[i] = (uint8_t)(100 + i);
        sr[i] = (uint8_t)(200 - i);
    }
    CHECK(qgcm_dtls_key_block(m.get(), cr.get(), sr.get(), out.get()) == QGCM_OK);
    CHECK(qgcm_dtls_key_block(m.get(), cr.get(), sr.get(), again.get()) == QGCM_OK);
    CHECK(memcmp(out.get(), again.get(), 72) == 0);
    // PRF_SHA384 of this input, from hashlib / hmac (RFC 5246 5): its first and last four bytes
    const uint8_t head[4] = {0xdb, 0xb3, 0xe7, 0xb3}, tail[4] = {0xd0, 0x3f, 0x8d, 0x68};
    CHECK(memcmp(out.get(), head, 4) == 0 && memcmp(out.get() + 68, tail, 4) == 0);
    cr[0] ^= 1;
    CHECK(qgcm_dtls_key_block(m.get(), cr.get(), sr.get(), again.get()) == QGCM_OK && memcmp(out.get(), again.get(), 72) != 0);
    CHECK(qgcm_dtls_key_block(nullptr, cr.get(), sr.get(), out.get()) == QGCM_E_ARG);
}

static void udp() {
    const int rx = qgcm_udp_socket("127.0.0.1", 0, 1 << 20), tx = qgcm_udp_socket("127.0.0.1", 0, 1 << 20);
    CHECK(rx >= 0 && tx >= 0);
    const uint64_t stride = 64;
    const uint32_t n = 6;
    auto arena = exact<uint8_t>(n * stride);
    auto hdr = exact<qgcm_dtls_hdr>(n);
    auto lens = exact<uint32_t>(n);
    auto peer = exact<uint32_t>(n);
    auto status = exact<uint8_t>(n);
    for (uint32_t i = 0; i < n * stride; ++i) arena[i] = (uint8_t)(i * 7);
    for (uint32_t i = 0; i < n; ++i) {
        memset(hdr[i].b, (int)(0x10 + i), sizeof hdr[i].b);
        lens[i] = i == 2 ? 64 : 1 + 9 * i;
        status[i] = i != 4;
    }
    qgcm_peer_addr to{};
    inet_pton(AF_INET, "127.0.0.1", &to.ip);
    to.port = htons((uint16_t)qgcm_udp_port(rx));
    CHECK(qgcm_udp_send_dtls(tx, arena.get(), stride, n, lens.get(), hdr.get(), status.get(), peer.get(), &to, 1) == 5);
    // one more record of 64 bytes, for the receive into shorter slots below
    auto extra = exact<uint8_t>(64);
    auto xl = exact<uint32_t>(1);
    auto xh = exact<qgcm_dtls_hdr>(1);
    auto xp = exact<uint32_t>(1);
    xl[0] = 64;
    CHECK(qgcm_udp_send_dtls(tx, extra.get(), 64, 1, xl.get(), xh.get(), nullptr, xp.get(), &to, 1) == 1);
    // receive into exactly 5 slots, in two calls
    auto r_arena = exact<uint8_t>(5 * stride);
    auto r_hdr = exact<qgcm_dtls_hdr>(5);
    auto r_lens = exact<uint32_t>(5);
    auto r_addr = exact<qgcm_peer_addr>(5);
    uint32_t got = 0, dropped = 0, d = 0;
    for (int tries = 0; tries < 50 && got < 5; ++tries) {
        const int k = qgcm_udp_recv_dtls(rx, r_arena.get() + got * stride, stride, got < 2 ? 2 - got : 5 - got,
                                         r_lens.get() + got, r_hdr.get() + got, r_addr.get() + got, 200, &d);
        CHECK(k >= 0);
        got += (uint32_t)k;
        dropped += d;
    }
    CHECK(got == 5 && dropped == 0);
    const uint32_t src[5] = {0, 1, 2, 3, 5};
    for (uint32_t k = 0; k < 5; ++k) {
        CHECK(r_lens[k] == lens[src[k]] && memcmp(r_arena.get() + k * stride, arena.get() + src[k] * stride, r_lens[k]) == 0);
        CHECK(memcmp(r_hdr[k].b, hdr[src[k]].b, 21) == 0 && r_hdr[k].b[21] == 0 && r_hdr[k].b[31] == 0);
        CHECK(r_addr[k].port == htons((uint16_t)qgcm_udp_port(tx)));
    }
    // the 64-byte record fits a 64-byte slot; into 60-byte slots it is too long and is dropped and counted
    auto s_arena = exact<uint8_t>(2 * 60);
    CHECK(qgcm_udp_recv_dtls(rx, s_arena.get(), 60, 2, r_lens.get(), r_hdr.get(), nullptr, 200, &d) == 0 && d == 1);
    CHECK(qgcm_udp_close(rx) == 0 && qgcm_udp_close(tx) == 0);
}

int main() {
    window_rules();
    numbering();
    key_block();
    udp();
    printf("dtls_san_driver ok\n");
    return 0;
}
