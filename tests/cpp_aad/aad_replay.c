/*
 * aad_replay.c -- replays, through include/qgcm.h, the C calls go/crypto/aes_gpu.go makes for Encrypt /
 * Decrypt with `additional` longer than the 4-byte Payload IP header (the shim no longer refuses it:
 * len(additional) goes straight to qgcm_seal_one / qgcm_open_one, and a -1 becomes the seal error or
 * errOpen).  No Go toolchain exists where the tests run, so the cgo shim is exercised by its calls, as
 * tests/cpp/go_replay.c does for the rest of the shim.  TEST INFRASTRUCTURE: links the oracle
 * (oracle/_build/liboracle.so) as the checker: the nonce the library drew is in the output, so
 * oracle_aesgo_encrypt(key, plaintext, L, additional, that nonce) must reproduce the sealed bytes.
 *
 *   TestAESAdditional  NewAES on the process-wide device set (every device the process sees, 64 key
 *                      slots), then Encrypt / Decrypt of a 1350-B packet with a 13-B and a 1000-B
 *                      additional, each against the oracle; Decrypt under additional with one bit
 *                      flipped -> errOpen and zeroed plaintext, tag and nonce untouched; additional
 *                      past QGCM_MAX_AAD -> the seal error with data untouched, errOpen on Decrypt
 * Usage: aad_replay [TestName ...] (default: all).  Prints "--- PASS: Name" per test.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qgcm.h"

/* oracle/gcm_oracle.c (test infrastructure) */
long oracle_aesgo_encrypt(const uint8_t key[32], uint8_t *data, long length, const uint8_t *aad, long aad_len,
                          const uint8_t nonce[12]);

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                       \
            return;                                                           \
        }                                                                     \
    } while (0)

static const char kSecret[] = "AES256Key-32Characters1234567890";

struct aes { /* type AES struct { g, ctx, idx, salt } */
    qgcm_ctx *ctx;
    uint32_t idx;
    uint8_t key[32]; /* kept for the oracle only; the Go object holds no key bytes */
};

/* Devices() + NewAES(secret, salt): the device set, the slot's owner, qgcm_derive_key + qgcm_set_key */
static qgcm_group *g_group;
static int new_aes(const uint8_t *secret, size_t slen, const uint8_t *salt, size_t saltlen, struct aes *out) {
    static uint32_t next;
    if (!g_group) {
        char err[QGCM_ERRLEN];
        int devs[64], n = qgcm_device_count();
        if (n > 64) n = 64;
        for (int i = 0; i < n; ++i) devs[i] = i;
        if (n <= 0 || !(g_group = qgcm_group_create(devs, n, 64, err, sizeof err))) {
            fprintf(stderr, "qgcm_group_create: %s\n", n > 0 ? err : "no device");
            return -1;
        }
    }
    const uint32_t idx = next++;
    qgcm_ctx *ctx = qgcm_group_ctx(g_group, qgcm_group_shard(g_group, idx));
    if (!ctx || qgcm_derive_key(secret, slen, salt, saltlen, out->key) != QGCM_OK ||
        qgcm_set_key(ctx, idx, out->key) != QGCM_OK)
        return -1;
    out->ctx = ctx;
    out->idx = idx;
    return 0;
}

/* AES.Encrypt / AES.Decrypt: the shim's remaining guards, then the C call on the owner */
static long aes_encrypt(const struct aes *a, uint8_t *data, long cap, long length, const uint8_t *ad, long adlen) {
    if (length < 0 || length + QGCM_OVERHEAD > cap) return -1; /* errShortBuffer */
    return qgcm_seal_one(a->ctx, a->idx, data, length, adlen ? ad : NULL, (uint32_t)adlen, NULL);
}
static long aes_decrypt(const struct aes *a, uint8_t *data, long len, const uint8_t *ad, long adlen) {
    if (len < QGCM_OVERHEAD) return -1; /* errOpen */
    return qgcm_open_one(a->ctx, a->idx, data, len, adlen ? ad : NULL, (uint32_t)adlen);
}

static void TestAESAdditional(void) {
    enum { L = 1350, kMaxAd = QGCM_MAX_AAD + 1 };
    uint8_t salt[QGCM_SALT_BYTES];
    for (int i = 0; i < 32; ++i) salt[i] = (uint8_t)(i * 37 + 1);
    struct aes a;
    CHECK(new_aes((const uint8_t *)kSecret, 32, salt, 32, &a) == 0);
    static uint8_t ad[kMaxAd];
    for (int i = 0; i < kMaxAd; ++i) ad[i] = (uint8_t)(i * 131 + 7);
    const long adlens[] = {13, 1000};
    for (unsigned k = 0; k < sizeof adlens / sizeof adlens[0]; ++k) {
        const long n = adlens[k];
        uint8_t data[L + 28], plain[L], want[L + 28], nonce[12], tail[28];
        for (int i = 0; i < L; ++i) plain[i] = data[i] = (uint8_t)(i * 29 + k);
        memset(data + L, 0, 28);
        CHECK(aes_encrypt(&a, data, sizeof data, L, ad, n) == L + 28);
        memcpy(nonce, data + L + 16, 12);
        memcpy(want, plain, L);
        CHECK(oracle_aesgo_encrypt(a.key, want, L, ad, n, nonce) == L + 28);
        CHECK(memcmp(data, want, L + 28) == 0);
        /* additional with one bit flipped: errOpen, plaintext zeroed, tag and nonce as they were */
        uint8_t bad[L + 28];
        memcpy(bad, data, sizeof bad);
        memcpy(tail, data + L, 28);
        ad[n - 1] ^= 0x80;
        CHECK(aes_decrypt(&a, bad, sizeof bad, ad, n) == -1);
        ad[n - 1] ^= 0x80;
        for (int i = 0; i < L; ++i) CHECK(bad[i] == 0);
        CHECK(memcmp(bad + L, tail, 28) == 0);
        CHECK(aes_decrypt(&a, data, sizeof data, ad, n) == L);
        CHECK(memcmp(data, plain, L) == 0);
    }
    /* past QGCM_MAX_AAD: the seal error with data untouched, errOpen with data untouched */
    uint8_t data[L + 28], before[L + 28];
    for (int i = 0; i < L + 28; ++i) data[i] = before[i] = (uint8_t)(i * 3 + 1);
    CHECK(aes_encrypt(&a, data, sizeof data, L, ad, kMaxAd) == -1);
    CHECK(memcmp(data, before, sizeof data) == 0);
    CHECK(aes_decrypt(&a, data, sizeof data, ad, kMaxAd) == -1);
    CHECK(memcmp(data, before, sizeof data) == 0);
    printf("--- PASS: TestAESAdditional\n");
}

int main(int argc, char **argv) {
    const struct {
        const char *name;
        void (*fn)(void);
    } tests[] = {{"TestAESAdditional", TestAESAdditional}};
    for (unsigned t = 0; t < sizeof tests / sizeof tests[0]; ++t) {
        int want = argc <= 1;
        for (int i = 1; i < argc; ++i) want |= !strcmp(argv[i], tests[t].name);
        if (want) tests[t].fn();
    }
    if (g_group) qgcm_group_destroy(g_group);
    return failures ? 1 : 0;
}
