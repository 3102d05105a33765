/* ossl_dtls_peer.c -- an OpenSSL DTLS 1.2 session to test the record layer against (tests/test_dtls_openssl.py,
 * tests/golden/make_dtls_records.py).  Two SSL objects in one thread, client and server, joined by an AF_UNIX
 * SOCK_DGRAM socketpair (non-blocking, no network), handshake ECDHE-ECDSA-AES256-GCM-SHA384 with a self-signed
 * P-256 certificate made in the process.  Then it takes commands on stdin, one per line, and answers on stdout:
 *
 *   keys                 -> "master <hex>", "client_random <hex>", "server_random <hex>", "cipher <name>"
 *   cwrite <hex>         the client SSL_writes the bytes; -> "record <hex>": the datagram, taken off the wire
 *   swrite <hex>         the same for the server
 *   sinject <hex>        puts a datagram on the wire towards the server; -> "ok"
 *   cinject <hex>        ... towards the client
 *   sread / cread        SSL_read on that side; -> "plain <hex>" or "none" (nothing deliverable: the record was
 *                        dropped, as a replayed or forged one is)
 *   quit
 * A record "taken off the wire" is not delivered to the other side unless it is injected again. */
#include <openssl/bio.h>
#include <openssl/ec.h>
#include <openssl/err.h>
#include <openssl/evp.h>
#include <openssl/ssl.h>
#include <openssl/x509.h>

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#define MAXREC 20000

static void die(const char *what) {
    fprintf(stderr, "ossl_dtls_peer: %s\n", what);
    ERR_print_errors_fp(stderr);
    exit(1);
}

static void put_hex(const char *tag, const unsigned char *p, size_t n) {
    printf("%s ", tag);
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
    fflush(stdout);
}

static int unhex(const char *s, unsigned char *out, size_t cap) {
    size_t n = 0;
    while (s[0] && s[1] && s[0] != '\n') {
        unsigned v;
        if (n == cap || sscanf(s, "%2x", &v) != 1) return -1;
        out[n++] = (unsigned char)v;
        s += 2;
    }
    return (int)n;
}

static X509 *self_signed(EVP_PKEY *key) {
    X509 *x = X509_new();
    if (!x) die("X509_new");
    X509_set_version(x, 2);
    ASN1_INTEGER_set(X509_get_serialNumber(x), 1);
    X509_gmtime_adj(X509_getm_notBefore(x), -3600);
    X509_gmtime_adj(X509_getm_notAfter(x), 86400);
    X509_set_pubkey(x, key);
    X509_NAME *name = X509_get_subject_name(x);
    X509_NAME_add_entry_by_txt(name, "CN", MBSTRING_ASC, (const unsigned char *)"dtls-peer", -1, -1, 0);
    X509_set_issuer_name(x, name);
    if (!X509_sign(x, key, EVP_sha256())) die("X509_sign");
    return x;
}

static SSL *make_side(SSL_CTX *ctx, int fd, int server) {
    SSL *s = SSL_new(ctx);
    BIO *b = BIO_new_dgram(fd, BIO_NOCLOSE);
    BIO_ADDR *peer = BIO_ADDR_new();
    if (!s || !b || !peer) die("SSL_new / BIO_new_dgram");
    BIO_ctrl_set_connected(b, peer); /* without it the first write fails: the BIO would sendto() a NULL address */
    BIO_ADDR_free(peer);
    SSL_set_bio(s, b, b);
    SSL_set_options(s, SSL_OP_NO_QUERY_MTU);
    DTLS_set_link_mtu(s, 1500);
    if (server)
        SSL_set_accept_state(s);
    else
        SSL_set_connect_state(s);
    return s;
}

int main(void) {
    int fd[2];
    if (socketpair(AF_UNIX, SOCK_DGRAM, 0, fd) != 0) die("socketpair");
    for (int i = 0; i < 2; ++i) {
        fcntl(fd[i], F_SETFL, fcntl(fd[i], F_GETFL) | O_NONBLOCK);
        int sz = 1 << 20;
        setsockopt(fd[i], SOL_SOCKET, SO_SNDBUF, &sz, sizeof sz);
    }
    SSL_CTX *ctx = SSL_CTX_new(DTLS_method());
    if (!ctx) die("SSL_CTX_new");
    SSL_CTX_set_min_proto_version(ctx, DTLS1_2_VERSION);
    SSL_CTX_set_max_proto_version(ctx, DTLS1_2_VERSION);
    if (!SSL_CTX_set_cipher_list(ctx, "ECDHE-ECDSA-AES256-GCM-SHA384")) die("cipher list");
    SSL_CTX_set_verify(ctx, SSL_VERIFY_NONE, NULL);
    EVP_PKEY *key = EVP_EC_gen("P-256");
    if (!key) die("EVP_EC_gen");
    X509 *cert = self_signed(key);
    if (!SSL_CTX_use_certificate(ctx, cert) || !SSL_CTX_use_PrivateKey(ctx, key)) die("certificate");
    SSL *side[2] = {make_side(ctx, fd[0], 0), make_side(ctx, fd[1], 1)}; /* 0 client, 1 server */
    int done[2] = {0, 0};
    for (int round = 0; round < 200 && !(done[0] && done[1]); ++round)
        for (int k = 0; k < 2; ++k) {
            if (done[k]) continue;
            const int r = SSL_do_handshake(side[k]);
            if (r == 1) {
                done[k] = 1;
                continue;
            }
            const int e = SSL_get_error(side[k], r);
            if (e != SSL_ERROR_WANT_READ && e != SSL_ERROR_WANT_WRITE) die("handshake");
        }
    if (!(done[0] && done[1])) die("handshake did not finish");
    printf("ready\n");
    fflush(stdout);

    static char line[2 * MAXREC + 64];
    static unsigned char buf[MAXREC], rec[MAXREC];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "quit", 4)) break;
        if (!strncmp(line, "keys", 4)) {
            unsigned char m[48], cr[32], sr[32];
            if (SSL_SESSION_get_master_key(SSL_get_session(side[0]), m, sizeof m) != 48) die("master key");
            SSL_get_client_random(side[0], cr, sizeof cr);
            SSL_get_server_random(side[0], sr, sizeof sr);
            put_hex("master", m, 48);
            put_hex("client_random", cr, 32);
            put_hex("server_random", sr, 32);
            printf("cipher %s\n", SSL_get_cipher_name(side[0]));
            fflush(stdout);
        } else if (!strncmp(line + 1, "write ", 6) && (line[0] == 'c' || line[0] == 's')) {
            const int k = line[0] == 's', n = unhex(line + 7, buf, sizeof buf);
            if (n <= 0 || SSL_write(side[k], buf, n) != n) die("SSL_write");
            const ssize_t r = recv(fd[1 - k], rec, sizeof rec, 0); /* off the wire, at the other end */
            if (r <= 0) die("no datagram after SSL_write");
            put_hex("record", rec, (size_t)r);
        } else if (!strncmp(line + 1, "inject ", 7) && (line[0] == 'c' || line[0] == 's')) {
            const int k = line[0] == 's', n = unhex(line + 8, buf, sizeof buf);
            if (n <= 0 || send(fd[1 - k], buf, (size_t)n, 0) != n) die("inject"); /* arrives at side k's socket */
            printf("ok\n");
            fflush(stdout);
        } else if (!strncmp(line + 1, "read", 4) && (line[0] == 'c' || line[0] == 's')) {
            const int k = line[0] == 's';
            const int r = SSL_read(side[k], buf, sizeof buf);
            if (r > 0) {
                put_hex("plain", buf, (size_t)r);
            } else {
                printf("none\n");
                fflush(stdout);
            }
        } else {
            die("unknown command");
        }
    }
    SSL_free(side[0]);
    SSL_free(side[1]);
    X509_free(cert);
    EVP_PKEY_free(key);
    SSL_CTX_free(ctx);
    close(fd[0]);
    close(fd[1]);
    return 0;
}
