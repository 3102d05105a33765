/*
 * qgcm.h -- C ABI of the MI355X-native AES-256-GCM packet sealer (libqgcm.so).
 *
 * This is the drop-in boundary for quantum's Encryption plugin path.  Every entry point
 * names the reference interface it replaces (paths relative to the quantum tree):
 *
 *   crypto/aes.go:22-26   type AES {block, aead, salt}        -> qgcm_ctx + key slot (key_idx)
 *   crypto/aes.go:65-83   NewAES(secret, salt)                -> qgcm_derive_key + qgcm_set_key
 *   crypto/aes.go:41-52   (*AES).Encrypt(data, length, aad)   -> qgcm_seal_one / qgcm_seal_batch
 *   crypto/aes.go:57-62   (*AES).Decrypt(data, aad)           -> qgcm_open_one / qgcm_open_batch
 *   crypto/aes.go:29-36   EncryptedSize / DecryptedSize       -> QGCM_OVERHEAD (= 16 + 12)
 *   crypto/ecdh.go:13-31  GenerateECKeyPair / GenerateSharedSecret -> qgcm_x25519*
 *   plugin/encryption.go:16-40 Encryption.Apply calls Encrypt/Decrypt per packet (qgcm_seal_one /
 *                         qgcm_open_one); workers that batch their packets call the host or device
 *                         batch entry points instead.
 *   worker/outgoing.go:28-35, worker/incoming.go:28-34 resolve -> router/router.go:21-31 Resolve
 *                         -> qgcm_routes_set + qgcm_resolve_outgoing / qgcm_resolve_incoming
 *   worker/outgoing.go:37-53 stats, metric/aggregator.go:24-68 -> qgcm_route_account / qgcm_route_stats
 *   Outgoing.pipeline / Incoming.pipeline for a batch         -> qgcm_route_seal_host / qgcm_route_open_host
 *   main.go:41-51 plugin order, compression.go:31-33 / encryption.go:17-19 SupportedPlugins gate
 *                         -> qgcm_peer_plugins_set + qgcm_chain_outgoing / qgcm_chain_incoming,
 *                            qgcm_route_account_bytes, qgcm_route_chain_seal_host / qgcm_route_chain_open_host
 *   socket/udp.go:44-47 Write(payload, mapping)               -> qgcm_udp_send_slots_to, or grouped per peer:
 *                                                                qgcm_send_plan + qgcm_udp_send_plan, or with
 *                                                                the trains packed on the GPU: qgcm_train_pack +
 *                                                                qgcm_udp_send_packed /
 *                                                                qgcm_route_chain_seal_packed_host
 *   socket/udp.go:35-41 Read() for a batch                    -> qgcm_udp_recv_slots, or coalesced (UDP_GRO):
 *                                                                qgcm_udp_recv_gro + qgcm_gro_unpack /
 *                                                                qgcm_gro_resolve (unpack and resolve in one
 *                                                                launch) / qgcm_route_chain_open_gro_host
 *   device/tun.go:60-63 Write(payload) for a batch            -> qgcm_tun_write_slots, or packed on the GPU:
 *                                                                qgcm_deliver_pack + qgcm_tun_write_packed /
 *                                                                qgcm_route_chain_open_gro_packed_host
 *   device/tun.go:51-57 Read() for a batch                    -> qgcm_tun_read_slots, or packed: qgcm_tun_read_packed +
 *                                                                qgcm_frames_resolve, or as TSO / USO super-frames
 *                                                                cut on the GPU: qgcm_tun_open_offload +
 *                                                                qgcm_tun_read_gso + qgcm_gso_resolve /
 *                                                                qgcm_route_chain_seal_gso_host
 *
 * Error convention follows the reference's own cgo layer (crypto/dtls.go:37-40, dtls.h:43-48):
 * constructors return NULL and fill a caller-supplied error buffer; everything else returns
 * a negative QGCM_E* code (see qgcm_strerror) or, for the per-packet calls, -1 exactly where the
 * Go method returns an error.  All functions are thread-safe unless stated otherwise.
 *
 * Packet slot layout (common/payload.go:7-45, common/common.go:16-38): a slot is one
 * common.Payload.Raw buffer: [0:4) sender private IPv4 = the GCM additional data,
 * [4:4+L) payload.  Sealing writes ct over the payload, then tag (16 B) and nonce (12 B):
 * [4:4+L) ct, [4+L:4+L+16) tag, [4+L+16:4+L+28) nonce -- exactly crypto/aes.go:49-51.
 * Slot offsets must be multiples of 4; slots need capacity 4+L+28 bytes.
 *
 * Device pointers are HIP device pointers on the context's device; `stream` is a hipStream_t
 * (NULL = the null stream).  Batch calls are asynchronous with respect to the host.
 */
#ifndef QGCM_H
#define QGCM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QGCM_KEY_BYTES 32    /* crypto/crypto.go:7 keyLength */
#define QGCM_SALT_BYTES 32   /* crypto/aes.go:17 SaltLength */
#define QGCM_NONCE_BYTES 12  /* cipher.NewGCM standard nonce */
#define QGCM_TAG_BYTES 16    /* cipher.NewGCM standard tag (aead.Overhead()) */
#define QGCM_OVERHEAD 28     /* EncryptedSize - len = Overhead + NonceSize, crypto/aes.go:29-36 */
#define QGCM_PBKDF2_ITERS 10000 /* crypto/aes.go:18 */
#define QGCM_MAX_PAYLOAD (1u << 28) /* largest plaintext per packet (GCM allows 2^36-32; packets are <= 9000) */
#define QGCM_ERRLEN 120      /* crypto/dtls.go:23 errorLen */
#define QGCM_MAX_AAD 16384   /* longest additional data of a per-packet call (qgcm_seal_one / qgcm_open_one) */
#define QGCM_MAX_BATCH (1u << 31) /* packets per batch call (tile indices stay 32-bit); more -> QGCM_E_ARG */
/* largest max_keys of a context: the descriptor sort key is key_idx << 12 | length rank, 32 bits, and
 * its all-ones value marks excluded packets, so key index 2^20 - 1 is reserved */
#define QGCM_MAX_KEYS ((1u << 20) - 1)

/* status codes */
#define QGCM_OK 0
#define QGCM_E_ARG -1       /* bad argument / size */
#define QGCM_E_HIP -2       /* HIP runtime error */
#define QGCM_E_KEY -3       /* key index not set or out of range */
#define QGCM_E_AUTH -4      /* message authentication failed (errOpen) */
#define QGCM_E_NOMEM -5

typedef struct qgcm_ctx qgcm_ctx;

/* One packet descriptor of a device batch.  For seal, len = payload length L
 * (Encrypt's `length`); for open, len = sealed length L+28 (len(Payload.Packet) as
 * passed to Decrypt).  offset = byte offset of the slot (the Raw buffer) in the arena. */
typedef struct qgcm_desc {
    uint64_t offset;
    uint32_t len;
    uint32_t key_idx;
} qgcm_desc;

/* ---- context (replaces the per-process Go AEAD objects) ---- */
/* max_keys in [1, QGCM_MAX_KEYS].  Key slots start unset: a packet naming an unset slot fails (status 0,
 * slot untouched; QGCM_E_KEY / -1 from the uniform and per-packet calls), as Apply would on a peer
 * whose Mapping.AES is nil (common/mapping.go:94-99 leaves it nil when the peer published no keys). */
qgcm_ctx *qgcm_create(int device, uint32_t max_keys, char *err, int errlen);
void qgcm_destroy(qgcm_ctx *ctx);
const char *qgcm_strerror(int code);
const char *qgcm_version(void);
/* HIP devices this process sees (0 when there are none or the runtime fails).  The Go drop-in's
 * process-wide device set (go/crypto/aes_gpu.go, QGCM_DEVICES unset) is every one of them. */
int qgcm_device_count(void);

/* ---- key setup: crypto/aes.go:65-83 NewAES, common/mapping.go:90-99 ---- */
/* key = PBKDF2-HMAC-SHA512(secret, salt, 10000, 32)  (crypto/aes.go:66) -- host */
int qgcm_derive_key(const uint8_t *secret, size_t secret_len, const uint8_t *salt, size_t salt_len,
                    uint8_t key[QGCM_KEY_BYTES]);
/* Batched: keys[i] = PBKDF2(secrets[i], salts[i]) for count peers, multithreaded host. */
int qgcm_derive_keys(const uint8_t *secrets, const uint8_t *salts, uint32_t count, uint8_t *keys);
/* aes.NewCipher + cipher.NewGCM (crypto/aes.go:68-76): expands round keys and the GHASH
 * tables on the device for slot key_idx.  Synchronous. */
int qgcm_set_key(qgcm_ctx *ctx, uint32_t key_idx, const uint8_t key[QGCM_KEY_BYTES]);
int qgcm_set_keys(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t *keys);
/* ---- peer keys derived on the GPU (batched NewAES; DESIGN.md "Peer keys derived on the GPU") ---- */
/* keys[i] = PBKDF2-HMAC-SHA512(secrets[i], salts[i], iters, 32) for count 32-byte secrets and salts, derived
 * on ctx's GPU; host arrays in and out; the same bytes as qgcm_derive_keys when iters = QGCM_PBKDF2_ITERS.
 * iters in [1, 2^20].  Synchronous.  One key per GPU lane: a key takes longer than on a CPU core, a table
 * of a few hundred keys or more takes less than on all of them.  Errors in this order: NULL ctx, or a NULL
 * array with count > 0: QGCM_E_ARG; count 0: QGCM_OK; iters out of range: QGCM_E_ARG (keys untouched). */
int qgcm_derive_keys_device(qgcm_ctx *ctx, const uint8_t *secrets, const uint8_t *salts, uint32_t count,
                            uint32_t iters, uint8_t *keys);
/* NewAES for a whole peer table: derives count keys (QGCM_PBKDF2_ITERS) and installs key i in slot
 * first_idx + i.  Argument errors as qgcm_set_keys (QGCM_E_ARG, then QGCM_E_KEY for first_idx + count >
 * max_keys with nothing derived or installed, then QGCM_OK for count 0).  Derives on the GPU when count >=
 * QGCM_KDF_DEVICE_MIN (environment, read at qgcm_create: 0 = never, 1 = always; default 576), else with
 * qgcm_derive_keys on the host; both install the same bytes.  On the device path the key bytes never come
 * back to the host.  The derivation holds none of the context's I/O locks (it runs on a stream of its own,
 * created by the first device derivation; derivations of one context are serialised): seals, opens and
 * per-packet calls on keys already installed go on meanwhile.  The install that follows is one pass like
 * qgcm_set_keys: synchronous, ends the resident instance once. */
int qgcm_derive_set_keys(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t *secrets,
                         const uint8_t *salts);
/* {keys derived on the device, keys derived on the host by qgcm_derive_set_keys, KDF kernel launches,
 *  install passes}; writes min(n, 4) values, returns that number or -1.  An install pass is one locked
 *  update of the key tables: every qgcm_set_key(s) call is one, and so is every qgcm_derive_set_keys. */
int qgcm_kdf_stats(const qgcm_ctx *ctx, uint64_t *out, int n);

/* Marks key slots [first_idx, first_idx + count) unset (the slot's AES was released: go/crypto/aes_gpu.go's
 * finalizer, crypto::DeviceSet::Release).  Afterwards every call naming one of them fails as for a key never
 * set (per-packet calls -1 / QGCM_E_KEY, descriptor batches status 0) until qgcm_set_key(s) installs a new
 * key there, so a stale key index never seals or opens under the slot's next peer.  Synchronous; ends the
 * resident instance like qgcm_set_keys. */
int qgcm_clear_keys(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count);
/* X25519 (crypto/ecdh.go:13-31): pub = X25519(priv, 9); secret = X25519(priv, peer_pub). */
int qgcm_x25519_base(uint8_t pub[32], const uint8_t priv[32]);
int qgcm_x25519(uint8_t secret[32], const uint8_t priv[32], const uint8_t peer_pub[32]);
/* ---- a peer table keyed from public keys on the GPU (batched X25519; DESIGN.md "Peer secrets computed on
 * the GPU") ---- */
/* out[i] = X25519(scalars[i * scalar_stride .. +32), points[i]); scalar_stride 0 (one scalar for all) or 32.
 * Host, multithreaded like qgcm_derive_keys.  The semantics of qgcm_x25519: the scalar is clamped, bit 255 of
 * a point is ignored, nothing is refused (a small-order point gives the all-zero output).  A NULL array with
 * count > 0, or another stride: QGCM_E_ARG. */
int qgcm_x25519_batch(const uint8_t *scalars, uint32_t scalar_stride, const uint8_t *points, uint32_t count,
                      uint8_t *out);
/* The same bytes computed on ctx's GPU, one ladder per lane; host arrays in and out.  Synchronous.  Errors in
 * this order: NULL ctx, or a NULL array with count > 0: QGCM_E_ARG; another stride: QGCM_E_ARG; count 0:
 * QGCM_OK.  A failed call leaves out untouched. */
int qgcm_x25519_device(qgcm_ctx *ctx, const uint8_t *scalars, uint32_t scalar_stride, const uint8_t *points,
                       uint32_t count, uint8_t *out);
/* common/mapping.go:90-99 for a table, on ctx's GPU: keys[i] = PBKDF2-HMAC-SHA512(X25519(priv_key,
 * pub_keys[i]), X25519(priv_salt, pub_salts[i]), QGCM_PBKDF2_ITERS, 32).  One ladder launch over 2 * count
 * lanes, then the derivation kernel, on the context's derivation stream; only the keys come back.
 * Synchronous. */
int qgcm_peer_keys_device(qgcm_ctx *ctx, const uint8_t priv_key[32], const uint8_t priv_salt[32],
                          const uint8_t *pub_keys, const uint8_t *pub_salts, uint32_t count, uint8_t *keys);
/* The same, installed in slots first_idx + i.  Argument errors as qgcm_derive_set_keys (NULL: QGCM_E_ARG;
 * first_idx + count > max_keys: QGCM_E_KEY with nothing computed; count 0: QGCM_OK).  Runs on the GPU when
 * count >= QGCM_KDF_DEVICE_MIN -- the secrets, salts and keys then never reach the host -- else
 * qgcm_x25519_batch and qgcm_derive_keys on the host; both install the same bytes.  Locks, the install pass
 * and the four qgcm_kdf_stats counters are those of qgcm_derive_set_keys for the same count. */
int qgcm_peers_set_keys(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t priv_key[32],
                        const uint8_t priv_salt[32], const uint8_t *pub_keys, const uint8_t *pub_salts);
/* {ladders run on the device, ladders run on the host by qgcm_peers_set_keys, ladder kernel launches};
 * writes min(n, 3) values, returns that number or -1. */
int qgcm_ecdh_stats(const qgcm_ctx *ctx, uint64_t *out, int n);

/* ---- device batches (the throughput path) ---- */
/* Seal n packets in place.  nonces: device array of n*12 bytes (nonce i for packet i, written
 * into the slot like crypto/aes.go:50), or NULL to use the nonce already present at
 * [4+L+16, 4+L+28) of each slot, or QGCM_NONCES_GENERATE to have the library draw them on the GPU (see
 * "nonce source" below; the same three forms in every batch seal).  aad_len: 0 (nil additional) or 4 (the Payload IP header).
 * status (device, n bytes, may be NULL): 1 = sealed, 0 = rejected (key index out of range or never set,
 * payload of QGCM_MAX_PAYLOAD or more; the slot is untouched). */
int qgcm_seal_batch(qgcm_ctx *ctx, uint8_t *d_arena, const qgcm_desc *d_descs, uint32_t n,
                    const uint8_t *d_nonces, uint32_t aad_len, uint8_t *d_status, void *stream);
/* Open n packets in place.  status[i] = 1 if authentic (plaintext at [4, 4+len-28)),
 * 0 on errOpen (tag mismatch: plaintext region zeroed as Go 1.9 gcm.Open does;
 * len < 28: slot untouched). */
int qgcm_open_batch(qgcm_ctx *ctx, uint8_t *d_arena, const qgcm_desc *d_descs, uint32_t n,
                    uint32_t aad_len, uint8_t *d_status, void *stream);
/* Uniform batches: slot i at i*stride, same length and key for all packets (no descriptor
 * traffic).  seal: len = L; open: len = L + 28. */
int qgcm_seal_uniform(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t len,
                      uint32_t key_idx, const uint8_t *d_nonces, uint32_t aad_len,
                      uint8_t *d_status, void *stream);
int qgcm_open_uniform(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t len,
                      uint32_t key_idx, uint32_t aad_len, uint8_t *d_status, void *stream);

/* ---- per-packet host calls, the exact Encrypt/Decrypt contract ---- */
/* crypto/aes.go:41-52: seals data[0:length] in place, appends tag and nonce; data must have
 * capacity length+28.  nonce NULL -> 12 fresh bytes from getrandom(2) as crypto/rand does.
 * aad may be NULL (aad_len 0); aad_len may be anything in [0, QGCM_MAX_AAD], as cipher.AEAD takes
 * additional data of any length.  Calls with aad_len <= 4 (nil, or the Payload IP header) are served
 * on every path, payloads that fall through to the batch kernel included.  Calls with aad_len > 4
 * are served by the latency engine alone, when the record and the additional data fit its staging
 * area together:
 *   ((4 + length + 28 + 15) & ~15) + ((aad_len + 15) & ~15) <= 32752
 * (every packet quantum can produce fits this many times over).  Anything larger returns -1 and leaves
 * data untouched; so does every aad_len > 4 on a context created with QGCM_ONE_KERNEL=0 (that A/B knob
 * forces the batch kernel, which has no long-AAD form).  Returns length+28, or -1. */
long qgcm_seal_one(qgcm_ctx *ctx, uint32_t key_idx, uint8_t *data, long length, const uint8_t *aad,
                   uint32_t aad_len, const uint8_t *nonce);
/* crypto/aes.go:57-62: opens data[0:len] in place.  Returns len-28, or -1 (errOpen; data[0:len-28]
 * zeroed on tag mismatch; len < 28 leaves data untouched -- the reference panics below 12).
 * aad_len as for qgcm_seal_one: [0, QGCM_MAX_AAD]; beyond 4 bytes the call is served when
 *   ((4 + len + 15) & ~15) + ((aad_len + 15) & ~15) <= 32752
 * and the context was not created with QGCM_ONE_KERNEL=0, else it returns -1 with data untouched. */
long qgcm_open_one(qgcm_ctx *ctx, uint32_t key_idx, uint8_t *data, long len, const uint8_t *aad,
                   uint32_t aad_len);

/* Per-packet calls are served by a RESIDENT kernel (16 workgroups by default, QGCM_RESIDENT_WORKERS;
 * 16 request slots each, QGCM_RESIDENT_SLOTS), so a call costs no launch: the caller writes its packet and
 * a 16-B request record into fine-grained DEVICE memory through the PCIe BAR (the CPU agent is granted
 * access with hsa_amd_agents_allow_access), the workers poll those records in their own HBM, and write
 * the result and a done word into pinned host memory that the caller watches.  Without CPU access to that
 * memory (or QGCM_RESIDENT=0), and for payloads past ~16 KiB, every call takes a gcm_one_kernel launch
 * instead; qgcm_resident_stats says which served (requests served, instances launched).
 * The kernel is started by the first call and ends by itself after QGCM_RESIDENT_IDLE_US (2000) without
 * a request or QGCM_RESIDENT_LIFE_US (8000) of life, after serving what is pending (the next call starts
 * it again): work queued behind it on a shared hardware queue, or a device-wide synchronize, waits that
 * long at most.  qgcm_set_key(s) and qgcm_destroy end it too (it caches key tables).
 * Per-packet calls of up to 2016 B hash with per-key tables of H^1..H^128 (6-bit combs, 2.75 MiB of
 * device memory per key slot, built by qgcm_set_key(s)) for the first QGCM_FLAT_GHASH_KEYS slots
 * (default min(max_keys, 256); 0 = off: every packet takes the slower chained GHASH).
 * A seal without a caller's nonce draws the nonce of its slot's NEXT seal too and hands it to the worker,
 * which computes that nonce's counter blocks while idle (QGCM_RESIDENT_AHEAD=0: off); the next seal
 * on the slot uses that nonce (drawn from getrandom like any other, used once) and skips the counter
 * blocks.  qgcm_resident_stop ends it now; qgcm_resident_stats writes {requests served, instances
 * launched, request slots, workers running now, seals served from a keystream computed ahead, callers
 * asleep now, callers spinning now, 1 if the resident path has failed and every call takes the launch
 * path} (min(n, 8) values, returns that number or -1).  qgcm_set_key(s) ends the instance before it
 * changes the key tables and holds the next one back until the new keys are published; a per-packet call
 * racing it waits (or, if the context's resident service was not started yet, starts it). */
int qgcm_resident_stop(qgcm_ctx *ctx);
int qgcm_resident_stats(const qgcm_ctx *ctx, uint64_t *out, int n);

/* ---- host batches (end-to-end incl. PCIe) ---- */
/* Slots in host memory at i*stride; copies in, runs the device batch, copies back, synchronously.
 * Pipelined in 64 MiB chunks over 3 streams (H2D of chunk c+1 || kernel c || D2H of chunk c-1);
 * h_arena from qgcm_host_alloc (pinned) is DMA'd in place, pageable memory is staged by HIP.  A pinned
 * batch of up to 65536 packets (128 MiB) with 16-B-aligned slots (stride a multiple of 16) is sealed in place
 * instead: one kernel on the arena's device view, no copies (QGCM_HOST_DIRECT=0 disables it).
 * Returns the number of packets that failed (0 = all ok) or a negative error.  status may be NULL.
 * Replaces the per-packet Apply loop of worker/outgoing.go:55-93 / worker/incoming.go:54-92 for a
 * batch of packets a worker has collected. */
int qgcm_seal_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t len,
                   uint32_t key_idx, const uint8_t *h_nonces, uint32_t aad_len, uint8_t *h_status);
int qgcm_open_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t len,
                   uint32_t key_idx, uint32_t aad_len, uint8_t *h_status);

/* ---- several GPUs behind one process (quantum is one process: main.go:29-114, 72-75) ---- */
/* A group of `count` member contexts, member k on devices[k] (members may share a device, but then share
 * its hardware queues and PCIe link: one member per GPU is the intended layout).  Keyed
 * traffic is hash-sharded: key index k belongs to member qgcm_group_shard(k) = ((k * 0x9E3779B97F4A7C15)
 * mod 2^64 >> 32) mod count (quantum_amd/shard.py key_shard), so a peer's packets stay on
 * one GPU and each member holds only its peers' keys.  No collective, no GPU-to-GPU traffic.
 * NULL + err on failure. */
typedef struct qgcm_group qgcm_group;
qgcm_group *qgcm_group_create(const int *devices, int count, uint32_t max_keys, char *err, int errlen);
void qgcm_group_destroy(qgcm_group *g);
int qgcm_group_size(const qgcm_group *g);
qgcm_ctx *qgcm_group_ctx(qgcm_group *g, int member);  /* member's context (device batches on it) */
/* Number of CPUs member's host thread is pinned to: its GPU's NUMA-local CPUs (sysfs local_cpulist of
 * the PCI device) that the process may use; 0 = not pinned (no sysfs answer). */
int qgcm_group_member_cpus(const qgcm_group *g, int member);
int qgcm_group_shard(const qgcm_group *g, uint32_t key_idx);
/* Installs keys[i] as key first_idx + i on its owning member only (qgcm_set_keys there). */
int qgcm_group_set_keys(qgcm_group *g, uint32_t first_idx, uint32_t count, const uint8_t *keys);
/* qgcm_derive_set_keys over the group: each member gets the secrets and salts of the key indices it owns
 * (qgcm_group_shard), all members derive at once (one host thread each; device or host by each member's
 * own share and threshold), and each installs its keys in ONE pass, however its indices are scattered
 * (qgcm_group_set_keys makes one qgcm_set_keys call per run of consecutive indices).  Returns the first
 * member's error; members that finished keep the keys they installed. */
int qgcm_group_derive_set_keys(qgcm_group *g, uint32_t first_idx, uint32_t count, const uint8_t *secrets,
                               const uint8_t *salts);
/* qgcm_peers_set_keys over the group: each member gets the public values of the key indices it owns
 * (qgcm_group_shard), all members work at once (ladders and derivation on each member's GPU or host by its
 * own threshold), one install pass per member.  Errors as qgcm_group_derive_set_keys. */
int qgcm_group_peers_set_keys(qgcm_group *g, uint32_t first_idx, uint32_t count, const uint8_t priv_key[32],
                              const uint8_t priv_salt[32], const uint8_t *pub_keys, const uint8_t *pub_salts);
/* qgcm_clear_keys on the owning member of each key index. */
int qgcm_group_clear_keys(qgcm_group *g, uint32_t first_idx, uint32_t count);
/* Host batches over the group: packet i is the Raw slot at h_arena + h_descs[i].offset (seal: len = L,
 * capacity 4 + L + 28; open: len = L + 28), any key mix.  Packets are split by owner; one host thread and
 * one stream set per member gathers its packets into pinned staging, copies them to its device, runs the
 * descriptor batch, copies back and writes the results into the same slots (input order kept).
 * h_nonces: n * 12 B (seal; NULL = nonce already in the slot; QGCM_NONCES_GENERATE = each member draws its
 * packets' nonces on its GPU).  h_status[i] (may be NULL): 1 ok, 0 failed
 * (as qgcm_seal_batch / qgcm_open_batch).  Returns the number of failed packets or a negative error.
 * One call at a time per group (calls are serialized).  When h_arena (and h_nonces) is pinned host memory
 * (qgcm_host_alloc, hipHostMalloc, hipHostRegister) holding every record, the members' GPUs gather and
 * scatter the records themselves over PCIe (zero-copy); otherwise host threads copy them through pinned
 * staging (QGCM_GROUP_THREADS per member); so does a batch with a record offset that is not a multiple of
 * 4.  QGCM_GROUP_ZEROCOPY=0 forces the copy path. */
int qgcm_group_seal_host(qgcm_group *g, uint8_t *h_arena, const qgcm_desc *h_descs, uint32_t n,
                         const uint8_t *h_nonces, uint32_t aad_len, uint8_t *h_status);
int qgcm_group_open_host(qgcm_group *g, uint8_t *h_arena, const qgcm_desc *h_descs, uint32_t n, uint32_t aad_len,
                         uint8_t *h_status);
/* 1 if the last qgcm_group_seal_host / open_host call took the zero-copy path on every member, else 0. */
int qgcm_group_last_zerocopy(const qgcm_group *g);
/* DMA runs: when the descriptors are in arena order (offsets nondecreasing, multiples of 4) and a member's
 * packets form runs of adjacent records (consecutive packets, at most 256 B between one record's end and
 * the next one's start) averaging 64 KiB or more, that member copies each run to and from its device with
 * one DMA each way (64 MiB chunks, three staging slots, three streams), with no gather, scatter or
 * shader-driven PCIe traffic;
 * the gap bytes inside a run go back unchanged.  A batch laid out in qgcm_group_order's order, or any batch
 * of a one-member group, takes it.  A chunk of at most 8192 packets whose records all start 16-B aligned
 * runs one workgroup per packet instead of the sorted worklist (QGCM_DESC_ONE=0 disables that).
 * Direct: a member's share of up to 65536 packets (128 MiB) whose records all start 16-B aligned, in a
 * pinned arena that also holds each record's 16-B-rounded area, is sealed in place by that kernel over
 * PCIe with no copies, whether the members' records are adjacent or interleaved (QGCM_GROUP_DIRECT=0
 * disables it).
 * QGCM_GROUP_DMA=0 disables the DMA runs.  qgcm_group_last_path: the path member
 * took in the last call (0 host copies, 1 zero-copy, 2 DMA runs, 3 direct) or QGCM_E_ARG. */
int qgcm_group_last_path(const qgcm_group *g, int member);
/* The order in which to lay out a keyed batch so that each member's packets are contiguous (a stable
 * counting sort by qgcm_group_shard): order[0..n) = input indices, member by member; member_counts
 * (may be NULL) receives each member's packet count.  A caller that assembles its batch in this order
 * gets the DMA-run path.  Returns QGCM_OK or QGCM_E_ARG. */
int qgcm_group_order(const qgcm_group *g, const uint32_t *key_idx, uint32_t n, uint32_t *order,
                     uint32_t *member_counts);

/* Pinned (page-locked) host memory for arenas handed to the *_host calls; NULL on failure. */
void *qgcm_host_alloc(size_t bytes);
void qgcm_host_free(void *p);

/* ---- nonce source for production seals (crypto/aes.go:42-47 draws per packet) ---- */
/* Fills n*12 bytes of host memory from getrandom(2). */
int qgcm_random_nonces(uint8_t *h_out, uint32_t n);
/* Nonces generated on the GPU.  Each context owns an AES-256-CTR generator (SP 800-38A counter mode): a
 * key K (32 B) and a 128-bit counter V, both drawn from getrandom(2) on first use.  Nonce number j of the
 * stream is the first 12 bytes of AES-256_K(BE128(V0 + j)), the counter a big-endian 128-bit integer.  A
 * call that needs n nonces reserves [V, V + n) and carries its own copy of the round keys to the device,
 * so calls on different streams or threads never share a position and never see each other's reseed.
 * Reseed rule: before reserving, when at least one nonce was drawn since the last (re)seed and that count
 * plus n would exceed the reseed interval (QGCM_NONCE_RESEED at qgcm_create, default 2^32), K and V are
 * drawn anew from getrandom(2); one call always uses one key.  GCM needs nonces that never repeat under a
 * key, not secret ones: they travel in the clear behind every packet.
 *
 * QGCM_NONCES_GENERATE as the nonce argument of qgcm_seal_uniform, qgcm_seal_batch, qgcm_seal_host or
 * qgcm_group_seal_host: the library writes nonce j of the call's reservation into packet j's nonce field
 * ([4+L+16, 4+L+28) of the slot) with a kernel on the call's stream, then seals with the nonce in the
 * slot.  No nonce array, no host round trip; pinned arenas sealed in place get their nonces over PCIe from
 * the same kernel.  A packet the seal rejects (status 0) gets no nonce -- its slot stays untouched -- but
 * keeps its stream position.  A call refused with QGCM_E_ARG or QGCM_E_KEY, or with n = 0, draws nothing.
 * Group calls draw from each member's own context.  qgcm_compress_seal_host does not take it (QGCM_E_ARG).
 * QGCM_E_NOMEM from such a call: getrandom(2) failed, nothing was written. */
#define QGCM_NONCES_GENERATE ((const uint8_t *)(uintptr_t)1)
/* Writes the next n nonces of ctx's generator to d_out (device memory, n*12 bytes, 4-B aligned).
 * Asynchronous on stream. */
int qgcm_nonce_fill(qgcm_ctx *ctx, uint8_t *d_out, uint32_t n, void *stream);
/* Sets the generator's key and counter (BE128) and restarts the reseed count: the hook for known-answer
 * tests and reproducible runs.  Two contexts seeded alike produce the same nonces -- never do that with a
 * key that seals traffic.  key NULL (counter ignored): reseed from getrandom(2) now. */
int qgcm_nonce_seed(qgcm_ctx *ctx, const uint8_t key[32], const uint8_t counter[16]);

/* ---- snappy block format: the compression plugin (plugin/compression.go) ---- */
/* Host codec (C++; golang/snappy is not in the reference).  Encode restates golang/snappy's block
 * encoder (compression.go:17 snappy.Encode), the same bytes as libsnappy 1.1.8 (tests/golden/
 * snappy.json); Decode accepts every valid stream and returns -1 on malformed input
 * (compression.go:22-25 decode error). */
size_t qgcm_snappy_max_compressed_length(size_t n);
long qgcm_snappy_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap);
long qgcm_snappy_uncompressed_length(const uint8_t *src, size_t n);
long qgcm_snappy_uncompress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap);
/* Payload.Raw slots at i*stride: packet i = lens[i] bytes at slot+4, (de)compressed in place,
 * lens[i] updated (compression.go Apply, Outgoing / Incoming), `threads` host workers.  Returns the
 * number of packets that failed (untouched; status[i] = 0) or -1. */
int qgcm_snappy_compress_slots(uint8_t *arena, uint64_t stride, uint32_t n, uint32_t *lens, int threads);
/* As qgcm_snappy_compress_slots, but a packet also fails when its compressed form exceeds `limit`
 * bytes (room left for the seal's tag and nonce); status[i] = 1 ok / 0 failed (may be NULL). */
int qgcm_snappy_compress_slots_limit(uint8_t *arena, uint64_t stride, uint32_t n, uint32_t *lens, uint64_t limit,
                                     uint8_t *status, int threads);
int qgcm_snappy_uncompress_slots(uint8_t *arena, uint64_t stride, uint32_t n, uint32_t *lens,
                                 uint8_t *status, int threads);
/* Device codec (gfx950, one wave per packet), the same bytes as the host codec: Payload.Raw slots at
 * i*stride in device memory (stride a multiple of 4), packet i = d_lens[i] bytes at slot+4, replaced
 * in place (compression.go:39-51), d_lens[i] updated.  compress: packets longer than max_len, or
 * whose compressed form exceeds limit, fail; uncompress: packets longer than max_len, that do not
 * decode, or that decode to more than cap bytes fail.  A failed packet's slot and length are
 * untouched (d_status[i] = 0; 1 = ok; may be NULL).  All limits are at most stride - 4; compress's
 * max_len and uncompress's cap at most QGCM_SNAPPY_DEVICE_MAX, uncompress's max_len at most
 * qgcm_snappy_max_compressed_length(QGCM_SNAPPY_DEVICE_MAX).  compress also writes, when d_descs_out is
 * not NULL, the seal descriptor of each packet ({i*stride, compressed length, key_idx}; a failed packet
 * gets length QGCM_MAX_PAYLOAD, which the seal rejects), so qgcm_seal_batch can follow on the stream
 * (the chain main.go:50-51 sorts: compression, then encryption).  Asynchronous on stream. */
#define QGCM_SNAPPY_DEVICE_MAX 16384
int qgcm_snappy_compress_batch(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                               uint32_t max_len, uint32_t limit, uint8_t *d_status, qgcm_desc *d_descs_out,
                               uint32_t key_idx, void *stream);
int qgcm_snappy_uncompress_batch(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                                 uint32_t max_len, uint32_t cap, uint8_t *d_status, void *stream);

/* ---- Compression + Encryption chain (BASELINE config 5) ---- */
/* Host batches in the order main.go:50-51 sorts the plugins: outgoing compression.go then
 * encryption.go Apply, incoming the reverse.  Slot i at i*stride holds [aad 4][packet lens[i] B].
 * compress_seal: snappy-compress each packet in place, then seal it (lens[i] <- compressed + 28).
 * open_uncompress: open each sealed packet, then uncompress (lens[i] <- plaintext length).
 * Chunks pipeline the codec (`threads` host workers and/or the device codec, qgcm_chain_codec) with
 * PCIe copies and the device kernels.
 * Returns the number of failed packets (status 0: codec error, no room for the tag and nonce, or
 * failed authentication -- plaintext zeroed as in qgcm_open_batch), or a negative error. */
int qgcm_compress_seal_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *lens,
                            uint32_t key_idx, const uint8_t *h_nonces, uint32_t aad_len, int threads,
                            uint8_t *h_status);
int qgcm_open_uncompress_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *lens,
                              uint32_t key_idx, uint32_t aad_len, int threads, uint8_t *h_status);
/* Where the chained calls run the snappy codec: 0 = host workers only; 1 = split (default): the device
 * codec takes the chunks the host workers cannot keep up with (seal: the last untouched chunks when a
 * stream slot is free and fewer than two compressed host chunks are waiting; open: when the host decode
 * backlog exceeds two chunks); 2 = device only.  The bytes are the same either way.  Returns the previous mode
 * (mode -1: just read it) or QGCM_E_ARG.  QGCM_CHAIN_DEVICE sets the initial mode. */
int qgcm_chain_codec(qgcm_ctx *ctx, int mode);

/* ---- batched UDP I/O (socket/udp.go:35-70, one syscall per batch) ---- */
/* Datagram i is slot i's Raw[:lens[i]] (wire format [4-B IP][packet]), moved with recvmmsg/sendmmsg
 * straight into / out of a host arena (pinned from qgcm_host_alloc: then also the DMA source of
 * qgcm_*_host).  qgcm_udp_socket binds ip:port (port 0: any; bufbytes > 0 sizes SO_RCVBUF/SNDBUF)
 * and returns the fd or -1.  recv waits up to timeout_ms (-1 forever) for the first datagram and then
 * takes what is queued, up to max_n; returns the count (0 on timeout) or -1.  send returns the
 * number of datagrams sent or -1. */
int qgcm_udp_socket(const char *ip, int port, int bufbytes);
/* One queue of a multi-queue socket (socket/udp.go:55-70: one per worker on the same address):
 * SO_REUSEPORT, so the kernel spreads incoming flows over the queues of the group. */
int qgcm_udp_queue(const char *ip, int port, int bufbytes);
int qgcm_udp_port(int fd);
int qgcm_udp_close(int fd);
int qgcm_udp_recv_slots(int fd, uint8_t *arena, uint64_t stride, uint32_t max_n, uint32_t *lens, int timeout_ms);
int qgcm_udp_send_slots(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                        const char *ip, int port);

/* ---- batched TUN I/O (device/tun.go:51-118) ---- */
/* qgcm_tun_open: device/tun.go:97-118 (createTUN) for `queues` queues of one multi-queue TUN device
 * (IFF_TUN | IFF_NO_PI | IFF_MULTI_QUEUE), fds[i] = queue i; the kernel's device name goes to
 * ifname_out.  qgcm_tun_up: device/tun.go:121-150 (initTun): up, MTU, address/prefix.  Both return 0
 * or -errno.  read_slots: device/tun.go:51-57 batched -- waits up to timeout_ms for the first packet,
 * then drains what the queue holds (up to max_n) into Raw[4:] of slots 0, 1, ... (lens[i] = packet
 * length); returns the count (0 on timeout) or -1.  write_slots: device/tun.go:60-63 batched --
 * writes Raw[4 : 4 + lens[i]]; returns the number written or -1. */
int qgcm_tun_open(const char *name, int queues, int *fds, char *ifname_out, size_t ifname_len);
int qgcm_tun_up(const char *ifname, const char *ip, int prefix, int mtu);
int qgcm_tun_read_slots(int fd, uint8_t *arena, uint64_t stride, uint32_t max_n, uint32_t *lens, int timeout_ms);
int qgcm_tun_write_slots(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens);
int qgcm_tun_close(int fd);

/* ---- routes resolved on the GPU (worker resolve + stats) ---- */
/* The route table: the datastore's private-IP -> mapping map (etcdv2.go:210-234 sync) with the peer's key
 * slot in place of the Mapping, plus the values router/router.go:21-31 resolves with.  Addresses are
 * common.IPtoInt values (common/common.go:42-45): the little-endian uint32 of the four address bytes, so
 * 10.99.0.1 is 0x0100630a.  net / mask: cfg.NetworkConfig.IPNet; gateway: the datastore's gateway address
 * (etcdv2.go:285-288); own_ip: cfg.PrivateIP.
 *
 * qgcm_routes_set replaces the whole table (count 0: an empty one).  A duplicate ip takes its last entry,
 * as a map assignment does.  A peer at or above the context's max_keys: QGCM_E_ARG, nothing installed.
 * Before the first qgcm_routes_set every qgcm_resolve_*, qgcm_route_* call returns QGCM_E_ARG.  The table
 * is built on the host (open addressing, linear probing, a power-of-two capacity of at least 2 * count,
 * 8-byte entries {ip, peer}, peer QGCM_NO_PEER = empty), uploaded into a fresh allocation, and the
 * context's pointer is swapped under the context's route lock.  A launch takes pointer and capacity as
 * kernel arguments: a resolve enqueued before qgcm_routes_set returns sees the old table whole, one
 * enqueued after it the new one whole.  The old table is released with hipFree after the swap, which waits
 * for the device -- so for the launches that use it; qgcm_routes_set is a control-plane call and may take
 * that long.  Keys are not touched: a route may name a slot whose key is not set (its packets then
 * resolve, and the seal rejects them with status 0). */
#define QGCM_NO_PEER 0xffffffffu
typedef struct qgcm_route { uint32_t ip; uint32_t peer; } qgcm_route;
typedef struct qgcm_route_net { uint32_t net, mask, gateway, own_ip; } qgcm_route_net;
int qgcm_routes_set(qgcm_ctx *ctx, const qgcm_route *routes, uint32_t count, const qgcm_route_net *net);
/* One launch turns a batch of raw slots into peer indices and seal / open descriptors.  Slot i at i * stride
 * in device memory (4-B aligned; stride a nonzero multiple of 4), d_lens / d_peer n uint32 each, d_descs n
 * descriptors (16-B aligned); n at most QGCM_MAX_BATCH, n == 0: QGCM_OK, nothing launched.  Bad
 * arguments: QGCM_E_ARG.  Asynchronous on stream.
 *
 * outgoing: d_lens[i] is the TUN packet length (qgcm_tun_read_slots), the packet at slot + 4.  The
 * destination is Packet[16:20] (no IP-version check, as outgoing.go:29 makes none); inside the net
 * ((dst & mask) == (net & mask)) it is looked up itself, else the gateway is (router.go:25-30).  Hit: own_ip
 * into Raw[0:4] (outgoing.go:30), d_peer[i] = peer, d_descs[i] = {i * stride, d_lens[i], peer}.  Miss:
 * d_peer[i] = QGCM_NO_PEER, d_descs[i] = {i * stride, d_lens[i], QGCM_NO_PEER}, the slot untouched byte
 * for byte -- qgcm_seal_batch rejects that key index with status 0 and leaves the slot alone too.
 * incoming: d_lens[i] is the datagram length (qgcm_udp_recv_slots, Raw[:n]); the sender is Raw[0:4], the
 * rule the same (incoming.go:29); d_descs[i] = {i * stride, d_lens[i] - 4, peer or QGCM_NO_PEER}; the arena
 * is only read.
 * Divergences, all treated as a miss: an outgoing packet shorter than 20 bytes (the reference slices
 * stale buffer bytes there); an outgoing packet with 4 + len + 28 > stride (the reference's MTU rules it
 * out); an incoming datagram shorter than 4 bytes (descriptor length 0) or longer than stride. */
int qgcm_resolve_outgoing(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                          uint32_t *d_peer, qgcm_desc *d_descs, void *stream);
int qgcm_resolve_incoming(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                          uint32_t *d_peer, qgcm_desc *d_descs, void *stream);
/* Link metrics (metric.Metrics, metric/aggregator.go:24-32): per direction the context holds four uint64
 * counters {Packets, Bytes, DroppedPackets, DroppedBytes} for the totals and four per key slot for the
 * links, in device memory, zero at the first qgcm_routes_set.  qgcm_route_account adds one batch, after its
 * seal (QGCM_TX) or open (QGCM_RX) on the same stream: d_descs are the descriptors that call took, d_status
 * its status array (NULL: every resolved packet was delivered).  With len = d_descs[i].len:
 *   d_peer[i] == QGCM_NO_PEER:  totals DroppedPackets += 1, bytes 0 (resolve returned nil: outgoing.go:34,
 *                               incoming.go:33, stats at :44-50); no link
 *   delivered, Tx:              totals and link  Packets += 1, Bytes += 4 + len + 28 (encryption.go:36-37)
 *   delivered, Rx:              totals and link  Packets += 1, Bytes += 4 + len - 28
 *   resolved but status 0:      totals and link  DroppedPackets += 1, DroppedBytes += 4 + len (Apply
 *                               returned its inputs: the length the packet came with)
 * An Rx packet with len < 28 counts as dropped whatever its status (the open rejects it); a d_peer[i] at or
 * above max_keys counts as unresolved.  The sums are exact integers, added with 64-bit atomics after the
 * packets of a wave and of a workgroup that share a link were summed on chip, so calls on several streams
 * may run at once.  Per-queue counters are the caller's to keep: a batch comes from one queue, so the
 * batch's own sums are that queue's.
 * qgcm_route_stats copies one set of four out (peer QGCM_NO_PEER: the totals; a peer at or above max_keys:
 * QGCM_E_ARG).  It reports what completed accounting launches have added: synchronise the streams first. */
#define QGCM_TX 0
#define QGCM_RX 1
int qgcm_route_account(qgcm_ctx *ctx, int dir, uint32_t n, const uint32_t *d_peer, const qgcm_desc *d_descs,
                       const uint8_t *d_status, void *stream);
int qgcm_route_stats(qgcm_ctx *ctx, int dir, uint32_t peer, uint64_t out[4]);
/* Outgoing.pipeline / Incoming.pipeline for a batch in host memory (pinned or pageable), slot i at
 * i * stride: in chunks of at most 65536 packets, on one stream of the context: copy in, resolve, seal or
 * open (aad_len 4, the semantics of qgcm_seal_batch / qgcm_open_batch), account as Tx / Rx, copy back.
 * Synchronous; one call at a time per context (calls are serialized); the chunks are not pipelined.
 * seal: h_lens[i] in: the TUN packet length L; out: the datagram length 4 + L + 28, or 0 for a dropped
 * packet.  h_nonces as in qgcm_seal_host: n * 12 bytes, NULL (the nonce is in the slot) or
 * QGCM_NONCES_GENERATE.  open: h_lens[i] in: the datagram length; out: the plaintext packet length (what
 * qgcm_tun_write_slots takes), or 0.  Both: h_peer[i] = the peer or QGCM_NO_PEER; h_status[i] (may be NULL)
 * 1 or 0; returns the number of dropped packets or a negative error. */
int qgcm_route_seal_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                         const uint8_t *h_nonces, uint32_t *h_peer, uint8_t *h_status);
int qgcm_route_open_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                         uint32_t *h_peer, uint8_t *h_status);
/* ---- plugin chain on routed batches (main.go:41-51, plugin/compression.go, plugin/encryption.go) ---- */
/* The reference decides per packet and per peer which plugins run: compression.go:31-33 and
 * encryption.go:17-19 pass a packet through untouched when the peer's mapping.SupportedPlugins does not list
 * the plugin, and main.go:41-51 runs the node's configured plugins in order: compression then encryption
 * outgoing, the reverse incoming.  Here each key slot has one byte of plugin flags in device memory; the
 * effective plugins of a packet are F = plugins & flags[peer], `plugins` being the node's own --plugins mask
 * that every chain call takes.
 *
 * Every slot starts as QGCM_PLUGIN_ENCRYPTION, so a context that never calls qgcm_peer_plugins_set treats
 * its peers as qgcm_route_seal_host / qgcm_route_open_host do.  set / get move count flag bytes of slots
 * [first_idx, first_idx + count); a bit other than the two defined, or a range past max_keys: QGCM_E_ARG and
 * nothing changes.  Synchronous.  A call sequence reads a packet's flags once and carries them with the
 * packet in its work area: a qgcm_peer_plugins_set racing a batch changes each packet of it as a whole or
 * not at all. */
#define QGCM_PLUGIN_COMPRESSION 1u
#define QGCM_PLUGIN_ENCRYPTION  2u
int qgcm_peer_plugins_set(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t *flags);
int qgcm_peer_plugins_get(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, uint8_t *flags);
/* The chain of one batch, after qgcm_resolve_outgoing / qgcm_resolve_incoming on the same stream, with that
 * call's d_lens, d_peer and d_descs (the descriptors are rewritten).  d_status (n bytes) and d_bytes (n
 * uint32) receive each packet's verdict and the payload.Length that worker/outgoing.go:37-53 counts for it;
 * d_work is QGCM_CHAIN_WORK(n) bytes of caller memory, 16-B aligned.  Arguments are checked as in the resolve
 * calls (and plugins may hold only the two bits); n == 0 launches nothing; asynchronous on stream.  d_nonces
 * takes the three forms of qgcm_seal_batch; with QGCM_NONCES_GENERATE packet j of the call owns nonce j of
 * the reservation whether or not it ends up sealed.
 *
 * outgoing (d_lens[i] in: the TUN packet length L):
 *   d_peer[i] == QGCM_NO_PEER or >= max_keys   slot untouched              d_lens 0      status 0  bytes 0
 *   F has compression and the device codec     slot as resolve left it     d_lens 0      status 0  bytes 4 + L
 *     refuses the packet: L > QGCM_SNAPPY_DEVICE_MAX, or a compressed form longer than
 *     stride - 4 - (F has encryption ? 28 : 0) -- a divergence: snappy.Encode never fails
 *   compression applied                        Raw[4:] <- the bytes of qgcm_snappy_compress, L <- their length
 *   F has encryption, key slot unset           the (compressed) packet     d_lens 0      status 0  bytes 4 + L
 *   F has encryption, sealed                   ct | tag | nonce under key  d_lens 4+L+28 status 1  bytes 4+L+28
 *                                              `peer`, AAD Raw[0:4]
 *   F has no encryption                        the (compressed) packet     d_lens 4 + L  status 1  bytes 4 + L
 * d_lens out is the datagram length qgcm_udp_send_slots_to takes.
 *
 * incoming (d_lens[i] in: the datagram length m; encryption first, then compression):
 *   unresolved                                                             d_lens 0      status 0  bytes 0
 *   F has encryption and the open fails (tag, unset key, m - 4 < 28): the slot as qgcm_open_batch leaves it
 *                                                                          d_lens 0      status 0  bytes m
 *   F has compression and the decode fails (malformed, an empty result, longer than min(stride - 4,
 *     QGCM_SNAPPY_DEVICE_MAX)): the slot keeps the packet the codec was given
 *                                                                          d_lens 0      status 0  bytes 4 + the
 *                                              length entering the plugin (m - 4 - 28 if opened, else m - 4)
 *   delivered                                  the packet at Raw[4:]       d_lens = its length (what
 *                                              qgcm_tun_write_slots takes) status 1  bytes 4 + that length
 * d_status is authoritative: a delivered empty packet also has length 0. */
#define QGCM_CHAIN_WORK(n) (4 * (((uint64_t)(n) + 15) & ~(uint64_t)15))
int qgcm_chain_outgoing(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                        const uint32_t *d_peer, qgcm_desc *d_descs, uint32_t plugins, const uint8_t *d_nonces,
                        uint8_t *d_status, uint32_t *d_bytes, void *d_work, void *stream);
int qgcm_chain_incoming(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                        const uint32_t *d_peer, qgcm_desc *d_descs, uint32_t plugins,
                        uint8_t *d_status, uint32_t *d_bytes, void *d_work, void *stream);
/* qgcm_route_account with the byte counts of a chain call: the same counters, sums and on-chip combining.
 * Unresolved (d_peer[i] == QGCM_NO_PEER or >= max_keys): totals DroppedPackets += 1; status 1: totals and
 * link Packets += 1, Bytes += d_bytes[i]; any other status: DroppedPackets += 1, DroppedBytes += d_bytes[i].
 * d_status NULL: every resolved packet was delivered. */
int qgcm_route_account_bytes(qgcm_ctx *ctx, int dir, uint32_t n, const uint32_t *d_peer,
                             const uint32_t *d_bytes, const uint8_t *d_status, void *stream);
/* qgcm_route_seal_host / qgcm_route_open_host with the chain in place of the seal or open: the same chunks,
 * the same one stream, the same serialisation; accounted with qgcm_route_account_bytes.  h_lens out is as in
 * the tables above; returns the number of dropped packets or a negative error. */
int qgcm_route_chain_seal_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                               const uint8_t *h_nonces, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status);
int qgcm_route_chain_open_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                               uint32_t plugins, uint32_t *h_peer, uint8_t *h_status);
/* socket/udp.go:44-47 with mapping.Sockaddr per packet: datagram i (Raw[:lens[i]] of slot i) goes to
 * addrs[peer[i]], in sendmmsg batches.  Packets with peer[i] == QGCM_NO_PEER or lens[i] == 0 are skipped.
 * Returns the number sent, or -1 (also, before anything is sent, when some peer[i] >= n_addrs). */
typedef struct qgcm_peer_addr { uint32_t ip; uint16_t port; uint16_t pad; } qgcm_peer_addr; /* network byte order */
int qgcm_udp_send_slots_to(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                           const uint32_t *peer, const qgcm_peer_addr *addrs, uint32_t n_addrs);

/* ---- send plan on routed batches: per-peer segmented UDP sends ---- */
/* With the UDP_SEGMENT control message one sendmsg carries many datagrams of one length to one destination.
 * A routed batch interleaves its peers, so the batch is grouped first: on the GPU, from the d_peer and d_lens
 * arrays that qgcm_chain_outgoing (or a resolve and qgcm_seal_batch) leave there.
 *
 * Packet i is sendable when d_peer[i] < max_keys of the context and d_lens[i] != 0: the skip rule of
 * qgcm_udp_send_slots_to, and the accounting's rule for a peer at or above max_keys.  The plan of a batch:
 *   order[0..m)   the sendable indices, sorted by peer ascending and by index ascending within a peer: arena
 *                 order per link, so no flow is reordered
 *   runs          the maximal stretches of order whose packets have one peer and one length L
 *   cap(L)        1 when L > max_seg_len, else max(1, min(max_segs, max_bytes / L)) (integer division)
 *   trains[0..t)  every run of r packets cut from its front into trains of cap(L) packets, the last holding
 *                 the remainder: {first (an index into order), count, peer, seg_len (the common length)}.
 *                 Trains follow order's order and tile [0, m) exactly
 *   counts        {m, t}
 * A shorter last segment, which the kernel interface would take, is not used.  Entries of order past m and of
 * trains past t are unspecified.
 *
 * limits (NULL: all defaults): a zero field takes its default -- max_segs 64 (UDP_MAX_SEGMENTS of the oldest
 * kernels with UDP_SEGMENT), max_seg_len 65507, max_bytes 65507; max_segs above 1024 (UIO_MAXIOV) or
 * max_bytes above 65507: QGCM_E_ARG.  max_seg_len is the caller's path-MTU guard: a datagram longer than path
 * MTU - 28 cannot be a segment (the kernel refuses the message), so it is planned as a train of one and goes
 * out, fragmented, as it does today.
 *
 * qgcm_send_plan: device arrays, asynchronous on stream; d_order n uint32, d_trains n entries (16-B aligned),
 * d_counts 2 uint32, d_work qgcm_send_plan_work(n) bytes of device memory, 256-B aligned, the call's own
 * until it has run.  It keeps no state in the context beyond max_keys and needs no route table, so calls on
 * several streams may run at once.  n == 0: QGCM_OK, nothing launched; n above QGCM_MAX_BATCH, a NULL or
 * misaligned array, bad limits: QGCM_E_ARG, nothing launched.
 * qgcm_send_plan_cpu: the same plan by the host (a counting sort per 8-bit digit of the peer, one pass for the
 * trains), with max_keys in place of a context; allocates nothing (it borrows trains' storage while it
 * sorts).  counts is written for n == 0 too.
 * qgcm_send_plan_host: host arrays in and out, synchronous, serialised with the context's other routed host
 * calls: copies lens and peer up (8 B a packet), plans on the context's routed stream in a work area the
 * context owns and grows on demand, and copies counts, order[0..m) and trains[0..t) back.  Batches of fewer
 * than QGCM_PLAN_DEVICE_MIN packets (environment, read at qgcm_create; 0: always the device, 4294967295:
 * never; default 65536, the measured crossover of DESIGN.md 4.5) are planned by qgcm_send_plan_cpu's code
 * instead; both paths write the same bytes. */
typedef struct qgcm_train { uint32_t first, count, peer, seg_len; } qgcm_train;
typedef struct qgcm_plan_limits { uint32_t max_segs, max_seg_len, max_bytes; } qgcm_plan_limits;
uint64_t qgcm_send_plan_work(uint32_t n);
int qgcm_send_plan(qgcm_ctx *ctx, uint32_t n, const uint32_t *d_lens, const uint32_t *d_peer,
                   const qgcm_plan_limits *limits, uint32_t *d_order, qgcm_train *d_trains, uint32_t *d_counts,
                   void *d_work, void *stream);
int qgcm_send_plan_cpu(uint32_t n, const uint32_t *lens, const uint32_t *peer, uint32_t max_keys,
                       const qgcm_plan_limits *limits, uint32_t *order, qgcm_train *trains, uint32_t counts[2]);
int qgcm_send_plan_host(qgcm_ctx *ctx, uint32_t n, const uint32_t *h_lens, const uint32_t *h_peer,
                        const qgcm_plan_limits *limits, uint32_t *h_order, qgcm_train *h_trains, uint32_t counts[2]);
/* Sends a planned batch: one message per train, `count` iovecs (one per slot, nothing is copied), msg_name
 * addrs[peer], and for count > 1 a UDP_SEGMENT control message of seg_len; in sendmmsg batches of at most
 * 1024 messages over a bounded iovec pool.  lens are the batch's n datagram lengths, order / m and trains /
 * n_trains the plan.  The whole plan is checked before anything is sent; any violation returns -1 with
 * nothing sent: an order[j] >= n; a train with first + count > m, count outside [1, 1024] or peer >= n_addrs;
 * a seg_len of 0, or above 65535 in a train of more than one (the segment size travels as 16 bits); a member
 * whose lens differs from the train's seg_len or exceeds stride (a plan that does not match the lengths
 * would move datagram boundaries).
 * A segmented message that fails with EINVAL, EIO, EMSGSIZE, ENOPROTOOPT or EOPNOTSUPP (a kernel without
 * UDP_SEGMENT, more segments than it takes, a segment above the path MTU) is sent again as `count` single
 * datagrams and the call goes on; after ENOPROTOOPT or EOPNOTSUPP the rest of the call goes unsegmented
 * without asking again (on such a host set QGCM_UDP_GSO=0 and save that one refusal per call).  A plain message that fails ends the call as qgcm_udp_send_slots_to ends:
 * the number sent so far, or -1 if none; EINTR is retried.  QGCM_UDP_GSO=0 (environment, read at each call)
 * sends every train unsegmented, in plan order.  Returns the number of datagrams sent.  stats (may be NULL):
 * {messages sent, of them segmented, trains that fell back}. */
int qgcm_udp_send_plan(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                       const uint32_t *order, uint32_t m, const qgcm_train *trains, uint32_t n_trains,
                       const qgcm_peer_addr *addrs, uint32_t n_addrs, uint64_t stats[3]);

/* ---- coalesced receive on routed batches: UDP_GRO buffers unpacked into slots ---- */
/* With the UDP_GRO socket option one recvmsg returns a whole train of equal-length datagrams of one sender --
 * what qgcm_udp_send_plan puts on the wire -- as one buffer, with the segment size in a control message.  The
 * buffers are received back to back into a packed byte area, cross to the device at their own size, and a
 * kernel scatters their datagrams into the slots that resolve, chain and accounting take.
 *
 * qgcm_gro_buf describes one received buffer inside the packed area: off its byte offset (any alignment), len
 * the bytes received (0 .. 65535), seg_len the value of the UDP_GRO control message or 0 when there was none,
 * first the slot of its first datagram.  The buffer holds `count` datagrams: 1 when seg_len == 0 or seg_len >=
 * len (a lone datagram, one of length 0 included), else ceil(len / seg_len).  Datagram k is packed[off +
 * k * seg_len ..) of length L = min(seg_len, len - k * seg_len) (len when count is 1) and belongs to slot
 * first + k.  The unpack sets d_lens[first + k] = L and bytes [0, min(L, stride)) of that slot to the
 * datagram's; every other byte of the arena and every other length stays as it was (slot tails, slots no
 * buffer names).  A datagram longer than stride keeps its true length, which qgcm_resolve_incoming treats as
 * a miss.  A buffer with off + len > packed_len or first + count > n is skipped whole: nothing is written for
 * it.
 *
 * qgcm_udp_gro sets the socket option (on: 1 / 0); returns 0 or -errno.
 * qgcm_udp_recv_gro waits up to timeout_ms (-1: forever) for the first datagram as qgcm_udp_recv_slots does,
 * then takes what is queued with MSG_DONTWAIT, each recvmsg straight into the packed area at the fill position
 * rounded up to 16 B (every off is a multiple of 16), and writes one entry per buffer, `first` included.  It
 * stops before a receive when fewer than 65536 bytes of room are left (a coalesced buffer is never
 * truncated), when max_bufs entries are written, or when fewer than QGCM_GRO_SEGS slots of max_n are left
 * (the kernel's cap per buffer); what it did not take stays queued for the next call.  Returns the number of
 * datagrams n (the slots the table names), 0 on timeout, or -1 (also for a NULL array, and for a packed_cap,
 * max_bufs or max_n that allows no receive at all).  out (may be NULL): {buffers, bytes of the packed area
 * used = the end of the last buffer, datagrams cut}.  A buffer with more datagrams than slots are left is cut
 * to the ones that fit and the rest are counted in out[2]; no current kernel produces one.  Works with the
 * option off and on a host that does not coalesce: every buffer is then one datagram.
 *
 * qgcm_gro_unpack: device arrays, asynchronous on stream, no context state (calls on several streams may run
 * at once).  d_packed 16-B aligned and its allocation rounded up to 16 B: the kernel may read up to the 16-B
 * boundary behind packed_len, never further.  d_bufs 16-B aligned, d_lens 4-B aligned; stride a nonzero
 * multiple of 4 and d_arena 4-B aligned (a stride that is a multiple of 16 under a 16-B-aligned arena takes
 * the 16-byte path).  The `first` values ascend, as qgcm_udp_recv_gro writes them (each slot finds its buffer
 * by a binary search over them); a table in which they do not is memory-safe, and which of its slots are
 * written is unspecified.  n == 0 or n_bufs == 0: QGCM_OK, nothing launched.  n > QGCM_MAX_BATCH, n_bufs > n,
 * a bad stride, a NULL or misaligned pointer: QGCM_E_ARG.
 * qgcm_gro_resolve: qgcm_gro_unpack and qgcm_resolve_incoming of the same arrays in one launch: device arrays,
 * asynchronous on stream, no context state beyond the route table (calls on several streams may run at once).
 * It leaves in the arena, d_lens, d_peer and d_descs exactly what
 *   qgcm_gro_unpack(ctx, d_packed, packed_len, d_bufs, n_bufs, n, d_arena, stride, d_lens, stream) and then
 *   qgcm_resolve_incoming(ctx, d_arena, stride, n, d_lens, d_peer, d_descs, stream)
 * leave, byte for byte.  Datagram k of a buffer that is not skipped (slot i = first + k, length L): d_lens[i] = L,
 * bytes [0, min(L, stride)) of the slot are the datagram's and the slot's tail keeps its bytes; the packet is
 * readable when 4 <= L <= stride, its peer then the route of key = in-net(addr) ? addr : gateway with addr the
 * datagram's first four bytes -- read from the packed area, not from the slot -- and else QGCM_NO_PEER;
 * d_descs[i] = {i * stride, L >= 4 ? L - 4 : 0, peer}, d_peer[i] = peer.  A slot i < n that no unskipped buffer
 * names (a gap in `first`, a buffer past packed_len or past n) keeps d_lens[i] and its bytes, and its peer and
 * descriptor are resolved from that length and from Raw[0:4] as they were: d_lens is input and output, as it is
 * for the pair.  n_bufs == 0 with n > 0 is qgcm_resolve_incoming.  n == 0: QGCM_OK, nothing launched.  A table
 * whose `first` values do not ascend is memory-safe as for qgcm_gro_unpack (every table index is checked
 * against n_bufs, every source byte against packed_len, every slot against n); which slots are written, and
 * with what, is then unspecified.  QGCM_E_ARG with nothing launched: a NULL ctx, n > QGCM_MAX_BATCH, n_bufs > n,
 * a stride that is zero or not a multiple of 4, any NULL array when n > 0, d_packed, d_bufs or d_descs off a
 * 16-B boundary, d_arena, d_lens or d_peer off a 4-B boundary, a context without qgcm_routes_set.  The read
 * bound is qgcm_gro_unpack's: up to the 16-B boundary behind packed_len, never further.
 * qgcm_gro_unpack_cpu: the same for host arrays (no alignment asked), by the host, so that a worker can use
 * the coalesced receive with qgcm_route_open_host.  It checks the table first: each `first` is the exclusive
 * prefix sum of the counts before it and the counts total n; if not, QGCM_E_ARG and nothing is written.
 *
 * qgcm_route_open_gro_host / qgcm_route_chain_open_gro_host: qgcm_route_open_host /
 * qgcm_route_chain_open_host with the copy-in replaced.  The table is checked as in qgcm_gro_unpack_cpu
 * (QGCM_E_ARG, nothing launched).  The batch is cut into chunks at buffer boundaries under the packet and
 * byte limits of those calls (a buffer with more datagrams than a chunk holds is a chunk of its own); per
 * chunk only the chunk's packed bytes and table entries are copied up, unpacked into the context's device
 * arena and resolved (qgcm_gro_unpack, then the resolve; the one launch of qgcm_gro_resolve when
 * QGCM_GRO_FUSED=1 was in the environment at qgcm_create -- the outputs are the same), then opened or chained,
 * accounted and copied back as in those calls, serialised on the context's routed stream like them.  h_lens is output only.  h_peer, h_status, h_lens, the return value
 * and the Rx counters are what the existing call gives for the arena and lengths that qgcm_gro_unpack_cpu
 * makes of the same input (a buffer past packed_len counts as datagrams of length 0); delivered packets are
 * equal over Raw[:4 + h_lens[i]], dropped ones over Raw[:datagram length].  The slot bytes behind that are
 * unspecified: they come from the context's device arena, not from h_arena. */
#define QGCM_GRO_SEGS 64u
typedef struct qgcm_gro_buf { uint32_t off, len, seg_len, first; } qgcm_gro_buf;
int qgcm_udp_gro(int fd, int on);
int qgcm_udp_recv_gro(int fd, uint8_t *packed, uint64_t packed_cap, qgcm_gro_buf *bufs, uint32_t max_bufs,
                      uint32_t max_n, int timeout_ms, uint64_t out[3]);
int qgcm_gro_unpack(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gro_buf *d_bufs,
                    uint32_t n_bufs, uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, void *stream);
int qgcm_gro_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gro_buf *d_bufs,
                     uint32_t n_bufs, uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens,
                     uint32_t *d_peer, qgcm_desc *d_descs, void *stream);
int qgcm_gro_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_gro_buf *bufs, uint32_t n_bufs,
                        uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens);
int qgcm_route_open_gro_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_gro_buf *bufs,
                             uint32_t n_bufs, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                             uint32_t *h_peer, uint8_t *h_status);
int qgcm_route_chain_open_gro_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                   const qgcm_gro_buf *bufs, uint32_t n_bufs, uint8_t *h_arena, uint64_t stride,
                                   uint32_t n, uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status);

/* ---- delivered packets packed on routed batches: the copy back and the TUN write ---- */
/* After the incoming chain the delivered packets lie scattered over slots of `stride` bytes, between the
 * dropped ones and in front of slot tails nobody reads.  The pack lays them back to back -- the mirror of
 * qgcm_gro_unpack -- so that the copy back and the TUN write move delivered bytes only.
 *
 * Packet i of a batch is delivered when d_status[i] == 1 and 4 + d_lens[i] <= stride (d_status == NULL: every
 * packet has status 1).  A status-1 packet with an impossible length is left out, not clamped, so a bad length
 * array cannot move the kernel past a slot.  The delivered packets are taken in arena order (index ascending:
 * no flow is reordered) and numbered k = 0 .. m-1.  Record k is Raw[0 : 4 + L] of its slot -- the 4-byte header
 * that payload.IPAddress aliases, then the packet, L = d_lens[i] -- padded with zero bytes to
 * R = (4 + L + 15) & ~15 and placed at off_k, the sum of R over the records before it: every off is a multiple
 * of 16, as in the receive side's table.  recs[k] = {off_k, L, i, d_peer[i]}; counts = {m, bytes}, bytes the sum
 * of all R: the full need, even when it does not fit.  A record with off_k + R > packed_cap is not copied and
 * its entry gets off = 0xffffffff; these records form a suffix, because offsets ascend.  Every byte of
 * [0, min(bytes, the end of the last record that fits)) of the packed area is determined, zero padding
 * included; every byte behind it is untouched; recs entries past m are unspecified.  A delivered empty packet
 * (L == 0) is a 16-byte record.
 *
 * qgcm_deliver_pack: device arrays, asynchronous on stream, no context state (calls on several streams may run
 * at once).  stride a nonzero multiple of 4 and d_arena 4-B aligned (a stride that is a multiple of 16 under a
 * 16-B-aligned arena takes the 16-byte path, anything else the dword path); d_lens and d_peer 4-B aligned,
 * d_status any alignment or NULL; d_packed and d_recs (n entries) 16-B aligned, d_counts (two uint64) 8-B
 * aligned; d_work qgcm_deliver_pack_work(n) bytes of device memory, 16-B aligned, the call's own until it has
 * run.  Nothing at or past slot * stride + stride is read, nothing at or past packed_cap is written.  n == 0:
 * counts = {0, 0}, nothing else launched.  n > QGCM_MAX_BATCH, a bad stride, packed_cap above 2^32 - 16 (off is
 * 32 bits), a NULL or misaligned pointer: QGCM_E_ARG, nothing launched.
 * qgcm_deliver_pack_cpu: the same contract for host arrays (no alignment asked), by the host, so that a worker
 * on qgcm_route_chain_open_host can pack for qgcm_tun_write_packed.
 *
 * qgcm_tun_write_packed: qgcm_tun_write_slots for a packed batch: writes packed[off + 4 .. off + 4 + len) of
 * records 0 .. m-1 in order; a packet the kernel rejects ends the batch there and EINTR is retried, as in
 * qgcm_tun_write_slots.  The whole table is checked first: every off + 4 + len <= packed_len, otherwise -1 with
 * nothing written (a record that did not fit, off = 0xffffffff, fails that check).  Returns the number written
 * (m on success) or -1 when none was.
 *
 * qgcm_route_chain_open_packed_host / qgcm_route_chain_open_gro_packed_host: qgcm_route_chain_open_host /
 * qgcm_route_chain_open_gro_host with the copy back replaced.  Chunks, serialisation and the order of resolve,
 * chain and accounting are theirs.  Per chunk the delivered packets are packed into an area the context owns
 * (cn * round16(stride) bytes, grown on demand: the device pack always fits) and the chunk's counts come down.
 * If its bytes do not fit behind the fill position of h_out, the call returns QGCM_E_NOMEM before that chunk is
 * accounted or copied: the caller's input is whole and the call can be repeated from packet out[0] on (the GRO
 * form: from that packet's buffer, which is a chunk's first, with a table rebased so that it is again a prefix
 * sum from 0).  Otherwise the chunk is accounted and its bytes and records are appended to h_out (16-B steps)
 * and h_recs (n entries), `off` rebased by the fill position and `slot` by the chunk's first slot: the table is
 * the one qgcm_deliver_pack_cpu makes of the whole batch.  h_peer, h_status and h_lens come back for all n
 * packets as from the existing calls; the slots-in form reads h_arena and never writes it.  out = {packets
 * fully processed, records written, bytes of h_out used}, written on success and on QGCM_E_NOMEM.  out_cap
 * above 2^32 - 16 counts as 2^32 - 16.  Returns the number of drops or a negative error.  Only the chain forms
 * have a packed variant: the plain open's lengths are datagram lengths, and a chain with
 * QGCM_PLUGIN_ENCRYPTION alone is that call. */
typedef struct qgcm_pack_rec { uint32_t off, len, slot, peer; } qgcm_pack_rec;
uint64_t qgcm_deliver_pack_work(uint32_t n);
int qgcm_deliver_pack(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                      const uint32_t *d_peer, const uint8_t *d_status, uint8_t *d_packed, uint64_t packed_cap,
                      qgcm_pack_rec *d_recs, uint64_t *d_counts, void *d_work, void *stream);
int qgcm_deliver_pack_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                          const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_pack_rec *recs,
                          uint64_t counts[2]);
int qgcm_tun_write_packed(int fd, const uint8_t *packed, uint64_t packed_len, const qgcm_pack_rec *recs, uint32_t m);
int qgcm_route_chain_open_packed_host(qgcm_ctx *ctx, const uint8_t *h_arena, uint64_t stride, uint32_t n,
                                      uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                      uint8_t *h_out, uint64_t out_cap, qgcm_pack_rec *h_recs, uint64_t out[3]);
int qgcm_route_chain_open_gro_packed_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                          const qgcm_gro_buf *bufs, uint32_t n_bufs, uint64_t stride, uint32_t n,
                                          uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                          uint8_t *h_out, uint64_t out_cap, qgcm_pack_rec *h_recs, uint64_t out[3]);

/* ---- planned trains packed on routed batches: one iovec a train, own-size copy back ---- */
/* After the outgoing chain the sealed datagrams lie in slots of `stride` bytes and the plan of qgcm_send_plan
 * names them train by train.  The pack lays every train's datagrams back to back -- the mirror of
 * qgcm_gro_unpack: aligned slots to unaligned destinations -- so that the copy back moves datagram bytes only
 * and the sender hands the kernel one iovec a train.  A qgcm_ptrain is a qgcm_train with `first` replaced by
 * the byte offset `off` of the train in the packed area.
 *
 * Inputs: an arena of n slots of `stride` bytes and a plan as qgcm_send_plan leaves it: order[0..m),
 * trains[0..t), counts = {m, t}.  Train j holds its `count` datagrams with no gaps: datagram k is
 * Raw[0 : seg_len] of slot order[first + k] and sits at off_j + k * seg_len; the train is padded with zero bytes
 * to R_j = (count * seg_len + 15) & ~15, and off_j is the sum of R over the trains before it, so every off is a
 * multiple of 16.  ptrains[j] = {off_j, count, peer, seg_len}; pcounts = {t, bytes}, bytes the sum of all R: the
 * full need, even when it does not fit.  A train with off_j + R_j > packed_cap is not copied and its entry gets
 * off = 0xffffffff; these trains form a suffix, because offsets ascend.  Every byte of [0, the end of the last
 * train that fits) of the packed area is determined, zero padding included; every byte behind it is untouched;
 * ptrains entries past t are unspecified.  The pack does not read the batch's lengths: the plan's seg_len is the
 * length, and the plan guarantees the two are equal.
 *
 * A plan is well-formed when m <= n and t <= m, the trains tile [0, m) in order (each `first` the sum of the
 * counts before it, the counts total m), every count is in [1, 1024], every seg_len in [1, stride] and every
 * order[p] < n.  qgcm_train_pack reads the plan from device memory and cannot refuse it, so it stays memory-safe
 * on any plan: m and t as read from d_plan_counts are clamped to n; a train with a count or seg_len out of
 * range, or with first + count > m (in 64 bits), is void: its size is 0 and its off 0xffffffff; a member with
 * order[p] >= n is packed as seg_len zero bytes, no slot is read for it.  For a plan that does not tile the
 * packed bytes are unspecified.  In every case nothing outside the arena's n * stride bytes is read (and of a
 * slot nothing at or past min(round16(seg_len), stride)), and nothing at or past packed_cap is written.
 *
 * qgcm_train_pack: device arrays, asynchronous on stream, no context state (calls on several streams may run
 * at once).  It reads m and t on the device, so it follows qgcm_send_plan on the same stream with no host
 * synchronisation in between.  stride a nonzero multiple of 4 and d_arena 4-B aligned (a stride that is a
 * multiple of 16 under a 16-B-aligned arena takes the 16-byte path, anything else the dword path); d_order and
 * d_plan_counts (two uint32) 4-B aligned; d_trains, d_packed and d_ptrains (n entries) 16-B aligned; d_pcounts
 * (two uint64) 8-B aligned; d_work qgcm_train_pack_work(n) bytes of device memory, 16-B aligned, the call's own
 * until it has run.  n == 0: pcounts = {0, 0}, nothing else launched.  n > QGCM_MAX_BATCH, a bad stride,
 * packed_cap above 2^32 - 16 (off is 32 bits), a NULL or misaligned pointer: QGCM_E_ARG, nothing launched.
 * qgcm_train_pack_cpu: the same contract for host arrays (no alignment asked), by the host, with m and t by
 * value.  It checks the whole plan first: a plan that is not well-formed returns QGCM_E_ARG with nothing
 * written.
 *
 * qgcm_udp_send_packed: qgcm_udp_send_plan for a packed batch: one message per train with ONE iovec,
 * packed[off .. off + count * seg_len), msg_name addrs[peer], and for count > 1 a UDP_SEGMENT control message of
 * seg_len; in sendmmsg batches of at most 1024 messages.  The whole table is checked before anything is sent;
 * any violation returns -1 with nothing sent: off + count * seg_len > packed_len (so a train that did not fit,
 * off = 0xffffffff, fails), count outside [1, 1024], peer >= n_addrs, a seg_len of 0, or above 65535 in a train of
 * more than one.  The fallback to single datagrams (cut from the packed bytes), the sticky ENOPROTOOPT /
 * EOPNOTSUPP rule, QGCM_UDP_GSO=0, stats and the return value are those of qgcm_udp_send_plan.
 *
 * qgcm_route_chain_seal_packed_host: qgcm_route_chain_seal_host with the copy back replaced.  Chunks,
 * serialisation and the order of resolve, chain and Tx accounting are that call's.  Per chunk the chunk's d_lens
 * and d_peer are planned on the device under `limits` (as qgcm_send_plan; always the device planner: the arrays
 * are already there) and its trains are packed into an area the context owns (cn * round16(stride) bytes, grown
 * on demand: the device pack always fits); then the counts come down.  If the chunk's bytes do not fit behind
 * the fill position of h_out, the call returns QGCM_E_NOMEM before that chunk is accounted or copied: the
 * caller's input is whole and the call can be repeated from packet out[0] on.  Otherwise the chunk is accounted
 * and appended: its bytes to h_out (16-B steps), its table to h_ptrains (n entries; `off` rebased by the fill
 * position) and, if h_order is not NULL, its order[0..m) to h_order (n entries; rebased by the chunk's first
 * slot), so that h_order names the slot of every packed datagram in table order.  Trains never span a chunk:
 * for a batch of one chunk (n <= 65536 and n * stride <= 256 MiB) the table is exactly qgcm_send_plan_cpu +
 * qgcm_train_pack_cpu of qgcm_route_chain_seal_host's output.  h_arena is read and never written.  h_peer,
 * h_status, h_lens and the return value are those of qgcm_route_chain_seal_host.  out = {packets fully
 * processed, trains written, bytes of h_out used, datagrams in those trains}, written on success and on
 * QGCM_E_NOMEM.  out_cap above 2^32 - 16 counts as 2^32 - 16. */
typedef struct qgcm_ptrain { uint32_t off, count, peer, seg_len; } qgcm_ptrain;
uint64_t qgcm_train_pack_work(uint32_t n);
int qgcm_train_pack(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_order,
                    const qgcm_train *d_trains, const uint32_t *d_plan_counts, uint8_t *d_packed, uint64_t packed_cap,
                    qgcm_ptrain *d_ptrains, uint64_t *d_pcounts, void *d_work, void *stream);
int qgcm_train_pack_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *order, uint32_t m,
                        const qgcm_train *trains, uint32_t t, uint8_t *packed, uint64_t packed_cap,
                        qgcm_ptrain *ptrains, uint64_t pcounts[2]);
int qgcm_udp_send_packed(int fd, const uint8_t *packed, uint64_t packed_len, const qgcm_ptrain *ptrains,
                         uint32_t n_trains, const qgcm_peer_addr *addrs, uint32_t n_addrs, uint64_t stats[3]);
int qgcm_route_chain_seal_packed_host(qgcm_ctx *ctx, const uint8_t *h_arena, uint64_t stride, uint32_t n,
                                      uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins,
                                      const qgcm_plan_limits *limits, uint32_t *h_peer, uint8_t *h_status,
                                      uint8_t *h_out, uint64_t out_cap, qgcm_ptrain *h_ptrains, uint32_t *h_order,
                                      uint64_t out[4]);

/* ---- outgoing frames packed on routed batches: the TUN read and the copy up at their own size ---- */
/* qgcm_tun_read_slots reads every TUN packet into a slot of `stride` bytes and the outgoing pipelines copy whole
 * slots up.  Here the read lays the packets back to back, a table names them, and one launch on the device puts
 * them into slots and resolves them -- the mirror of the packed copy back, so that the outgoing pipeline crosses
 * PCIe at its own size in both directions.
 *
 * Frame table: frame i is packed[off_i, off_i + len_i) and belongs to slot i.  A frame is valid when off is a
 * multiple of 16 and off + len <= packed_len (computed in 64 bits); any other frame is void.
 *
 * qgcm_frames_resolve: device arrays, asynchronous on stream, one launch.  For a valid frame it leaves exactly
 * what an unpack followed by qgcm_resolve_outgoing leaves: Raw[4 : 4 + min(len, stride - 4)) of slot i takes the
 * frame's bytes; d_lens[i] = len (the true length, also when the bytes were clamped); own_ip into Raw[0:4] on a
 * hit, while on a miss the four bytes keep their value; d_peer[i] and d_descs[i] as qgcm_resolve_outgoing
 * documents them, its divergences included (len < 20 and 4 + len + 28 > stride are misses).  Every other byte of
 * the arena keeps its value: the slot's tail, and what lies behind a short frame.  For a void frame d_lens[i] = 0,
 * d_peer[i] = QGCM_NO_PEER, d_descs[i] = {i * stride, 0, QGCM_NO_PEER} and the slot is untouched.  The call is
 * memory-safe on any table: it reads nothing behind the 16-byte boundary after packed_len and nothing outside
 * the arena's n * stride bytes.  d_packed and d_descs 16-B aligned, the d_packed allocation rounded up to 16 B;
 * d_frames 8-B aligned; d_lens, d_peer and d_arena 4-B aligned; stride a nonzero multiple of 4 and at least 8 (a
 * stride that is a multiple of 16 under a 16-B-aligned arena takes the 16-byte path, anything else the dword
 * path).  n == 0: QGCM_OK, nothing launched.  n > QGCM_MAX_BATCH, a bad stride, a NULL or misaligned pointer, or
 * a call before qgcm_routes_set: QGCM_E_ARG, nothing launched.  The route table is taken under the context's
 * route lock as qgcm_resolve_outgoing takes it.
 *
 * qgcm_frames_unpack_cpu: the unpack half for host arrays (no alignment asked; stride as above), for workers
 * without the device path, and the yardstick of the pipeline below.  It checks the table first: a frame that is
 * not valid returns QGCM_E_ARG with nothing written.  Otherwise lens[i] = len and Raw[4 : 4 + min(len,
 * stride - 4)) of slot i for every frame, nothing else.
 *
 * qgcm_tun_read_packed: qgcm_tun_read_slots for a packed area.  It waits up to timeout_ms for the first packet,
 * then drains what the queue holds with one preadv2(RWF_NOWAIT) per packet straight into `packed` at the fill
 * position rounded up to 16, and writes one qgcm_frame per packet.  It stops before a read when fewer than 65536
 * bytes of room are left -- no frame is ever truncated -- and at max_n.  Where RWF_NOWAIT is refused, or with
 * QGCM_TUN_URING=-1, it polls and reads as qgcm_tun_read_slots does; with QGCM_TUN_URING=1 it still uses preadv2:
 * a ring submission names every destination before a length is known, so it cannot lay frames back to back.
 * Returns the count, 0 on timeout, or -1 (also for a NULL array or a packed_cap below 65536).  out (may be NULL)
 * = {frames, bytes used = the end of the last frame}.
 *
 * qgcm_route_chain_seal_frames_host: qgcm_route_chain_seal_packed_host with the copy-in replaced.  The whole
 * table is checked first: every frame valid and the offsets ascending without overlap (off_i + len_i <=
 * off_{i+1}), else QGCM_E_ARG with nothing launched.  h_nonces n * 12 bytes or QGCM_NONCES_GENERATE; NULL is
 * QGCM_E_ARG (no host slot exists to carry a nonce).  Chunks are that call's (at most 65536 packets and 256 MiB
 * of slots) and fall at frame boundaries.  Per chunk only the packed bytes its frames span (from the first
 * frame's off, a 16-B boundary, to the last frame's end) and their table entries (rebased to the span) go up;
 * qgcm_frames_resolve puts them into the context's device arena; the chain, the plan, the train pack, the Tx
 * accounting and the copy back follow as in that call, on the same stream and under the same pipeline lock.
 * h_lens is output only.  h_peer, h_status, h_lens, h_out, h_ptrains, h_order, out, the return value and the Tx
 * counters are what qgcm_route_chain_seal_packed_host gives for the arena and lengths qgcm_frames_unpack_cpu makes
 * of the same input.  QGCM_E_NOMEM as in that call (out written); the call is then repeated with
 * frames + out[0] and n - out[0] over the same packed area -- offsets are absolute, nothing is rebased. */
typedef struct qgcm_frame { uint32_t off, len; } qgcm_frame;
int qgcm_tun_read_packed(int fd, uint8_t *packed, uint64_t packed_cap, qgcm_frame *frames,
                         uint32_t max_n, int timeout_ms, uint64_t out[2]);
int qgcm_frames_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len,
                        const qgcm_frame *d_frames, uint32_t n, uint8_t *d_arena, uint64_t stride,
                        uint32_t *d_lens, uint32_t *d_peer, qgcm_desc *d_descs, void *stream);
int qgcm_frames_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_frame *frames,
                           uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens);
int qgcm_route_chain_seal_frames_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                      const qgcm_frame *frames, uint64_t stride, uint32_t n,
                                      uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins,
                                      const qgcm_plan_limits *limits, uint32_t *h_peer, uint8_t *h_status,
                                      uint8_t *h_out, uint64_t out_cap, qgcm_ptrain *h_ptrains,
                                      uint32_t *h_order, uint64_t out[4]);

/* ---- TUN super-frames segmented on routed batches: TSO / USO for the outgoing path ---- */
/* A TUN queue opened with IFF_VNET_HDR and TUNSETOFFLOAD hands over one TCP (or UDP_L4) super-frame of up to 64 KiB
 * with a 10-byte virtio_net_hdr in front, and leaves the segmentation and the L4 checksum to the reader.  Here
 * the read lays the super-frames back to back, a table names them, and one launch on the device cuts them into
 * the per-packet slots, lengths, peers and descriptors the chain, the plan and the train pack take: the frame
 * crosses PCIe once, its headers not repeated.
 *
 * Table: entry e is the IP packet packed[off, off + len) (behind its vnet header) and names the slots
 * [first, first + count).  One rule, from the entry alone (never from packet bytes), says whether it is valid:
 *   every kind:  off % 16 == 0, off + len <= packed_len (64 bits), first + count <= n, kind <= 3;
 *   PLAIN, CSUM: count == 1;
 *   CSUM:        l4_off and csum_off even, l4_off + csum_off + 2 <= len;
 *   TCP4, UDP4:  l4_off in [20, 60] and a multiple of 4; UDP4: hdr_len == l4_off + 8; TCP4: hdr_len - l4_off in
 *                [20, 60] and a multiple of 4; hdr_len < len; gso_size >= 1;
 *                count == ceil((len - hdr_len) / gso_size) and count <= QGCM_GSO_SEGS.
 * Any other entry is void (`reserved` is not looked at).  A void entry with count >= 1 and first < n gives slot
 * `first` the void-frame result of qgcm_frames_resolve -- d_lens = 0, QGCM_NO_PEER, descriptor {first * stride, 0,
 * QGCM_NO_PEER}, the slot untouched -- and writes nothing for the further slots it names.
 *
 * Segment k of a valid TCP4 / UDP4 entry goes to slot first + k: the packet at Raw[4:] of length L_k = hdr_len +
 * P_k, P_k = min(gso_size, len - hdr_len - k * gso_size).  Its header is the frame's first hdr_len bytes, its
 * payload packed[off + hdr_len + k * gso_size ..).  IPv4: total length L_k (mod 2^16), identification id0 + k mod
 * 2^16, header checksum recomputed over l4_off bytes.  TCP4: sequence number seq0 + k * gso_size mod 2^32, FIN and
 * PSH cleared on every segment but the last, checksum from scratch over pseudo-header (protocol 6), header and
 * payload, an odd payload padded with a zero byte; what the frame had in the field is ignored.  UDP4: UDP length
 * 8 + P_k (mod 2^16), checksum from scratch (protocol 17), a result of 0 stored as 0xffff.  CSUM: the packet is
 * copied and the 16-bit field at l4_off + csum_off becomes ~fold(sum of bytes [l4_off, len)), the partial value
 * already in the field included (virtio's NEEDS_CSUM), 0 stored as 0xffff.  PLAIN: what qgcm_frames_resolve does
 * for a frame.  For every slot written, as qgcm_frames_resolve documents: d_lens[i] is the true length, also when
 * clamped; only Raw[4 : 4 + min(L, stride - 4)) is written (checksums are those of the whole packet); the
 * destination is Packet[16:20], L < 20 or 4 + L + 28 > stride is a miss; own_ip into Raw[0:4] on a hit only; slot
 * tails, Raw[0:4] of misses and slots no entry names keep their bytes, and a slot i < n no entry names keeps its
 * d_lens, d_peer and d_descs too.
 *
 * `first` ascends: the host calls (qgcm_gso_unpack_cpu, qgcm_route_chain_seal_gso_host) check that every entry is
 * valid, that each `first` is the sum of the counts before it and that the counts total n; else QGCM_E_ARG with
 * nothing written.  qgcm_gso_resolve is memory-safe on any table: it reads the table below n_frames only, nothing
 * behind the 16-byte boundary after packed_len and nothing of the packed area outside [off, off + len) of a valid
 * entry rounded out to 16-byte boundaries, and it writes nothing outside the arena's n * stride bytes and entries
 * below n of d_lens, d_peer, d_descs; a slot is written from the last entry whose `first` is at or below it, so
 * on a table whose `first` does not ascend which slots are written is unspecified.
 *
 * qgcm_gso_resolve: device arrays, asynchronous on stream, one launch; the route table is taken as
 * qgcm_frames_resolve takes it.  d_packed, d_frames and d_descs 16-B aligned, the d_packed allocation rounded up
 * to 16 B; d_lens, d_peer and d_arena 4-B aligned; stride a multiple of 4, at least 8 (a multiple of 16 under a
 * 16-B-aligned arena takes the 16-byte path, anything else the dword path).  n == 0 or n_frames == 0: QGCM_OK,
 * nothing launched.  n > QGCM_MAX_BATCH, n_frames > n, a bad stride, a NULL or misaligned pointer, or a call before
 * qgcm_routes_set: QGCM_E_ARG, nothing launched.
 *
 * qgcm_gso_unpack_cpu: the segmentation for host arrays (no alignment asked): lens[i] and Raw[4 : 4 + min(L,
 * stride - 4)) of every slot, nothing else; the yardstick, and the path of a worker without a device.
 *
 * qgcm_tun_open_offload: qgcm_tun_open plus IFF_VNET_HDR, TUNSETVNETHDRSZ = 10 and TUNSETOFFLOAD.  `offloads`:
 * QGCM_TUN_TSO4 asks for TUN_F_CSUM | TUN_F_TSO4, QGCM_TUN_USO adds TUN_F_CSUM | TUN_F_USO4 | TUN_F_USO6 (the
 * kernel takes the two only as a pair); TUN_F_TSO6 and TUN_F_TSO_ECN are never set; any other bit: -EINVAL.
 * Returns 0 or -errno (every queue opened so far closed).
 *
 * qgcm_tun_read_gso: qgcm_tun_read_packed for such a queue.  Each read lands so that the IP packet starts on a
 * 16-byte boundary with the vnet header in the 10 bytes before it (the first packet at packed + 16).  It reads
 * only with 65536 + 16 bytes of room, only with at least QGCM_GSO_SEGS slots of max_n left, and at most
 * max_frames times, and fills one table entry a read from the vnet header: no GSO type -> PLAIN, or CSUM with
 * NEEDS_CSUM (csum_start, csum_offset); TCPV4 -> TCP4 and UDP_L4 over IPv4 -> UDP4 with l4_off = csum_start,
 * gso_size from the header, and the TCP header length from the packet's data-offset nibble (the vnet hdr_len is
 * the linear part of the kernel's buffer and is not used).  A frame it does not split -- TCPV6, UDP_L4 over
 * IPv6, UFO, the ECN bit, a read shorter than the vnet header, anything the validity rule refuses -- is written
 * as the PLAIN entry of length 0 at its offset, which gives its one slot the void-frame result, and is counted
 * in out[2].  Returns the number of slots named, 0 on timeout, -1 on an error (also a NULL array, packed_cap
 * below 65536 + 16 or max_n below QGCM_GSO_SEGS); out (may be NULL) = {entries, bytes used = the end of the last
 * frame, frames not split}.
 *
 * qgcm_route_chain_seal_gso_host: qgcm_route_chain_seal_frames_host with qgcm_gso_resolve in place of
 * qgcm_frames_resolve.  The table is checked first (above).  Chunks hold whole entries, as many as fit that
 * call's limits (65536 packets, 256 MiB of slots; a lone entry of more is a chunk of its own); per chunk only
 * the packed bytes its entries span and the entries, rebased to the span and to the chunk's first slot, go up;
 * everything after the first launch is that call's.  h_nonces n * 12 bytes or QGCM_NONCES_GENERATE.  The outputs
 * are what qgcm_route_chain_seal_frames_host gives, chunked at the same slots, for the packets
 * qgcm_gso_unpack_cpu makes.  After QGCM_E_NOMEM (out written) the call is repeated with the entries from the one
 * whose `first` is out[0] on, their `first` reduced by out[0]. */
#define QGCM_GSO_PLAIN 0u  /* copy only */
#define QGCM_GSO_CSUM  1u  /* copy, complete a partial checksum */
#define QGCM_GSO_TCP4  2u  /* split an IPv4 TCP super-frame */
#define QGCM_GSO_UDP4  3u  /* split an IPv4 UDP (UDP_L4) super-frame */
#define QGCM_GSO_SEGS  2048u
#define QGCM_TUN_TSO4 1u
#define QGCM_TUN_USO  2u
typedef struct qgcm_gso_frame {
    uint32_t off, len;            /* the IP packet in the packed area (behind the vnet header); off % 16 == 0 */
    uint32_t first, count;        /* its first slot, its number of slots */
    uint16_t gso_size, hdr_len;   /* payload bytes a segment; IP + L4 header bytes (TCP4/UDP4) */
    uint16_t l4_off, csum_off;    /* csum_start (= IPv4 header length for TCP4/UDP4); csum_offset (CSUM only) */
    uint32_t kind, reserved;      /* reserved: 0 on the read side, d_peer of `first` from qgcm_deliver_coalesce */
} qgcm_gso_frame;                 /* 32 bytes, 16-B aligned */
int qgcm_tun_open_offload(const char *name, int queues, int *fds, char *ifname_out, size_t ifname_len,
                          uint32_t offloads);
int qgcm_tun_read_gso(int fd, uint8_t *packed, uint64_t packed_cap, qgcm_gso_frame *frames, uint32_t max_frames,
                      uint32_t max_n, int timeout_ms, uint64_t out[3]);
int qgcm_gso_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gso_frame *d_frames,
                     uint32_t n_frames, uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens,
                     uint32_t *d_peer, qgcm_desc *d_descs, void *stream);
int qgcm_gso_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_gso_frame *frames, uint32_t n_frames,
                        uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens);
int qgcm_route_chain_seal_gso_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                   const qgcm_gso_frame *frames, uint32_t n_frames, uint64_t stride, uint32_t n,
                                   uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins,
                                   const qgcm_plan_limits *limits, uint32_t *h_peer, uint8_t *h_status,
                                   uint8_t *h_out, uint64_t out_cap, qgcm_ptrain *h_ptrains, uint32_t *h_order,
                                   uint64_t out[4]);

/* ---- delivered TCP segments coalesced on routed batches: GRO for the TUN write ---- */
/* The mirror of the section above.  A TUN queue with IFF_VNET_HDR takes a virtio_net_hdr with GSO_TCPV4 on write as
 * it hands one over on read, so a train of in-order TCP segments can go up as one frame: one write(2), one trip
 * through the receiving stack.  Which neighbours may be merged is a comparison of headers and a ones'-complement
 * sum over every byte; the merged frame goes up with NEEDS_CSUM and is trusted, so both checksums of every segment
 * are verified first, and a segment that crossed the tunnel with a bad checksum reaches the receiver as it is.
 *
 * Packet i is delivered exactly as qgcm_deliver_pack defines it: d_status[i] == 1 and 4 + d_lens[i] <= stride
 * (d_status == NULL: all 1); p = Raw[4 : 4 + L] is the packet.
 *
 * Candidate: a delivered packet with, every offset taken from p and bounded by L: L >= 40; p[0] >> 4 == 4;
 * ihl = 4 * (p[0] & 15) in [20, 60]; IPv4 total length == L; protocol 6; (p[6:8] & 0xbfff) == 0 (no fragment,
 * reserved bit clear, DF either way); doff = 4 * (p[ihl + 12] >> 4) in [20, 60]; hdr = ihl + doff and
 * P = L - hdr >= 1; the low nibble of p[ihl + 12] zero; TCP flags with (flags & 0xf7) == 0x10 (ACK, optionally
 * PSH, nothing else); the IPv4 header checksum field equal to the value recomputed over ihl bytes; the TCP
 * checksum field equal to the value recomputed from scratch over pseudo-header (protocol 6, length L - ihl),
 * header and payload, an odd length padded with a zero byte.  "Recomputed" is the value qgcm_gso_resolve would
 * write for that packet; equality with it, not "sums to 0xffff", is the rule (a field of 0xffff where 0x0000 is
 * recomputed is no candidate), so that segmentation and coalescing are exact inverses.
 *
 * link(i), 1 <= i < n: slots i - 1 and i are both candidates; d_peer equal; ihl and doff equal; every header
 * byte equal except IP total length, IP id, IP checksum, TCP sequence number, the PSH bit and TCP checksum (so
 * TOS, DF, TTL, addresses, IP options, ports, ack, window, urgent and TCP options match); seq_i == seq_{i-1} +
 * P_{i-1} mod 2^32; id_i == id_{i-1} + 1 mod 2^16; PSH clear on i - 1.  eq(i) = link(i) and P_i == P_{i-1};
 * lt(i) = link(i) and P_i < P_{i-1}; both false at i = 0 and i = n.  Adjacency is by slot: a dropped slot ends a
 * run as a packet of another flow does.
 *
 * Frames.  A stretch is a maximal run under eq, head h, j = i - h.  m = min(QGCM_COALESCE_SEGS, (65535 - hdr) / P).
 * Members of a stretch with equal j / m form one frame (the send plan's cut: no sequential walk).  Slot t is a
 * tail when lt(t) && !eq(t + 1) && !lt(t - 1) and the frame that ends at t - 1 has fewer than m members; it joins
 * that frame as its last member.  Three strictly falling sizes in a row merge only the first two: the rule stays
 * local.  A frame of one member is a PLAIN entry.  Every delivered packet appears in exactly one entry, in slot
 * order: no flow is reordered.
 *
 * Output: a packed area and a qgcm_gso_frame table in the layout qgcm_tun_read_gso produces.  Entry k's IP packet
 * starts at off_k, a multiple of 16, off_0 = 16; its 10-byte virtio_net_hdr lies in [off_k - 10, off_k), bytes
 * [off_k - 16, off_k - 10) are zero, the packet is zero-padded to 16 bytes, off_{k+1} = off_k + round16(len_k) + 16.
 *   PLAIN entry:     kind QGCM_GSO_PLAIN, ten zero bytes of vnet header, the packet verbatim, count 1, the other
 *                    16-bit fields 0.
 *   Coalesced entry: (c >= 2 members) kind QGCM_GSO_TCP4, gso_size the head's P, hdr_len = hdr, l4_off = ihl,
 *                    csum_off = 16, count = c.  The packet is the head's hdr bytes, then the members' payloads back
 *                    to back.  The header is the head's with: total length hdr + sum of P; the IPv4 checksum
 *                    recomputed; PSH taken from the last member; in the TCP checksum field the folded,
 *                    uncomplemented ones'-complement sum of the pseudo-header (source, destination, 6, doff + sum
 *                    of P), which is what NEEDS_CSUM expects.  The vnet header, host byte order: flags 1, gso_type
 *                    1 (TCPV4), hdr_len, gso_size, csum_start ihl, csum_offset 16.
 *   Every entry:     `first` the first member's slot, `reserved` d_peer of that slot.
 * counts[4] = {entries, bytes = the end of the last entry, coalesced entries, delivered packets}; bytes is the
 * full need even when it does not fit.  An entry whose region [off - 16, off + round16(len)) passes packed_cap is
 * not copied and gets off = 0xffffffff; such entries form a suffix.  Every byte of [0, bytes) that fits is
 * determined; everything behind it is untouched; table entries past counts[0] are unspecified.
 * On any input no byte of a slot at or past 4 + L has any effect.  Loads are whole aligned dwords (16-byte pieces
 * on the 16-byte path) that hold a byte below 4 + L: the bytes up to that dword's (that piece's) end, which lies
 * inside the slot because stride is a multiple of 4 (of 16), are loaded and masked off, and nothing behind it is
 * read.  Nothing at or past packed_cap is written, nothing past entry n of the table is written.
 *
 * qgcm_deliver_coalesce: device arrays, asynchronous on stream, no context state, no host synchronisation between
 * its launches, calls on several streams may run at once.  Alignments as qgcm_deliver_pack's (d_frames, n entries,
 * 16-B aligned; d_counts four uint64, 8-B aligned; d_work qgcm_deliver_coalesce_work(n) bytes, 16-B aligned, the
 * call's own until it has run); a stride that is a multiple of 16 under a 16-B-aligned arena takes the 16-byte
 * path, anything else the dword path.  n == 0: counts = {0, 0, 0, 0}, nothing else launched.  QGCM_E_ARG as
 * qgcm_deliver_pack.
 * qgcm_deliver_coalesce_cpu: the same contract for host arrays (no alignment asked), by the host: the yardstick,
 * and the path of a worker on qgcm_route_chain_open_host.
 *
 * qgcm_tun_write_gso: for a queue from qgcm_tun_open_offload (any `offloads`, 0 included).  The whole table is
 * checked first: every entry off >= 16, off % 16 == 0, off + len <= packed_len, kind PLAIN or TCP4, a TCP4 entry
 * valid by the rule of the section above apart from `first`; else -1 with nothing written.  Then
 * packed[off - 10, off + len) of each entry is written, in order; EINTR is retried; a TCP4 entry the kernel
 * refuses with EINVAL is cut on the host (qgcm_gso_unpack_cpu's segmentation) and written packet by packet behind
 * zero vnet headers; any other refusal ends the batch as in qgcm_tun_write_packed.  Returns the entries written,
 * or -1 when none was; out (may be NULL) = {entries, packets, entries that fell back}.
 *
 * qgcm_route_chain_open_coalesced_host / qgcm_route_chain_open_gro_coalesced_host: the two ..._packed_host
 * pipelines with the pack's launch replaced.  Chunks, order, accounting, QGCM_E_NOMEM and the rebasing of `off`
 * and `first` are those of the packed forms; the device area of a chunk is cn * (round16(stride) + 16) bytes; runs
 * do not cross a chunk edge: the result is qgcm_deliver_coalesce_cpu applied chunk by chunk, the chunks' areas
 * one behind the other.  out[5] = {packets processed, entries, bytes, coalesced entries, delivered packets}. */
#define QGCM_COALESCE_SEGS 64u
uint64_t qgcm_deliver_coalesce_work(uint32_t n);
int qgcm_deliver_coalesce(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                          const uint32_t *d_peer, const uint8_t *d_status, uint8_t *d_packed, uint64_t packed_cap,
                          qgcm_gso_frame *d_frames, uint64_t *d_counts, void *d_work, void *stream);
int qgcm_deliver_coalesce_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                              const uint32_t *peer, const uint8_t *status, uint8_t *packed, uint64_t packed_cap,
                              qgcm_gso_frame *frames, uint64_t counts[4]);
int qgcm_tun_write_gso(int fd, const uint8_t *packed, uint64_t packed_len, const qgcm_gso_frame *frames, uint32_t m,
                       uint64_t out[3]);
int qgcm_route_chain_open_coalesced_host(qgcm_ctx *ctx, const uint8_t *h_arena, uint64_t stride, uint32_t n,
                                         uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                         uint8_t *h_out, uint64_t out_cap, qgcm_gso_frame *h_frames, uint64_t out[5]);
int qgcm_route_chain_open_gro_coalesced_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                             const qgcm_gro_buf *bufs, uint32_t n_bufs, uint64_t stride, uint32_t n,
                                             uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                             uint8_t *h_out, uint64_t out_cap, qgcm_gso_frame *h_frames,
                                             uint64_t out[5]);

/* ---- DTLS 1.2 records on routed batches ---- */
/* The record layer of quantum's `dtls` backend (socket/dtls.go, crypto/dtls.c) for established sessions: every
 * Payload.Raw[:Length] that SSL_write would turn into one application-data record, and every record SSL_read
 * would open, as one GPU batch.  The reference fixes the suite to ECDHE-{ECDSA,RSA}-AES256-GCM-SHA384 over DTLS
 * 1.2 (dtls.h:19, dtls.c:194-204), so one cipher and one record format cover it.  Handshake, certificates,
 * cookies, alerts and retransmission stay in the host's DTLS stack.
 *
 * Record on the wire (RFC 6347 4.1, RFC 5288 3):
 *   type(1) = 23 | version(2) = FE FD | epoch(2) | seq(6) | length(2) = 8 + L + 16 | explicit_nonce(8) |
 *   ciphertext(L) | tag(16)
 * AES-256-GCM with nonce = write_IV(4) | explicit_nonce(8) and the 13 bytes of additional data
 *   epoch(2) | seq(6) | type | version(2) | L(2, big endian).
 * A sealed record carries explicit_nonce = epoch | seq; an opened one takes it from the record (OpenSSL's is
 * not the sequence number).
 *
 * Sessions.  A session is indexed like a peer (0 .. max_keys - 1, the index the resolve launches leave in d_peer)
 * and owns two key slots of the context, one per direction.  qgcm_dtls_sessions_set installs both keys of every
 * session of the call in one install pass (as qgcm_set_keys) and writes the device session table (allocated on
 * first use): slots, IVs, epochs, write_seq, and an empty anti-replay window (right edge R = 0, bitmap W = 0).
 * Errors, nothing installed: QGCM_E_ARG (NULL context, NULL keys with count > 0, write_slot == read_slot,
 * write_seq > 2^48, a slot named twice in the call), QGCM_E_KEY (first + count or a slot beyond max_keys).  An
 * epoch change (a renegotiation) means qgcm_dtls_sessions_set again.  qgcm_dtls_sessions_clear marks the sessions
 * unset and releases their key slots (qgcm_clear_keys).  qgcm_dtls_session_state reads {write_seq, R, W, set}
 * after synchronising the context's device.  Calls that touch the same session (set, clear, seal, open, state)
 * must be ordered by the caller: one stream, or a synchronisation between them.
 * qgcm_dtls_key_block (host): PRF_SHA384(master_secret, "key expansion", server_random | client_random), the 72
 * bytes client_write_key[32] | server_write_key[32] | client_write_IV[4] | server_write_IV[4] (RFC 5246 5, 6.3)
 * from what SSL_SESSION_get_master_key, SSL_get_client_random and SSL_get_server_random return.
 *
 * Slot form.  The record is kept split so that it composes with the rest of the path: the slot holds
 * ciphertext | tag at Raw[0 : L + 16] (what qgcm_chain_outgoing leaves and qgcm_deliver_pack takes is
 * Raw[0 : Length]); the 21 bytes in front live in a side array of qgcm_dtls_hdr: b[0:13] the record header,
 * b[13:21] the explicit nonce, b[21:32] zero after a seal and ignored by an open.  Arena 4-byte aligned, stride a
 * multiple of 4 (as qgcm_resolve_*), the header array 16-byte aligned.
 *
 * d_status[i] is 1 (sealed / delivered) or 0; d_reason (may be NULL) says why, and when several apply the
 * lowest step below wins (NO_SESSION before NOT_APPDATA / MALFORMED before AUTH before REPLAY; on the seal side
 * NO_SESSION before MALFORMED before SEQ_EXHAUSTED).
 *
 * qgcm_dtls_seal, slot i with p = d_peer[i], L = d_lens[i]:
 *   1. NO_SESSION: p >= max_keys, session unset, or its write key slot unset.
 *   2. MALFORMED: L == 0, L > 16384 or L + 16 > stride.
 *   3. The remaining packets of a session are numbered in arena order, seq = write_seq[p] + rank;
 *      SEQ_EXHAUSTED when seq > 2^48 - 1.  After the call write_seq[p] has advanced by the number of packets
 *      numbered, saturating at 2^48.
 *   4. A sealed packet: d_hdr[i] = 23 | FE FD | write_epoch | seq48 | (8 + L + 16) | write_epoch | seq48 | zeros,
 *      Raw[0:L] encrypted in place, tag at Raw[L : L + 16], d_lens[i] = L + 16, status 1.
 *   A rejected packet leaves slot, header entry and length untouched.  No byte of a slot at or past L + 16 is
 *   written.
 * qgcm_dtls_open, slot i with p = d_peer[i], B = d_lens[i] (bytes in the slot):
 *   1. NO_SESSION as above with the read key slot.
 *   2. NOT_APPDATA: b[0] != 23 (handshake retransmits, alerts, change-cipher-spec: they go to the host's DTLS
 *      stack).  Slot untouched.
 *   3. MALFORMED: version not FE FD, epoch not read_epoch, B < 17, B > 16400, B > stride, or the length field
 *      not 8 + B.  Slot untouched.
 *   4. AUTH: tag mismatch.  Raw[0 : B - 16] zeroed (as qgcm_open_batch), the tag and what follows untouched.
 *   5. REPLAY: the authentic packets of each session, in arena order, pass RFC 6347 4.1.2.6 packet by packet
 *      (OpenSSL's bitmap rule): bit k of W means R - k was seen; s > R is accepted and the window shifts; else
 *      rejected when R - s >= 64 or the bit is set, else accepted and the bit set.  A replayed packet keeps its
 *      plaintext in the slot; neither d_lens[i] nor the window changes for it.  Only authentic packets count: a
 *      forged record ahead of an authentic one with the same number does not make the latter a replay.
 *   6. Delivered: status 1, plaintext at Raw[0 : B - 16], d_lens[i] = B - 16.
 *   The session's (R, W) after the call is the sequential rule's end state.
 * Both: device arrays, asynchronous on stream, work areas owned by the context (calls on one context are
 * serialised on the device like descriptor batches); n == 0 launches nothing.  QGCM_E_ARG: NULL context or
 * arrays (d_status included; d_reason may be NULL), arena or d_lens / d_peer not 4-byte aligned, d_hdr not 16-byte
 * aligned, stride not a multiple of 4, below 20 or above 2^32, n > QGCM_MAX_BATCH; QGCM_E_KEY: no session was ever
 * set on the context.  The seal's numbering launch writes a sealed record's header entry, so the GCM kernel reads
 * header entries alike on both sides.
 * The window and the numbering run as a stable radix sort by session (and by (session, seq) for duplicates) and
 * reduce-then-scan launches; no workgroup waits for another and the result does not depend on scheduling.
 *
 * Host forms of the two ordered rules (quantum_amd/csrc/dtls_core.h), for tests and small batches; libqgcm has
 * no host AES-GCM:
 * qgcm_dtls_number_cpu: the seal's steps 1-3 and the header of step 4 for host arrays.  `keys` (n_sessions
 *   entries, a NULL entry list with n_sessions == 0 allowed) describes the sessions; set[p] != 0 marks session p
 *   usable (NULL: all); write_seq[p] is read and advanced.  hdr, lens, status and reason (may be NULL) are
 *   written as the seal writes them; the slots are not touched.
 * qgcm_dtls_replay_cpu: the open's step 5 over n packets given as (session, seq, authentic): accept[i] = 1 for a
 *   delivered packet; state[2 p] = R and state[2 p + 1] = W of session p < n_sessions are read and updated; a
 *   packet that is not authentic, or whose session is >= n_sessions, gets 0 and counts for nothing.
 *   parallel != 0 evaluates the parallel form (prefix maximum, duplicate test, closed-form end state), 0 the
 *   packet-by-packet rule; the two agree. */
#define QGCM_DTLS_OK 0
#define QGCM_DTLS_NO_SESSION 1
#define QGCM_DTLS_NOT_APPDATA 2
#define QGCM_DTLS_MALFORMED 3
#define QGCM_DTLS_AUTH 4
#define QGCM_DTLS_REPLAY 5
#define QGCM_DTLS_SEQ_EXHAUSTED 6
#define QGCM_DTLS_MAX_PLAIN 16384u /* RFC 6347 4.1: the longest plaintext fragment of a record */
#define QGCM_DTLS_HDR_BYTES 21u    /* record header and explicit nonce: what travels in front of the slot's bytes */
typedef struct qgcm_dtls_keys {
    uint8_t write_key[32], read_key[32];
    uint8_t write_iv[4], read_iv[4];
    uint16_t write_epoch, read_epoch; /* 1 after a first handshake */
    uint32_t write_slot, read_slot;   /* key slots of the context, distinct, < max_keys */
    uint64_t write_seq;               /* next sequence number to hand out, <= 2^48 */
} qgcm_dtls_keys;
typedef struct qgcm_dtls_hdr {
    uint8_t b[32];
} qgcm_dtls_hdr;
int qgcm_dtls_sessions_set(qgcm_ctx *ctx, uint32_t first, uint32_t count, const qgcm_dtls_keys *keys);
int qgcm_dtls_sessions_clear(qgcm_ctx *ctx, uint32_t first, uint32_t count);
int qgcm_dtls_session_state(qgcm_ctx *ctx, uint32_t session, uint64_t out[4]); /* {write_seq, R, W, set} */
int qgcm_dtls_key_block(const uint8_t master[48], const uint8_t client_random[32], const uint8_t server_random[32],
                        uint8_t out[72]);
int qgcm_dtls_seal(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                   const uint32_t *d_peer, qgcm_dtls_hdr *d_hdr, uint8_t *d_status, uint8_t *d_reason, void *stream);
int qgcm_dtls_open(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                   const uint32_t *d_peer, const qgcm_dtls_hdr *d_hdr, uint8_t *d_status, uint8_t *d_reason,
                   void *stream);
int qgcm_dtls_number_cpu(const qgcm_dtls_keys *keys, const uint8_t *set, uint64_t *write_seq, uint32_t n_sessions,
                         uint64_t stride, uint32_t n, uint32_t *lens, const uint32_t *peer, qgcm_dtls_hdr *hdr,
                         uint8_t *status, uint8_t *reason);
int qgcm_dtls_replay_cpu(uint32_t n, const uint32_t *session, const uint64_t *seq, const uint8_t *authentic,
                         uint32_t n_sessions, uint64_t *state, uint8_t *accept, int parallel);

/* Split records over UDP, one record per datagram (what OpenSSL sends for application data).
 * qgcm_udp_send_dtls: sendmmsg with two iovecs a datagram, hdr[i].b[0:21] then Raw[0 : lens[i]] of slot i, for the
 *   slots whose status is 1 (NULL: all) and whose peer[i] < n_addrs, to addrs[peer[i]], as qgcm_udp_send_slots_to.
 *   Returns the datagrams sent or -1.
 * qgcm_udp_recv_dtls: recvmmsg with two iovecs: the first 21 bytes to hdr[i] (b[21:32] zeroed), the rest to slot
 *   i, lens[i] the bytes in the slot, the sender to addrs_out[i] (may be NULL).  Waits up to timeout_ms for the
 *   first datagram (0: no wait, < 0: for ever), then takes what is queued.  A datagram shorter than 22 bytes or
 *   longer than 21 + stride is dropped and counted in *dropped (may be NULL).  Returns the slots filled or -1. */
int qgcm_udp_send_dtls(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                       const qgcm_dtls_hdr *hdr, const uint8_t *status, const uint32_t *peer,
                       const qgcm_peer_addr *addrs, uint32_t n_addrs);
int qgcm_udp_recv_dtls(int fd, uint8_t *arena, uint64_t stride, uint32_t max_n, uint32_t *lens, qgcm_dtls_hdr *hdr,
                       qgcm_peer_addr *addrs_out, int timeout_ms, uint32_t *dropped);

/* ---- introspection: which kernels served this context's calls ---- */
/* Launch counts per kernel family since qgcm_create (uniform batches launch in chunks of 2^19
 * packets; a descriptor batch launches the segmented kernel and then the per-wave kernel for its
 * short keys; gcm_one_kernel serves per-packet calls the resident kernel does not take and uniform
 * batches of up to 2048 packets).  Writes min(n, QGCM_KERNEL_COUNTERS) counters, returns that number or -1. */
#define QGCM_KERNEL_QUAD 0      /* gcm_quad_kernel, single-key (uniform) batches */
#define QGCM_KERNEL_SEGMENTED 1 /* gcm_seg_kernel, descriptor batches (long key runs) */
#define QGCM_KERNEL_PER_WAVE 2  /* gcm_quad_kernel, descriptor batches (short key runs) */
#define QGCM_KERNEL_ONE 3       /* gcm_one_kernel, one workgroup per packet */
#define QGCM_KERNEL_RESIDENT 4  /* per-packet calls served by the resident kernel (requests, not launches) */
#define QGCM_KERNEL_SNAPPY_ENC 5 /* snappy_compress_kernel (device codec; chained calls: one per device chunk) */
#define QGCM_KERNEL_SNAPPY_DEC 6 /* snappy_uncompress_kernel */
#define QGCM_KERNEL_TAIL_WAITS 7 /* uniform launches that waited, on their stream, for their shared-tail counter
                                    set's previous launch (the context's ring came round; not a launch) */
#define QGCM_KERNEL_COUNTERS 8
int qgcm_launch_counts(const qgcm_ctx *ctx, uint64_t *out, int n);

/* ---- measurement: achievable HBM copy rate (reads + writes bytes) for the roofline ---- */
/* 16-B aligned device buffers, bytes a multiple of 16.  Asynchronous on stream. */
int qgcm_stream_copy(qgcm_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes, void *stream);

/* ---- synthetic workload generator (bench/tests; BASELINE.json configs) ---- */
/* Slot i at i*stride: [aad_word LE][payload L bytes of the splitmix64(seed_payload) stream at
 * byte offset i*L]; nonces[i*12..] = splitmix64(seed_nonce) stream at byte offset i*12. */
int qgcm_fill_uniform(uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t len, uint32_t aad_word,
                      uint64_t seed_payload, uint8_t *d_nonces, uint64_t seed_nonce, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QGCM_H */
