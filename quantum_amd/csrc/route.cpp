// route.cpp -- the route table, the link counters and the routed host pipelines of include/qgcm.h
// ("routes resolved on the GPU").  Host work only: the open-addressing table is built here
// and uploaded, the kernels of route_kernels.hip do everything per packet.
//
// Table lifetime: qgcm_routes_set uploads the new table into a fresh allocation, swaps the context's
// pointer under the route lock, and then releases the old allocation with hipFree, which waits for the
// device: every launch that took the old pointer as its argument has finished by then.  A resolve holds
// the route lock from reading the pointer until its kernel is enqueued, so it never launches with a table
// that is already freed.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/qgcm.h"
#include "coalesce_core.h"
#include "frames_core.h"
#include "gcm_internal.h"
#include "gro_core.h"
#include "gso_core.h"
#include "pack_core.h"
#include "send_plan_core.h"
#include "train_core.h"

namespace qgcm {

constexpr uint32_t kRouteChunk = 65536;         // packets per chunk of the routed host pipelines
constexpr uint64_t kRouteChunkBytes = 256ull << 20;  // ... and bytes of slots

struct RouteState {
    std::mutex mu;  // the table pointer, the net and the counters' allocation
    bool set = false;
    uint2 *d_table = nullptr;
    uint32_t cap_mask = 0;
    qgcm_route_net net{};
    unsigned long long *d_counters = nullptr;  // [2 directions][1 + max_keys][4]
    size_t dir_words = 0;                      // 4 * (1 + max_keys)
    uint8_t *d_plugins = nullptr;  // [max_keys] per-peer plugin flags, made by the first qgcm_peer_plugins_set and
                                   // kept until the context goes (NULL: every peer QGCM_PLUGIN_ENCRYPTION)

    // the routed host pipelines: one stream, device staging grown on demand, one call at a time
    std::mutex pipe_mu;
    hipStream_t stream = nullptr;
    uint8_t *d_arena = nullptr, *d_side = nullptr;
    size_t arena_cap = 0, side_cap = 0;
    std::vector<uint8_t> h_stat;

    // qgcm_send_plan_host: its device arrays and work area (under pipe_mu, on `stream`), and the batch size
    // from which it plans on the device (QGCM_PLAN_DEVICE_MIN, read when the context is created)
    uint8_t *d_plan = nullptr;
    size_t plan_cap = 0;
    uint32_t plan_device_min = kPlanDeviceMin;

    // the coalesced-receive pipelines unpack and resolve a chunk with gro_unpack_kernel and the resolve kernel;
    // QGCM_GRO_FUSED=1 when the context is created selects the one launch of qgcm_gro_resolve instead (same
    // outputs).  The pair is the default because the pipeline measured 1-2 % slower with the one launch: a
    // chunk of 65536 slots gives it 1024 waves where the unpack has 16384
    bool gro_fused = false;

    // the pipelines whose batch arrives packed (coalesced buffers, frames, super-frames): a chunk's table and
    // packed bytes on the device, the rebased table on the host (under pipe_mu, on `stream`; one call at a time,
    // so one area serves the three forms)
    uint8_t *d_stage = nullptr;
    size_t stage_cap = 0;
    std::vector<uint8_t> h_stage;

    // the packed pipelines: a chunk's records, counts, scan work area and packed bytes on the device (under
    // pipe_mu, on `stream`)
    uint8_t *d_pack = nullptr;
    size_t pack_cap = 0;

    // the packed outgoing pipeline: a chunk's plan, its packed table, counts, work areas and packed bytes on the
    // device (under pipe_mu, on `stream`)
    uint8_t *d_train = nullptr;
    size_t train_cap = 0;
};

RouteState *route_state_create() {
    RouteState *r = new RouteState();
    if (const char *v = getenv("QGCM_PLAN_DEVICE_MIN"))
        if (*v) r->plan_device_min = (uint32_t)std::min<unsigned long long>(strtoull(v, nullptr, 0), 0xffffffffull);
    if (const char *v = getenv("QGCM_GRO_FUSED"))
        if (*v) r->gro_fused = strtoull(v, nullptr, 0) != 0;
    return r;
}

void route_state_destroy(RouteState *r) {
    if (!r) return;
    hipFree(r->d_table);
    hipFree(r->d_counters);
    hipFree(r->d_plugins);
    hipFree(r->d_arena);
    hipFree(r->d_side);
    hipFree(r->d_plan);
    hipFree(r->d_stage);
    hipFree(r->d_pack);
    hipFree(r->d_train);
    if (r->stream) hipStreamDestroy(r->stream);
    delete r;
}

}  // namespace qgcm

using namespace qgcm;

namespace {

int hip_rc(hipError_t e) { return e == hipSuccess ? QGCM_OK : QGCM_E_HIP; }

int resolve(qgcm_ctx *ctx, bool outgoing, uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
            uint32_t *d_peer, qgcm_desc *d_descs, hipStream_t s) {
    if (!ctx) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    if ((stride & 3) || n > QGCM_MAX_BATCH) return QGCM_E_ARG;
    if (n && (!d_arena || !d_lens || !d_peer || !d_descs || stride == 0)) return QGCM_E_ARG;
    if (((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) || ((uintptr_t)d_peer & 3) || ((uintptr_t)d_descs & 15))
        return QGCM_E_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->set) return QGCM_E_ARG;
    if (n == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    RouteArgs a{};
    a.table = r->d_table;
    a.cap_mask = r->cap_mask;
    a.net = r->net.net;
    a.mask = r->net.mask;
    a.gateway = r->net.gateway;
    a.own_ip = r->net.own_ip;
    a.arena = d_arena;
    a.stride = stride;
    a.n = n;
    a.lens = d_lens;
    a.peer = d_peer;
    a.descs = d_descs;
    return hip_rc(launch_route_resolve(outgoing, a, s));
}

// qgcm_frames_resolve: resolve() for a batch that is still packed; the table pointer is taken the same way.
int frames_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_frame *d_frames, uint32_t n,
                   uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, uint32_t *d_peer, qgcm_desc *d_descs, hipStream_t s) {
    if (!ctx) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    if ((stride & 3) || stride < 8 || n > QGCM_MAX_BATCH) return QGCM_E_ARG;
    if (n && (!d_packed || !d_frames || !d_arena || !d_lens || !d_peer || !d_descs)) return QGCM_E_ARG;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_frames & 7) || ((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) ||
        ((uintptr_t)d_peer & 3) || ((uintptr_t)d_descs & 15))
        return QGCM_E_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->set) return QGCM_E_ARG;
    if (n == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    FramesArgs a{};
    a.packed = d_packed;
    a.packed_len = packed_len;
    a.frames = d_frames;
    a.n = n;
    a.arena = d_arena;
    a.stride = stride;
    a.lens = d_lens;
    a.peer = d_peer;
    a.descs = d_descs;
    a.table = r->d_table;
    a.cap_mask = r->cap_mask;
    a.net = r->net.net;
    a.mask = r->net.mask;
    a.gateway = r->net.gateway;
    a.own_ip = r->net.own_ip;
    return hip_rc(launch_frames_resolve(a, s));
}

// qgcm_gso_resolve: frames_resolve() for a table of super-frames; the table pointer is taken the same way.
int gso_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gso_frame *d_frames, uint32_t n_frames,
                uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, uint32_t *d_peer, qgcm_desc *d_descs,
                hipStream_t s) {
    if (!ctx) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    if ((stride & 3) || stride < 8 || n > QGCM_MAX_BATCH || n_frames > n) return QGCM_E_ARG;
    if (n && (!d_packed || !d_frames || !d_arena || !d_lens || !d_peer || !d_descs)) return QGCM_E_ARG;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_frames & 15) || ((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) ||
        ((uintptr_t)d_peer & 3) || ((uintptr_t)d_descs & 15))
        return QGCM_E_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->set) return QGCM_E_ARG;
    if (n == 0 || n_frames == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    GsoArgs a{};
    a.packed = d_packed;
    a.packed_len = packed_len;
    a.frames = d_frames;
    a.n_frames = n_frames;
    a.n = n;
    a.arena = d_arena;
    a.stride = stride;
    a.lens = d_lens;
    a.peer = d_peer;
    a.descs = d_descs;
    a.table = r->d_table;
    a.cap_mask = r->cap_mask;
    a.net = r->net.net;
    a.mask = r->net.mask;
    a.gateway = r->net.gateway;
    a.own_ip = r->net.own_ip;
    return hip_rc(launch_gso_resolve(a, s));
}

// qgcm_gro_resolve: resolve(ctx, false, ...) for a batch that is still in its coalesced buffers; the table pointer
// is taken the same way.  Without a table there is nothing to unpack: the existing resolve kernel.
int gro_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gro_buf *d_bufs, uint32_t n_bufs,
                uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, uint32_t *d_peer, qgcm_desc *d_descs,
                hipStream_t s) {
    if (!ctx) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    if ((stride & 3) || stride == 0 || n > QGCM_MAX_BATCH || n_bufs > n) return QGCM_E_ARG;
    if (n && (!d_packed || !d_bufs || !d_arena || !d_lens || !d_peer || !d_descs)) return QGCM_E_ARG;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_bufs & 15) || ((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) ||
        ((uintptr_t)d_peer & 3) || ((uintptr_t)d_descs & 15))
        return QGCM_E_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->set) return QGCM_E_ARG;
    if (n == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    if (n_bufs == 0) {
        RouteArgs ra{};
        ra.table = r->d_table;
        ra.cap_mask = r->cap_mask;
        ra.net = r->net.net;
        ra.mask = r->net.mask;
        ra.gateway = r->net.gateway;
        ra.own_ip = r->net.own_ip;
        ra.arena = d_arena;
        ra.stride = stride;
        ra.n = n;
        ra.lens = d_lens;
        ra.peer = d_peer;
        ra.descs = d_descs;
        return hip_rc(launch_route_resolve(false, ra, s));
    }
    GroResolveArgs a{};
    a.packed = d_packed;
    a.packed_len = packed_len;
    a.bufs = d_bufs;
    a.n_bufs = n_bufs;
    a.n = n;
    a.arena = d_arena;
    a.stride = stride;
    a.lens = d_lens;
    a.peer = d_peer;
    a.descs = d_descs;
    a.table = r->d_table;
    a.cap_mask = r->cap_mask;
    a.net = r->net.net;
    a.mask = r->net.mask;
    a.gateway = r->net.gateway;
    return hip_rc(launch_gro_resolve(a, s));
}

template <typename T>
bool grow(T *&p, size_t &cap, size_t need) {
    if (need <= cap) return true;
    hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, need) != hipSuccess) return false;
    cap = need;
    return true;
}

constexpr uint32_t kAllPlugins = QGCM_PLUGIN_COMPRESSION | QGCM_PLUGIN_ENCRYPTION;

// The plugin chain between a resolve and the accounting, on s (qgcm_chain_outgoing / qgcm_chain_incoming).
int run_chain(qgcm_ctx *ctx, bool outgoing, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
              const uint32_t *d_peer, qgcm_desc *d_descs, uint32_t plugins, const uint8_t *d_nonces, uint8_t *d_status,
              uint32_t *d_bytes, void *d_work, hipStream_t s) {
    if (!ctx) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    if ((stride & 3) || n > QGCM_MAX_BATCH || (plugins & ~kAllPlugins)) return QGCM_E_ARG;
    if (n && (!d_arena || !d_lens || !d_peer || !d_descs || !d_status || !d_bytes || !d_work || stride == 0))
        return QGCM_E_ARG;
    if (((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) || ((uintptr_t)d_peer & 3) || ((uintptr_t)d_descs & 15) ||
        ((uintptr_t)d_bytes & 3) || ((uintptr_t)d_work & 15))
        return QGCM_E_ARG;
    const bool gen = d_nonces == QGCM_NONCES_GENERATE;
    if (outgoing && !gen && ((uintptr_t)d_nonces & 3)) return QGCM_E_ARG;
    ChainArgs a{};
    {
        std::lock_guard<std::mutex> g(r->mu);
        if (!r->set) return QGCM_E_ARG;
        a.peer_plugins = r->d_plugins;  // never freed or moved while the context lives
    }
    if (n == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    const uint64_t lanes = chain_work_lanes(n);
    a.plugins = plugins;
    a.max_keys = ctx_max_keys(ctx);
    a.stride = stride;
    a.n = n;
    a.lens = d_lens;
    a.peer = d_peer;
    a.descs = d_descs;
    a.status = d_status;
    a.bytes = d_bytes;
    a.flags = static_cast<uint8_t *>(d_work);
    a.gate = a.flags + lanes;
    a.cstat = a.gate + lanes;
    a.sstat = a.cstat + lanes;
    const bool comp = plugins & QGCM_PLUGIN_COMPRESSION, enc = plugins & QGCM_PLUGIN_ENCRYPTION;
    // the device codec's reach: slots of stride - 4 packet bytes, at most QGCM_SNAPPY_DEVICE_MAX of them
    const uint32_t room = (uint32_t)std::min<uint64_t>(stride - 4, QGCM_SNAPPY_DEVICE_MAX);
    int rc;
    if (outgoing) {
        // a resolved packet has 4 + L + 28 <= stride; below 36 bytes of slot there is none
        const bool codec = comp && stride >= 4 + 4 + QGCM_OVERHEAD;
        rc = hip_rc(launch_chain(kChainOutPlan, enc && !codec, a, s));
        if (rc == QGCM_OK && codec)
            rc = run_snappy_gated(ctx, true, d_arena, stride, n, d_lens, room, room,
                                  (uint32_t)std::min<uint64_t>(stride - 4 - QGCM_OVERHEAD, room), a.cstat, a.gate, s);
        if (rc == QGCM_OK && enc && codec) rc = hip_rc(launch_chain(kChainOutDescs, false, a, s));
        if (rc == QGCM_OK && enc) rc = qgcm_seal_batch(ctx, d_arena, d_descs, n, d_nonces, 4, a.sstat, s);
        if (rc == QGCM_OK) rc = hip_rc(launch_chain(kChainOutFinish, false, a, s));
        return rc;
    }
    rc = QGCM_OK;
    if (enc) {
        rc = hip_rc(launch_chain(kChainInPlan, false, a, s));
        if (rc == QGCM_OK) rc = qgcm_open_batch(ctx, d_arena, d_descs, n, 4, a.sstat, s);
    }
    if (rc == QGCM_OK) rc = hip_rc(launch_chain(kChainInMid, !enc, a, s));
    if (rc == QGCM_OK && comp) {
        // stride 4 holds no packet byte: every gated packet is the empty stream, which does not decode
        if (room)
            rc = run_snappy_gated(ctx, false, d_arena, stride, n, d_lens,
                                  (uint32_t)std::min<uint64_t>(stride - 4, qgcm_snappy_max_compressed_length(QGCM_SNAPPY_DEVICE_MAX)),
                                  room, 0, a.cstat, a.gate, s);
        if (rc == QGCM_OK) rc = hip_rc(launch_chain(kChainInFinish, false, a, s));
    }
    return rc;
}

int account(qgcm_ctx *ctx, int dir, uint32_t n, const uint32_t *d_peer, const qgcm_desc *d_descs, const uint32_t *d_bytes,
            bool by_bytes, const uint8_t *d_status, hipStream_t s) {
    if (!ctx || (dir != QGCM_TX && dir != QGCM_RX) || n > QGCM_MAX_BATCH) return QGCM_E_ARG;
    if (n && (!d_peer || (by_bytes ? !d_bytes : !d_descs))) return QGCM_E_ARG;
    if (((uintptr_t)d_peer & 3) || ((uintptr_t)d_descs & 15) || ((uintptr_t)d_bytes & 3)) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    RouteAccountArgs a{};
    {
        std::lock_guard<std::mutex> g(r->mu);
        if (!r->set) return QGCM_E_ARG;
        a.counters = r->d_counters + (size_t)dir * r->dir_words;
    }
    if (n == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    a.max_keys = ctx_max_keys(ctx);
    a.dir = dir;
    a.n = n;
    a.peer = d_peer;
    a.descs = d_descs;
    a.status = d_status;
    a.bytes = by_bytes ? d_bytes : nullptr;
    return hip_rc(launch_route_account(a, ctx_num_cus(ctx), s));
}

// The copy back of the packed pipelines (include/qgcm.h "delivered packets packed on routed batches"): where
// the caller's packed area and table are, and how far they are filled.
struct PackOut {
    uint8_t *h_out;
    uint64_t out_cap;  // at most kPackMaxCap: `off` is 32 bits
    qgcm_pack_rec *h_recs;
    uint64_t *out;     // {packets fully processed, records written, bytes of h_out used}
    uint64_t fill = 0, m = 0;
    // the device area of a chunk
    qgcm_pack_rec *d_recs = nullptr;
    uint64_t *d_counts = nullptr;
    void *d_work = nullptr;
    uint8_t *d_packed = nullptr;
    uint64_t h_counts[4] = {0, 0, 0, 0};
    // the coalesced pipelines (include/qgcm.h "delivered TCP segments coalesced on routed batches"): a table of
    // super-frames in place of h_recs, out = {packets, entries, bytes, coalesced entries, delivered packets}
    qgcm_gso_frame *h_frames = nullptr;
    qgcm_gso_frame *d_frames = nullptr;
    uint64_t coalesced = 0, delivered = 0;
};

// the device area of a chunk: every record (every entry behind its lead) fits
inline uint64_t pack_area_bytes(const PackOut &pk, uint32_t cn, uint64_t stride) {
    return std::min<uint64_t>((uint64_t)cn * (((stride + 15) & ~(uint64_t)15) + (pk.h_frames ? kCoLead : 0u)), kPackMaxCap);
}

// recs (16-B aligned first), counts, the scan's work area, the packed bytes (16-B aligned)
bool pack_grow(RouteState *r, PackOut &pk, uint32_t max_cn, uint64_t stride) {
    const size_t o_counts = (pk.h_frames ? 32ull : 16ull) * max_cn, o_work = o_counts + (pk.h_frames ? 32 : 16),
                 o_packed = o_work + (size_t)(pk.h_frames ? deliver_coalesce_work_bytes(max_cn) : deliver_pack_work_bytes(max_cn));
    if (!grow(r->d_pack, r->pack_cap, o_packed + std::max<size_t>((size_t)pack_area_bytes(pk, max_cn, stride), 16))) return false;
    pk.d_recs = reinterpret_cast<qgcm_pack_rec *>(r->d_pack);
    pk.d_frames = reinterpret_cast<qgcm_gso_frame *>(r->d_pack);
    pk.d_counts = reinterpret_cast<uint64_t *>(r->d_pack + o_counts);
    pk.d_work = r->d_pack + o_work;
    pk.d_packed = r->d_pack + o_packed;
    return true;
}

// A chunk's delivered packets packed on the device, behind its chain on s; its counts come down.  QGCM_E_NOMEM
// (out written) when the chunk's bytes do not fit behind the fill position: nothing of it is accounted or copied.
int pack_chunk(PackOut &pk, const uint8_t *d_arena, uint64_t stride, uint32_t c0, uint32_t cn, const uint32_t *d_lens,
               const uint32_t *d_peer, const uint8_t *d_stat, hipStream_t s) {
    const uint64_t area = pack_area_bytes(pk, cn, stride);
    const hipError_t e = pk.h_frames ? launch_deliver_coalesce(d_arena, stride, cn, d_lens, d_peer, d_stat, pk.d_packed, area,
                                                               pk.d_frames, pk.d_counts, pk.d_work, s)
                                     : launch_deliver_pack(d_arena, stride, cn, d_lens, d_peer, d_stat, pk.d_packed, area,
                                                           pk.d_recs, pk.d_counts, pk.d_work, s);
    if (e != hipSuccess || hipMemcpyAsync(pk.h_counts, pk.d_counts, pk.h_frames ? 32 : 16, hipMemcpyDeviceToHost, s) != hipSuccess)
        return QGCM_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess || pk.h_counts[0] > cn) return QGCM_E_HIP;
    pk.out[0] = c0;
    pk.out[1] = pk.m;
    pk.out[2] = pk.fill;
    if (pk.h_frames) {
        pk.out[3] = pk.coalesced;
        pk.out[4] = pk.delivered;
    }
    // a chunk whose records did not all fit the device area (slots of more than 4 GiB) cannot be delivered
    if (pk.h_counts[1] > area || pk.fill + pk.h_counts[1] > pk.out_cap) return QGCM_E_NOMEM;
    return QGCM_OK;
}

// ... and, once the chunk is accounted, its bytes and records appended to the caller's
bool pack_copy_back(PackOut &pk, hipStream_t s) {
    const uint64_t m = pk.h_counts[0], bytes = pk.h_counts[1];
    return (!bytes || hipMemcpyAsync(pk.h_out + pk.fill, pk.d_packed, (size_t)bytes, hipMemcpyDeviceToHost, s) == hipSuccess) &&
           (!m || (pk.h_frames ? hipMemcpyAsync(pk.h_frames + pk.m, pk.d_frames, 32ull * m, hipMemcpyDeviceToHost, s)
                               : hipMemcpyAsync(pk.h_recs + pk.m, pk.d_recs, 16ull * m, hipMemcpyDeviceToHost, s)) == hipSuccess);
}

// ... and, once they have arrived, rebased: `off` by the fill position, `slot` by the chunk's first slot
void pack_rebase(PackOut &pk, uint32_t c0, uint32_t cn) {
    const uint64_t m = pk.h_counts[0];
    if (pk.fill || c0)
        for (uint64_t k = pk.m; k < pk.m + m; ++k) {
            if (pk.h_frames) {
                pk.h_frames[k].off += (uint32_t)pk.fill;
                pk.h_frames[k].first += c0;
            } else {
                pk.h_recs[k].off += (uint32_t)pk.fill;
                pk.h_recs[k].slot += c0;
            }
        }
    pk.m += m;
    pk.fill += pk.h_counts[1];
    pk.out[0] = (uint64_t)c0 + cn;
    pk.out[1] = pk.m;
    pk.out[2] = pk.fill;
    if (pk.h_frames) {
        pk.out[3] = pk.coalesced += pk.h_counts[2];
        pk.out[4] = pk.delivered += pk.h_counts[3];
    }
}

// The copy back of the packed outgoing pipeline (include/qgcm.h "planned trains packed on routed batches"): where
// the caller's packed area, table and order are, and how far they are filled.
struct TrainOut {
    uint8_t *h_out;
    uint64_t out_cap;  // at most kTrainMaxCap: `off` is 32 bits
    qgcm_ptrain *h_ptrains;
    uint32_t *h_order;  // may be NULL
    uint64_t *out;      // {packets fully processed, trains written, bytes of h_out used, datagrams in those trains}
    qgcm_plan_limits lim;
    uint64_t fill = 0, t = 0, m = 0;
    // the device area of a chunk
    qgcm_train *d_trains = nullptr;
    qgcm_ptrain *d_ptrains = nullptr;
    uint32_t *d_order = nullptr, *d_counts = nullptr;
    uint64_t *d_pcounts = nullptr;
    void *d_plan_work = nullptr, *d_work = nullptr;
    uint8_t *d_packed = nullptr;
    uint64_t plan_work_bytes = 0;
    uint32_t h_counts[2] = {0, 0};
    uint64_t h_pcounts[2] = {0, 0};
};

inline uint64_t train_area_bytes(uint32_t cn, uint64_t stride) {
    return std::min<uint64_t>((uint64_t)cn * ((stride + 15) & ~(uint64_t)15), kTrainMaxCap);
}

// trains and ptrains (16-B aligned first), order, the plan's counts, pcounts (8-B aligned), the planner's work area
// (256-B aligned), the scan's, the packed bytes (16-B aligned)
bool train_grow(RouteState *r, TrainOut &tk, uint32_t max_cn, uint64_t stride) {
    tk.plan_work_bytes = send_plan_work_bytes(max_cn);
    const size_t o_ptrains = 16ull * max_cn, o_order = o_ptrains + 16ull * max_cn, o_counts = o_order + 4ull * max_cn,
                 o_pcounts = (o_counts + 8 + 15) & ~(size_t)15, o_plan_work = (o_pcounts + 16 + 255) & ~(size_t)255,
                 o_work = (o_plan_work + (size_t)tk.plan_work_bytes + 255) & ~(size_t)255,
                 o_packed = o_work + (size_t)train_pack_work_bytes(max_cn);
    if (!grow(r->d_train, r->train_cap, o_packed + std::max<size_t>((size_t)train_area_bytes(max_cn, stride), 16))) return false;
    tk.d_trains = reinterpret_cast<qgcm_train *>(r->d_train);
    tk.d_ptrains = reinterpret_cast<qgcm_ptrain *>(r->d_train + o_ptrains);
    tk.d_order = reinterpret_cast<uint32_t *>(r->d_train + o_order);
    tk.d_counts = reinterpret_cast<uint32_t *>(r->d_train + o_counts);
    tk.d_pcounts = reinterpret_cast<uint64_t *>(r->d_train + o_pcounts);
    tk.d_plan_work = r->d_train + o_plan_work;
    tk.d_work = r->d_train + o_work;
    tk.d_packed = r->d_train + o_packed;
    return true;
}

// A chunk's sealed datagrams planned and packed on the device, behind its chain on s; the counts of both come
// down.  QGCM_E_NOMEM (out written) when the chunk's bytes do not fit behind the fill position: nothing of it is
// accounted or copied.
int train_chunk(TrainOut &tk, uint32_t max_keys, const uint8_t *d_arena, uint64_t stride, uint32_t c0, uint32_t cn,
                const uint32_t *d_lens, const uint32_t *d_peer, hipStream_t s) {
    if (launch_send_plan(cn, max_keys, d_lens, d_peer, tk.lim, tk.d_order, tk.d_trains, tk.d_counts, tk.d_plan_work,
                         tk.plan_work_bytes, s) != hipSuccess ||
        launch_train_pack(d_arena, stride, cn, tk.d_order, tk.d_trains, tk.d_counts, tk.d_packed, train_area_bytes(cn, stride),
                          tk.d_ptrains, tk.d_pcounts, tk.d_work, s) != hipSuccess ||
        hipMemcpyAsync(tk.h_counts, tk.d_counts, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(tk.h_pcounts, tk.d_pcounts, 16, hipMemcpyDeviceToHost, s) != hipSuccess)
        return QGCM_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess || tk.h_counts[0] > cn || tk.h_counts[1] > tk.h_counts[0] ||
        tk.h_pcounts[0] != tk.h_counts[1])
        return QGCM_E_HIP;
    tk.out[0] = c0;
    tk.out[1] = tk.t;
    tk.out[2] = tk.fill;
    tk.out[3] = tk.m;
    // a chunk whose trains did not all fit the device area (slots of more than 4 GiB) cannot be sent
    if (tk.h_pcounts[1] > train_area_bytes(cn, stride) || tk.fill + tk.h_pcounts[1] > tk.out_cap) return QGCM_E_NOMEM;
    return QGCM_OK;
}

// ... and, once the chunk is accounted, its bytes, table and order appended to the caller's
bool train_copy_back(TrainOut &tk, hipStream_t s) {
    const uint64_t m = tk.h_counts[0], t = tk.h_counts[1], bytes = tk.h_pcounts[1];
    return (!bytes || hipMemcpyAsync(tk.h_out + tk.fill, tk.d_packed, (size_t)bytes, hipMemcpyDeviceToHost, s) == hipSuccess) &&
           (!t || hipMemcpyAsync(tk.h_ptrains + tk.t, tk.d_ptrains, 16ull * t, hipMemcpyDeviceToHost, s) == hipSuccess) &&
           (!m || !tk.h_order || hipMemcpyAsync(tk.h_order + tk.m, tk.d_order, 4ull * m, hipMemcpyDeviceToHost, s) == hipSuccess);
}

// ... and, once they have arrived, rebased: `off` by the fill position, the order by the chunk's first slot
void train_rebase(TrainOut &tk, uint32_t c0, uint32_t cn) {
    const uint64_t m = tk.h_counts[0], t = tk.h_counts[1];
    if (tk.fill)
        for (uint64_t j = tk.t; j < tk.t + t; ++j) tk.h_ptrains[j].off += (uint32_t)tk.fill;
    if (c0 && tk.h_order)
        for (uint64_t p = tk.m; p < tk.m + m; ++p) tk.h_order[p] += c0;
    tk.t += t;
    tk.m += m;
    tk.fill += tk.h_pcounts[1];
    tk.out[0] = (uint64_t)c0 + cn;
    tk.out[1] = tk.t;
    tk.out[2] = tk.fill;
    tk.out[3] = tk.m;
}

// The PackOut of a packed call (h_table: qgcm_pack_rec) or a coalesced one (qgcm_gso_frame), its `out` zeroed;
// false: an argument is missing.
bool pack_out(PackOut &pk, bool coalesced, uint32_t n, uint8_t *h_out, uint64_t out_cap, void *h_table, uint64_t *out) {
    if (!out || (n && (!h_out || !h_table))) return false;
    std::fill(out, out + (coalesced ? 5 : 3), 0);
    pk = PackOut{h_out, std::min<uint64_t>(out_cap, kPackMaxCap), coalesced ? nullptr : static_cast<qgcm_pack_rec *>(h_table), out};
    if (coalesced) pk.h_frames = static_cast<qgcm_gso_frame *>(h_table);
    return true;
}

// The TrainOut of a packed outgoing call, its `out` zeroed; false: an argument is missing or the limits are invalid.
bool train_out(TrainOut &tk, uint32_t n, uint8_t *h_out, uint64_t out_cap, qgcm_ptrain *h_ptrains, uint32_t *h_order,
               const qgcm_plan_limits *limits, uint64_t *out) {
    if (!out || (n && (!h_out || !h_ptrains))) return false;
    std::fill(out, out + 4, 0);
    tk = TrainOut{h_out, std::min<uint64_t>(out_cap, kTrainMaxCap), h_ptrains, h_order, out};
    return plan_limits_resolve(limits, &tk.lim);
}

// The routed host pipelines: Outgoing.pipeline / Incoming.pipeline for a batch in host memory, in chunks of at
// most kRouteChunk packets and kRouteChunkBytes of slots, on one stream.  Four front ends, one per form the batch
// arrives in -- slots (run_route_host), coalesced buffers (run_route_gro_host), packed frames
// (run_route_frames_host), super-frames (run_route_gso_host) -- differ in how they cut the chunks and in what goes
// up.  Each reads: its checks, pipe_enter, the chunks cut, chunk_grow (and stage_grow), then per chunk the table
// rebased, the copy in, the resolve, and chunk_tail for everything behind it.

// What a pipeline holds from pipe_enter on: the pipeline lock, the routed stream, the most slots a chunk takes.
struct Pipe {
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    uint32_t limit = 0;
};

// the routed stream, made by the first call that needs it (under pipe_mu); NULL when it cannot be made
hipStream_t pipe_stream(RouteState *r) {
    if (!r->stream && hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) r->stream = nullptr;
    return r->stream;
}

// The entry of a pipeline, behind the front end's own argument and table checks: the routes are set; for n == 0
// that is all (QGCM_OK: the caller returns it); else the pipeline lock, the device, the stream, the chunk limit.
int pipe_enter(qgcm_ctx *ctx, uint64_t stride, uint32_t n, Pipe &p) {
    RouteState *r = ctx_route(ctx);
    {
        std::lock_guard<std::mutex> g(r->mu);
        if (!r->set) return QGCM_E_ARG;
    }
    if (n == 0) return QGCM_OK;
    p.lock = std::unique_lock<std::mutex>(r->pipe_mu);
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess || !(p.s = pipe_stream(r))) return QGCM_E_HIP;
    p.limit = (uint32_t)std::min<uint64_t>(kRouteChunk, std::max<uint64_t>(1, kRouteChunkBytes / stride));
    return QGCM_OK;
}

// The side buffer of a chunk, in r->d_side: descriptors (16-B aligned first), lengths, peers, nonces, statuses;
// with the chain its byte counts and its work area (16-B aligned) behind them.  One layout for every pipeline:
// the coalesced-receive ones, which seal nothing, leave the nonces unused.
struct Side {
    qgcm_desc *d_descs;
    uint32_t *d_lens, *d_peer;
    uint8_t *d_non, *d_stat;
    uint32_t *d_bytes;  // NULL without the chain, as d_work
    void *d_work;
};

// The device areas of a call whose chunks have at most max_cn slots: the arena, the side buffer (laid out here and
// nowhere else), the statuses' host copy, and the areas of `pk` / `tk`.
bool chunk_grow(RouteState *r, Side &sd, uint32_t max_cn, uint64_t stride, bool chain, PackOut *pk, TrainOut *tk) {
    const size_t o_desc = 0, o_lens = o_desc + 16ull * max_cn, o_peer = o_lens + 4ull * max_cn, o_non = o_peer + 4ull * max_cn,
                 o_stat = o_non + 12ull * max_cn, o_bytes = (o_stat + max_cn + 15) & ~(size_t)15,
                 o_work = o_bytes + 4 * (size_t)chain_work_lanes(max_cn),
                 side = chain ? o_work + QGCM_CHAIN_WORK(max_cn) : o_stat + max_cn;
    if (!grow(r->d_arena, r->arena_cap, (size_t)max_cn * stride) || !grow(r->d_side, r->side_cap, side) ||
        (pk && !pack_grow(r, *pk, max_cn, stride)) || (tk && !train_grow(r, *tk, max_cn, stride)))
        return false;
    r->h_stat.resize(max_cn);
    uint8_t *d = r->d_side;
    sd = Side{reinterpret_cast<qgcm_desc *>(d + o_desc), reinterpret_cast<uint32_t *>(d + o_lens),
              reinterpret_cast<uint32_t *>(d + o_peer), d + o_non, d + o_stat,
              chain ? reinterpret_cast<uint32_t *>(d + o_bytes) : nullptr, chain ? d + o_work : nullptr};
    return true;
}

// The ingest staging of a call whose batch arrives packed, in r->d_stage: a chunk's table of at most max_entries
// entries (16-B aligned first), then its span of at most max_span packed bytes (16-B aligned, rounded up to 16 B);
// the table's host copy, where the front end rebases it, in r->h_stage.
template <typename T>
bool stage_grow(RouteState *r, uint32_t max_entries, uint64_t max_span, T *&h_tab, T *&d_tab, uint8_t *&d_packed) {
    const size_t table = sizeof(T) * (size_t)max_entries, o_packed = (table + 15) & ~(size_t)15;
    if (!grow(r->d_stage, r->stage_cap, std::max<size_t>(o_packed + (size_t)((max_span + 15) & ~(uint64_t)15), 16))) return false;
    r->h_stage.resize(table);
    h_tab = reinterpret_cast<T *>(r->h_stage.data());
    d_tab = reinterpret_cast<T *>(r->d_stage);
    d_packed = r->d_stage + o_packed;
    return true;
}

// A chunk that ends at a table-entry boundary: entries [e0, e1), slots [c0, c0 + cn), packed bytes [lo, hi).
struct Chunk {
    uint32_t e0, e1, c0, cn;
    uint64_t lo, hi;
};

// ... and the chunks of a call, with what sizes the device areas
struct Chunks {
    std::vector<Chunk> v;
    uint32_t max_cn = 0, max_entries = 0;
    uint64_t max_span = 0;
    void add(Chunk c) {
        if (c.lo > c.hi) c.lo = c.hi = 0;  // no entry of it has bytes that go up
        max_cn = std::max(max_cn, c.cn);
        max_entries = std::max(max_entries, c.e1 - c.e0);
        max_span = std::max(max_span, c.hi - c.lo);
        v.push_back(c);
    }
};

// What the chunks of one call share behind their resolve.
struct Job {
    qgcm_ctx *ctx;
    hipStream_t s;
    bool seal, chain;
    uint32_t plugins;  // of the chain
    uint64_t stride;
    uint32_t *h_lens, *h_peer;
    uint8_t *h_status;  // may be NULL
    bool lens_back;     // the lengths come down: the chain's are final on the device (the tables of include/qgcm.h),
                        // and an ingest kernel's exist nowhere else
    PackOut *pk;        // the incoming chain only: the copy back is the packed one, the arena stays on the device
    TrainOut *tk;       // the outgoing chain only: the same for the planned trains
    int dropped = 0;
};

// A chunk from "arena, lengths, peers and descriptors are resolved on the device" (rc: how the front end's copy in
// and resolve went) to "the host outputs are final": seal or open (chain: the plugin chain, then with `pk` / `tk`
// the pack or the plan and train pack, whose counts are waited for before the chunk is accounted) -> account ->
// copy back (h_dst: where the arena goes, unused with `pk` / `tk`) -> wait -> rebase -> statuses and lengths.
// `nonces` is on the device, QGCM_NONCES_GENERATE or NULL.
int chunk_tail(Job &j, const Side &sd, int rc, uint32_t c0, uint32_t cn, const uint8_t *nonces, uint8_t *h_dst) {
    RouteState *r = ctx_route(j.ctx);
    hipStream_t s = j.s;
    const int dir = j.seal ? QGCM_TX : QGCM_RX;
    if (rc == QGCM_OK && j.chain) {
        rc = run_chain(j.ctx, j.seal, r->d_arena, j.stride, cn, sd.d_lens, sd.d_peer, sd.d_descs, j.plugins, nonces, sd.d_stat,
                       sd.d_bytes, sd.d_work, s);
        if (rc == QGCM_OK && j.pk) rc = pack_chunk(*j.pk, r->d_arena, j.stride, c0, cn, sd.d_lens, sd.d_peer, sd.d_stat, s);
        if (rc == QGCM_OK && j.tk)
            rc = train_chunk(*j.tk, ctx_max_keys(j.ctx), r->d_arena, j.stride, c0, cn, sd.d_lens, sd.d_peer, s);
        if (rc == QGCM_OK) rc = account(j.ctx, dir, cn, sd.d_peer, nullptr, sd.d_bytes, true, sd.d_stat, s);
    } else if (rc == QGCM_OK) {
        rc = j.seal ? qgcm_seal_batch(j.ctx, r->d_arena, sd.d_descs, cn, nonces, 4, sd.d_stat, s)
                    : qgcm_open_batch(j.ctx, r->d_arena, sd.d_descs, cn, 4, sd.d_stat, s);
        if (rc == QGCM_OK) rc = qgcm_route_account(j.ctx, dir, cn, sd.d_peer, sd.d_descs, sd.d_stat, s);
    }
    if (rc == QGCM_OK &&
        ((j.pk   ? !pack_copy_back(*j.pk, s)
          : j.tk ? !train_copy_back(*j.tk, s)
                 : hipMemcpyAsync(h_dst, r->d_arena, (size_t)cn * j.stride, hipMemcpyDeviceToHost, s) != hipSuccess) ||
         hipMemcpyAsync(j.h_peer + c0, sd.d_peer, 4ull * cn, hipMemcpyDeviceToHost, s) != hipSuccess ||
         hipMemcpyAsync(r->h_stat.data(), sd.d_stat, cn, hipMemcpyDeviceToHost, s) != hipSuccess ||
         (j.lens_back && hipMemcpyAsync(j.h_lens + c0, sd.d_lens, 4ull * cn, hipMemcpyDeviceToHost, s) != hipSuccess)))
        rc = QGCM_E_HIP;
    // every way out waits for the stream: the next call reuses the staging, and the caller its arrays
    if (hipStreamSynchronize(s) != hipSuccess && rc == QGCM_OK) rc = QGCM_E_HIP;
    if (rc != QGCM_OK) return rc;
    if (j.pk) pack_rebase(*j.pk, c0, cn);
    if (j.tk) train_rebase(*j.tk, c0, cn);
    for (uint32_t i = 0; i < cn; ++i) {
        const bool ok = r->h_stat[i] == 1;
        if (!j.chain) {
            // from the length that went in (the caller's, or the datagram's that came down from an ingest kernel).
            // Sealed: the datagram Raw[:4 + L + 28]; opened: the plaintext packet qgcm_tun_write_slots takes
            const uint32_t len = j.h_lens[c0 + i];
            j.h_lens[c0 + i] = !ok ? 0 : j.seal ? 4 + len + QGCM_OVERHEAD : len - 4 - QGCM_OVERHEAD;
        }
        if (j.h_status) j.h_status[c0 + i] = ok ? 1 : 0;
        j.dropped += !ok;
    }
    return QGCM_OK;
}

// The batch in slots of the caller's arena: chunks of a fixed number of slots; a chunk's slots, lengths and (seal,
// the caller's) nonces go up and the resolve kernel resolves them.
int run_route_host(qgcm_ctx *ctx, bool seal, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                   const uint8_t *h_nonces, uint32_t *h_peer, uint8_t *h_status, bool chain = false,
                   uint32_t plugins = 0, PackOut *pk = nullptr, TrainOut *tk = nullptr) {
    if (!ctx) return QGCM_E_ARG;
    if ((stride & 3) || n > QGCM_MAX_BATCH) return QGCM_E_ARG;
    if (n && (!h_arena || !h_lens || !h_peer || stride == 0)) return QGCM_E_ARG;
    if (chain && (plugins & ~kAllPlugins)) return QGCM_E_ARG;
    Pipe p;
    int rc = pipe_enter(ctx, stride, n, p);
    if (rc != QGCM_OK || n == 0) return rc;
    RouteState *r = ctx_route(ctx);
    const bool gen = seal && h_nonces == QGCM_NONCES_GENERATE, non = seal && h_nonces && !gen;
    const uint32_t chunk = std::min(p.limit, n);
    Side sd;
    if (!chunk_grow(r, sd, chunk, stride, chain, pk, tk)) return QGCM_E_NOMEM;
    Job job{ctx, p.s, seal, chain, plugins, stride, h_lens, h_peer, h_status, chain, pk, tk};
    for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t cn = std::min(chunk, n - c0);
        uint8_t *h = h_arena + (uint64_t)c0 * stride;
        const bool up = hipMemcpyAsync(r->d_arena, h, (size_t)cn * stride, hipMemcpyHostToDevice, p.s) == hipSuccess &&
                        hipMemcpyAsync(sd.d_lens, h_lens + c0, 4ull * cn, hipMemcpyHostToDevice, p.s) == hipSuccess &&
                        (!non || hipMemcpyAsync(sd.d_non, h_nonces + 12ull * c0, 12ull * cn, hipMemcpyHostToDevice, p.s) == hipSuccess);
        rc = up ? resolve(ctx, seal, r->d_arena, stride, cn, sd.d_lens, sd.d_peer, sd.d_descs, p.s) : QGCM_E_HIP;
        rc = chunk_tail(job, sd, rc, c0, cn, gen ? QGCM_NONCES_GENERATE : non ? sd.d_non : nullptr, h);
        if (rc != QGCM_OK) return rc;
    }
    return job.dropped;
}

// The batch in coalesced buffers (qgcm_udp_recv_gro), incoming only.  Chunks end at buffer boundaries, and lo is
// aligned down to 16 B.  Per chunk the packed bytes its buffers span and their table entries (rebased to the span
// and to the chunk's first slot) go up; gro_unpack_kernel scatters them into the device arena and the resolve
// kernel resolves them (QGCM_GRO_FUSED=1: gro_resolve_kernel does both).  The lengths start as zeros on the
// device, so the slots of a buffer the kernel skips (one past packed_len) are datagrams of length 0.
int run_route_gro_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_gro_buf *bufs,
                       uint32_t n_bufs, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens, uint32_t *h_peer,
                       uint8_t *h_status, bool chain, uint32_t plugins, PackOut *pk = nullptr) {
    if (!ctx) return QGCM_E_ARG;
    if ((stride & 3) || n > QGCM_MAX_BATCH || n_bufs > n) return QGCM_E_ARG;
    if (n && (!h_packed || !bufs || (!h_arena && !pk) || !h_lens || !h_peer || stride == 0)) return QGCM_E_ARG;
    if (chain && (plugins & ~kAllPlugins)) return QGCM_E_ARG;
    if (!gro_table_ok(bufs, n_bufs, n)) return QGCM_E_ARG;
    Pipe p;
    int rc = pipe_enter(ctx, stride, n, p);
    if (rc != QGCM_OK || n == 0) return rc;
    RouteState *r = ctx_route(ctx);
    Chunks chunks;
    for (uint32_t b = 0; b < n_bufs;) {
        Chunk c{b, b, bufs[b].first, 0, UINT64_MAX, 0};
        for (; b < n_bufs; ++b) {
            const uint32_t count = (uint32_t)gro_count(bufs[b].len, bufs[b].seg_len);  // at most n: the table is checked
            if (c.cn && (uint64_t)c.cn + count > p.limit) break;
            c.cn += count;
            if ((uint64_t)bufs[b].off + bufs[b].len > packed_len) continue;  // skipped by the kernel: none of its bytes go up
            c.lo = std::min<uint64_t>(c.lo, bufs[b].off & ~15u);
            c.hi = std::max<uint64_t>(c.hi, (uint64_t)bufs[b].off + bufs[b].len);
        }
        c.e1 = b;
        chunks.add(c);
    }
    Side sd;
    qgcm_gro_buf *h_bufs, *d_bufs;
    uint8_t *d_packed;
    if (!chunk_grow(r, sd, chunks.max_cn, stride, chain, pk, nullptr) ||
        !stage_grow(r, chunks.max_entries, chunks.max_span, h_bufs, d_bufs, d_packed))
        return QGCM_E_NOMEM;
    Job job{ctx, p.s, false, chain, plugins, stride, h_lens, h_peer, h_status, true, pk, nullptr};
    for (const Chunk &c : chunks.v) {
        const uint32_t nb = c.e1 - c.e0;
        for (uint32_t j = 0; j < nb; ++j) {
            const qgcm_gro_buf &b = bufs[c.e0 + j];
            const bool past = (uint64_t)b.off + b.len > packed_len;
            // a buffer past packed_len stays one the kernel skips: its one entry keeps the search over `first` whole
            h_bufs[j] = past ? qgcm_gro_buf{0xffffffffu, 1, 0, b.first - c.c0}
                             : qgcm_gro_buf{(uint32_t)(b.off - c.lo), b.len, b.seg_len, b.first - c.c0};
        }
        const size_t span = (size_t)(c.hi - c.lo);
        const bool up = hipMemsetAsync(sd.d_lens, 0, 4ull * c.cn, p.s) == hipSuccess &&
                        (!span || hipMemcpyAsync(d_packed, h_packed + c.lo, span, hipMemcpyHostToDevice, p.s) == hipSuccess) &&
                        hipMemcpyAsync(d_bufs, h_bufs, 16ull * nb, hipMemcpyHostToDevice, p.s) == hipSuccess;
        if (!up) {
            rc = QGCM_E_HIP;
        } else if (r->gro_fused) {
            rc = gro_resolve(ctx, d_packed, span, d_bufs, nb, c.cn, r->d_arena, stride, sd.d_lens, sd.d_peer, sd.d_descs, p.s);
        } else {
            rc = hip_rc(launch_gro_unpack(d_packed, span, d_bufs, nb, c.cn, r->d_arena, stride, sd.d_lens, p.s));
            if (rc == QGCM_OK) rc = resolve(ctx, false, r->d_arena, stride, c.cn, sd.d_lens, sd.d_peer, sd.d_descs, p.s);
        }
        rc = chunk_tail(job, sd, rc, c.c0, c.cn, nullptr, pk ? nullptr : h_arena + (uint64_t)c.c0 * stride);
        if (rc != QGCM_OK) return rc;
    }
    return job.dropped;
}

// The batch read packed (qgcm_tun_read_packed), the packed outgoing chain only.  Frame i is slot i, so the chunks
// are run_route_host's.  Per chunk the packed bytes its frames span (the table ascends: from the first frame's off
// to the last frame's end) and their table entries (rebased to the span) go up, and frames_resolve_kernel puts
// them into the device arena and resolves them.
int run_route_frames_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_frame *frames, uint64_t stride,
                          uint32_t n, uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins, uint32_t *h_peer,
                          uint8_t *h_status, TrainOut &tk) {
    if (!ctx) return QGCM_E_ARG;
    if ((stride & 3) || stride < 8 || n > QGCM_MAX_BATCH || !h_nonces || (plugins & ~kAllPlugins)) return QGCM_E_ARG;
    if (n && (!h_packed || !frames || !h_lens || !h_peer)) return QGCM_E_ARG;
    if (!frames_table_ascends(frames, n, packed_len)) return QGCM_E_ARG;
    Pipe p;
    int rc = pipe_enter(ctx, stride, n, p);
    if (rc != QGCM_OK || n == 0) return rc;
    RouteState *r = ctx_route(ctx);
    const bool gen = h_nonces == QGCM_NONCES_GENERATE;
    const uint32_t chunk = std::min(p.limit, n);
    // the longest span of a chunk's frames
    uint64_t max_span = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
        const qgcm_frame &last = frames[c0 + std::min(chunk, n - c0) - 1];
        max_span = std::max<uint64_t>(max_span, (uint64_t)last.off + last.len - frames[c0].off);
    }
    Side sd;
    qgcm_frame *h_frames, *d_frames;
    uint8_t *d_packed;
    if (!chunk_grow(r, sd, chunk, stride, true, nullptr, &tk) || !stage_grow(r, chunk, max_span, h_frames, d_frames, d_packed))
        return QGCM_E_NOMEM;
    Job job{ctx, p.s, true, true, plugins, stride, h_lens, h_peer, h_status, true, nullptr, &tk};
    for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t cn = std::min(chunk, n - c0);
        const uint64_t lo = frames[c0].off, hi = (uint64_t)frames[c0 + cn - 1].off + frames[c0 + cn - 1].len;
        for (uint32_t j = 0; j < cn; ++j) h_frames[j] = qgcm_frame{(uint32_t)(frames[c0 + j].off - lo), frames[c0 + j].len};
        const bool up = (hi == lo || hipMemcpyAsync(d_packed, h_packed + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, p.s) == hipSuccess) &&
                        hipMemcpyAsync(d_frames, h_frames, 8ull * cn, hipMemcpyHostToDevice, p.s) == hipSuccess &&
                        (gen || hipMemcpyAsync(sd.d_non, h_nonces + 12ull * c0, 12ull * cn, hipMemcpyHostToDevice, p.s) == hipSuccess);
        rc = up ? frames_resolve(ctx, d_packed, hi - lo, d_frames, cn, r->d_arena, stride, sd.d_lens, sd.d_peer, sd.d_descs, p.s)
                : QGCM_E_HIP;
        rc = chunk_tail(job, sd, rc, c0, cn, gen ? QGCM_NONCES_GENERATE : sd.d_non, nullptr);
        if (rc != QGCM_OK) return rc;
    }
    return job.dropped;
}

// The batch read as super-frames (qgcm_tun_read_gso), the packed outgoing chain only.  An entry names a run of
// slots, so chunks end at entry boundaries; every entry is valid (the table is checked), so lo, a 16-B boundary, is
// the least off and hi the greatest end.  Per chunk the span and the entries (rebased to the span and to the
// chunk's first slot) go up, and gso_resolve_kernel segments them into the device arena and resolves them.
int run_route_gso_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_gso_frame *frames, uint32_t n_frames,
                       uint64_t stride, uint32_t n, uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins, uint32_t *h_peer,
                       uint8_t *h_status, TrainOut &tk) {
    if (!ctx) return QGCM_E_ARG;
    if ((stride & 3) || stride < 8 || n > QGCM_MAX_BATCH || n_frames > n || !h_nonces || (plugins & ~kAllPlugins)) return QGCM_E_ARG;
    if (n && (!h_packed || !frames || !h_lens || !h_peer)) return QGCM_E_ARG;
    if (!gso_table_ok(frames, n_frames, n, packed_len)) return QGCM_E_ARG;
    Pipe p;
    int rc = pipe_enter(ctx, stride, n, p);
    if (rc != QGCM_OK || n == 0) return rc;
    RouteState *r = ctx_route(ctx);
    const bool gen = h_nonces == QGCM_NONCES_GENERATE;
    Chunks chunks;
    for (uint32_t e = 0; e < n_frames;) {
        Chunk c{e, e, frames[e].first, 0, UINT64_MAX, 0};
        for (; e < n_frames; ++e) {
            if (c.cn && (uint64_t)c.cn + frames[e].count > p.limit) break;
            c.cn += frames[e].count;
            c.lo = std::min<uint64_t>(c.lo, frames[e].off);
            c.hi = std::max<uint64_t>(c.hi, (uint64_t)frames[e].off + frames[e].len);
        }
        c.e1 = e;
        chunks.add(c);
    }
    Side sd;
    qgcm_gso_frame *h_frames, *d_frames;
    uint8_t *d_packed;
    if (!chunk_grow(r, sd, chunks.max_cn, stride, true, nullptr, &tk) ||
        !stage_grow(r, chunks.max_entries, chunks.max_span, h_frames, d_frames, d_packed))
        return QGCM_E_NOMEM;
    Job job{ctx, p.s, true, true, plugins, stride, h_lens, h_peer, h_status, true, nullptr, &tk};
    for (const Chunk &c : chunks.v) {
        const uint32_t ne = c.e1 - c.e0;
        for (uint32_t j = 0; j < ne; ++j) {
            h_frames[j] = frames[c.e0 + j];
            h_frames[j].off -= (uint32_t)c.lo;
            h_frames[j].first -= c.c0;
        }
        const size_t span = (size_t)(c.hi - c.lo);
        const bool up = (!span || hipMemcpyAsync(d_packed, h_packed + c.lo, span, hipMemcpyHostToDevice, p.s) == hipSuccess) &&
                        hipMemcpyAsync(d_frames, h_frames, 32ull * ne, hipMemcpyHostToDevice, p.s) == hipSuccess &&
                        (gen || hipMemcpyAsync(sd.d_non, h_nonces + 12ull * c.c0, 12ull * c.cn, hipMemcpyHostToDevice, p.s) == hipSuccess);
        rc = up ? gso_resolve(ctx, d_packed, span, d_frames, ne, c.cn, r->d_arena, stride, sd.d_lens, sd.d_peer, sd.d_descs, p.s)
                : QGCM_E_HIP;
        rc = chunk_tail(job, sd, rc, c.c0, c.cn, gen ? QGCM_NONCES_GENERATE : sd.d_non, nullptr);
        if (rc != QGCM_OK) return rc;
    }
    return job.dropped;
}

}  // namespace

extern "C" {

int qgcm_routes_set(qgcm_ctx *ctx, const qgcm_route *routes, uint32_t count, const qgcm_route_net *net) {
    if (!ctx || !net || (count && !routes) || count > (1u << 30)) return QGCM_E_ARG;
    const uint32_t max_keys = ctx_max_keys(ctx);
    for (uint32_t i = 0; i < count; ++i)
        if (routes[i].peer >= max_keys) return QGCM_E_ARG;
    uint32_t cap = 2;
    while (cap < 2ull * count) cap <<= 1;
    std::vector<qgcm_route> table(cap, qgcm_route{0, QGCM_NO_PEER});
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t h = route_hash(routes[i].ip) & (cap - 1);
        while (table[h].peer != QGCM_NO_PEER && table[h].ip != routes[i].ip) h = (h + 1) & (cap - 1);
        table[h] = routes[i];  // a duplicate ip takes the last entry, as a map assignment does
    }
    RouteState *r = ctx_route(ctx);
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    uint2 *fresh = nullptr, *old = nullptr;
    if (hipMalloc(&fresh, (size_t)cap * 8) != hipSuccess) return QGCM_E_NOMEM;
    if (hipMemcpy(fresh, table.data(), (size_t)cap * 8, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(fresh);
        return QGCM_E_HIP;
    }
    {
        std::lock_guard<std::mutex> g(r->mu);
        if (!r->d_counters) {
            const size_t words = 4 * (1 + (size_t)max_keys);
            if (hipMalloc(&r->d_counters, 2 * words * 8) != hipSuccess ||
                hipMemset(r->d_counters, 0, 2 * words * 8) != hipSuccess) {
                hipFree(r->d_counters);
                r->d_counters = nullptr;
                hipFree(fresh);
                return QGCM_E_NOMEM;
            }
            r->dir_words = words;
        }
        old = r->d_table;
        r->d_table = fresh;
        r->cap_mask = cap - 1;
        r->net = *net;
        r->set = true;
    }
    if (old) hipFree(old);  // waits for the device: the launches that took `old` are done
    return QGCM_OK;
}

int qgcm_resolve_outgoing(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                          uint32_t *d_peer, qgcm_desc *d_descs, void *stream) {
    return resolve(ctx, true, d_arena, stride, n, d_lens, d_peer, d_descs, (hipStream_t)stream);
}

int qgcm_resolve_incoming(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                          uint32_t *d_peer, qgcm_desc *d_descs, void *stream) {
    return resolve(ctx, false, const_cast<uint8_t *>(d_arena), stride, n, d_lens, d_peer, d_descs, (hipStream_t)stream);
}

int qgcm_route_account(qgcm_ctx *ctx, int dir, uint32_t n, const uint32_t *d_peer, const qgcm_desc *d_descs,
                       const uint8_t *d_status, void *stream) {
    return account(ctx, dir, n, d_peer, d_descs, nullptr, false, d_status, (hipStream_t)stream);
}

int qgcm_route_account_bytes(qgcm_ctx *ctx, int dir, uint32_t n, const uint32_t *d_peer, const uint32_t *d_bytes,
                             const uint8_t *d_status, void *stream) {
    return account(ctx, dir, n, d_peer, nullptr, d_bytes, true, d_status, (hipStream_t)stream);
}

int qgcm_peer_plugins_set(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t *flags) {
    if (!ctx || (count && !flags)) return QGCM_E_ARG;
    const uint32_t max_keys = ctx_max_keys(ctx);
    if ((uint64_t)first_idx + count > max_keys) return QGCM_E_ARG;
    for (uint32_t i = 0; i < count; ++i)
        if (flags[i] & ~kAllPlugins) return QGCM_E_ARG;
    if (count == 0) return QGCM_OK;
    RouteState *r = ctx_route(ctx);
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->d_plugins) {
        uint8_t *fresh = nullptr;
        if (hipMalloc(&fresh, max_keys) != hipSuccess) return QGCM_E_NOMEM;
        if (hipMemset(fresh, QGCM_PLUGIN_ENCRYPTION, max_keys) != hipSuccess) {
            hipFree(fresh);
            return QGCM_E_HIP;
        }
        r->d_plugins = fresh;
    }
    // a batch in flight reads each packet's byte once (chain_kernels.hip): it sees the old or the new value
    return hip_rc(hipMemcpy(r->d_plugins + first_idx, flags, count, hipMemcpyHostToDevice));
}

int qgcm_peer_plugins_get(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, uint8_t *flags) {
    if (!ctx || (count && !flags)) return QGCM_E_ARG;
    if ((uint64_t)first_idx + count > ctx_max_keys(ctx)) return QGCM_E_ARG;
    if (count == 0) return QGCM_OK;
    RouteState *r = ctx_route(ctx);
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->d_plugins) {
        memset(flags, QGCM_PLUGIN_ENCRYPTION, count);
        return QGCM_OK;
    }
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    return hip_rc(hipMemcpy(flags, r->d_plugins + first_idx, count, hipMemcpyDeviceToHost));
}

int qgcm_chain_outgoing(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                        const uint32_t *d_peer, qgcm_desc *d_descs, uint32_t plugins, const uint8_t *d_nonces,
                        uint8_t *d_status, uint32_t *d_bytes, void *d_work, void *stream) {
    return run_chain(ctx, true, d_arena, stride, n, d_lens, d_peer, d_descs, plugins, d_nonces, d_status, d_bytes, d_work,
                     (hipStream_t)stream);
}

int qgcm_chain_incoming(qgcm_ctx *ctx, uint8_t *d_arena, uint64_t stride, uint32_t n, uint32_t *d_lens,
                        const uint32_t *d_peer, qgcm_desc *d_descs, uint32_t plugins, uint8_t *d_status,
                        uint32_t *d_bytes, void *d_work, void *stream) {
    return run_chain(ctx, false, d_arena, stride, n, d_lens, d_peer, d_descs, plugins, nullptr, d_status, d_bytes, d_work,
                     (hipStream_t)stream);
}

uint64_t qgcm_send_plan_work(uint32_t n) { return n > QGCM_MAX_BATCH ? 0 : send_plan_work_bytes(n); }

int qgcm_send_plan(qgcm_ctx *ctx, uint32_t n, const uint32_t *d_lens, const uint32_t *d_peer,
                   const qgcm_plan_limits *limits, uint32_t *d_order, qgcm_train *d_trains, uint32_t *d_counts,
                   void *d_work, void *stream) {
    if (!ctx || n > QGCM_MAX_BATCH) return QGCM_E_ARG;
    if (n && (!d_lens || !d_peer || !d_order || !d_trains || !d_counts || !d_work)) return QGCM_E_ARG;
    if (((uintptr_t)d_lens & 3) || ((uintptr_t)d_peer & 3) || ((uintptr_t)d_order & 3) || ((uintptr_t)d_trains & 15) ||
        ((uintptr_t)d_counts & 3) || ((uintptr_t)d_work & 255))
        return QGCM_E_ARG;
    qgcm_plan_limits lim;
    if (!plan_limits_resolve(limits, &lim)) return QGCM_E_ARG;
    if (n == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    // the area is the size the caller was told (the one size query of the call)
    return hip_rc(launch_send_plan(n, ctx_max_keys(ctx), d_lens, d_peer, lim, d_order, d_trains, d_counts, d_work,
                                   send_plan_work_bytes(n), (hipStream_t)stream));
}

int qgcm_send_plan_cpu(uint32_t n, const uint32_t *lens, const uint32_t *peer, uint32_t max_keys,
                       const qgcm_plan_limits *limits, uint32_t *order, qgcm_train *trains, uint32_t counts[2]) {
    if (n > QGCM_MAX_BATCH || !counts || (n && (!lens || !peer || !order || !trains))) return QGCM_E_ARG;
    qgcm_plan_limits lim;
    if (!plan_limits_resolve(limits, &lim)) return QGCM_E_ARG;
    send_plan_cpu(n, lens, peer, max_keys, lim, order, trains, counts);
    return QGCM_OK;
}

int qgcm_send_plan_host(qgcm_ctx *ctx, uint32_t n, const uint32_t *h_lens, const uint32_t *h_peer,
                        const qgcm_plan_limits *limits, uint32_t *h_order, qgcm_train *h_trains, uint32_t counts[2]) {
    if (!ctx || n > QGCM_MAX_BATCH || !counts || (n && (!h_lens || !h_peer || !h_order || !h_trains)))
        return QGCM_E_ARG;
    qgcm_plan_limits lim;
    if (!plan_limits_resolve(limits, &lim)) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    std::lock_guard<std::mutex> pg(r->pipe_mu);
    if (n == 0 || n < r->plan_device_min) {
        send_plan_cpu(n, h_lens, h_peer, ctx_max_keys(ctx), lim, h_order, h_trains, counts);
        return QGCM_OK;
    }
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    hipStream_t s = pipe_stream(r);
    if (!s) return QGCM_E_HIP;
    // trains (16-B aligned), lengths, peers, order, counts, then the work area (256-B aligned)
    const size_t o_trains = 0, o_lens = o_trains + 16ull * n, o_peer = o_lens + 4ull * n, o_order = o_peer + 4ull * n,
                 o_counts = o_order + 4ull * n, o_work = (o_counts + 8 + 255) & ~(size_t)255;
    const uint64_t work_bytes = send_plan_work_bytes(n);
    if (!grow(r->d_plan, r->plan_cap, o_work + (size_t)work_bytes)) return QGCM_E_NOMEM;
    qgcm_train *d_trains = reinterpret_cast<qgcm_train *>(r->d_plan + o_trains);
    uint32_t *d_lens = reinterpret_cast<uint32_t *>(r->d_plan + o_lens);
    uint32_t *d_peer = reinterpret_cast<uint32_t *>(r->d_plan + o_peer);
    uint32_t *d_order = reinterpret_cast<uint32_t *>(r->d_plan + o_order);
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(r->d_plan + o_counts);
    // every way out waits for the stream: the next call reuses d_plan, and the caller its arrays
    bool ok = hipMemcpyAsync(d_lens, h_lens, 4ull * n, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(d_peer, h_peer, 4ull * n, hipMemcpyHostToDevice, s) == hipSuccess &&
              launch_send_plan(n, ctx_max_keys(ctx), d_lens, d_peer, lim, d_order, d_trains, d_counts,
                               r->d_plan + o_work, work_bytes, s) == hipSuccess &&
              hipMemcpyAsync(counts, d_counts, 8, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok || counts[0] > n || counts[1] > counts[0]) return QGCM_E_HIP;
    ok = (!counts[0] || hipMemcpyAsync(h_order, d_order, 4ull * counts[0], hipMemcpyDeviceToHost, s) == hipSuccess) &&
         (!counts[1] || hipMemcpyAsync(h_trains, d_trains, 16ull * counts[1], hipMemcpyDeviceToHost, s) == hipSuccess);
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    return ok ? QGCM_OK : QGCM_E_HIP;
}

int qgcm_gro_unpack(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gro_buf *d_bufs,
                    uint32_t n_bufs, uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, void *stream) {
    if (!ctx || n > QGCM_MAX_BATCH || n_bufs > n || (stride & 3)) return QGCM_E_ARG;
    if (n_bufs && (!d_packed || !d_bufs || !d_arena || !d_lens || stride == 0)) return QGCM_E_ARG;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_bufs & 15) || ((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3))
        return QGCM_E_ARG;
    if (n == 0 || n_bufs == 0) return QGCM_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    return hip_rc(launch_gro_unpack(d_packed, packed_len, d_bufs, n_bufs, n, d_arena, stride, d_lens, (hipStream_t)stream));
}

int qgcm_gro_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gro_buf *d_bufs,
                     uint32_t n_bufs, uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens,
                     uint32_t *d_peer, qgcm_desc *d_descs, void *stream) {
    return gro_resolve(ctx, d_packed, packed_len, d_bufs, n_bufs, n, d_arena, stride, d_lens, d_peer, d_descs,
                       (hipStream_t)stream);
}

int qgcm_gro_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_gro_buf *bufs, uint32_t n_bufs,
                        uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens) {
    if (n > QGCM_MAX_BATCH || n_bufs > n || (stride & 3)) return QGCM_E_ARG;
    if (n && (!packed || !bufs || !arena || !lens || stride == 0)) return QGCM_E_ARG;
    if (!gro_table_ok(bufs, n_bufs, n)) return QGCM_E_ARG;
    gro_unpack_cpu(packed, packed_len, bufs, n_bufs, n, arena, stride, lens);
    return QGCM_OK;
}

int qgcm_route_open_gro_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_gro_buf *bufs,
                             uint32_t n_bufs, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                             uint32_t *h_peer, uint8_t *h_status) {
    return run_route_gro_host(ctx, h_packed, packed_len, bufs, n_bufs, h_arena, stride, n, h_lens, h_peer, h_status, false, 0);
}

int qgcm_route_chain_open_gro_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                   const qgcm_gro_buf *bufs, uint32_t n_bufs, uint8_t *h_arena, uint64_t stride,
                                   uint32_t n, uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status) {
    return run_route_gro_host(ctx, h_packed, packed_len, bufs, n_bufs, h_arena, stride, n, h_lens, h_peer, h_status, true,
                              plugins);
}

uint64_t qgcm_deliver_pack_work(uint32_t n) { return deliver_pack_work_bytes(n); }

int qgcm_deliver_pack(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                      const uint32_t *d_peer, const uint8_t *d_status, uint8_t *d_packed, uint64_t packed_cap,
                      qgcm_pack_rec *d_recs, uint64_t *d_counts, void *d_work, void *stream) {
    if (!ctx || n > QGCM_MAX_BATCH || (stride & 3) || packed_cap > kPackMaxCap || !d_counts) return QGCM_E_ARG;
    if (n && (!d_arena || !d_lens || !d_peer || !d_packed || !d_recs || !d_work || stride == 0)) return QGCM_E_ARG;
    if (((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) || ((uintptr_t)d_peer & 3) || ((uintptr_t)d_packed & 15) ||
        ((uintptr_t)d_recs & 15) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_work & 15))
        return QGCM_E_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    return hip_rc(launch_deliver_pack(d_arena, stride, n, d_lens, d_peer, d_status, d_packed, packed_cap, d_recs, d_counts,
                                      d_work, (hipStream_t)stream));
}

int qgcm_route_chain_open_packed_host(qgcm_ctx *ctx, const uint8_t *h_arena, uint64_t stride, uint32_t n,
                                      uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                      uint8_t *h_out, uint64_t out_cap, qgcm_pack_rec *h_recs, uint64_t out[3]) {
    PackOut pk;
    if (!pack_out(pk, false, n, h_out, out_cap, h_recs, out)) return QGCM_E_ARG;
    // the arena is only read: with `pk` the copy back never names it
    return run_route_host(ctx, false, const_cast<uint8_t *>(h_arena), stride, n, h_lens, nullptr, h_peer, h_status, true,
                          plugins, &pk);
}

int qgcm_route_chain_open_gro_packed_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                          const qgcm_gro_buf *bufs, uint32_t n_bufs, uint64_t stride, uint32_t n,
                                          uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                          uint8_t *h_out, uint64_t out_cap, qgcm_pack_rec *h_recs, uint64_t out[3]) {
    PackOut pk;
    if (!pack_out(pk, false, n, h_out, out_cap, h_recs, out)) return QGCM_E_ARG;
    return run_route_gro_host(ctx, h_packed, packed_len, bufs, n_bufs, nullptr, stride, n, h_lens, h_peer, h_status, true,
                              plugins, &pk);
}

uint64_t qgcm_deliver_coalesce_work(uint32_t n) { return deliver_coalesce_work_bytes(n); }

int qgcm_deliver_coalesce(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_lens,
                          const uint32_t *d_peer, const uint8_t *d_status, uint8_t *d_packed, uint64_t packed_cap,
                          qgcm_gso_frame *d_frames, uint64_t *d_counts, void *d_work, void *stream) {
    if (!ctx || n > QGCM_MAX_BATCH || (stride & 3) || packed_cap > kPackMaxCap || !d_counts) return QGCM_E_ARG;
    if (n && (!d_arena || !d_lens || !d_peer || !d_packed || !d_frames || !d_work || stride == 0)) return QGCM_E_ARG;
    if (((uintptr_t)d_arena & 3) || ((uintptr_t)d_lens & 3) || ((uintptr_t)d_peer & 3) || ((uintptr_t)d_packed & 15) ||
        ((uintptr_t)d_frames & 15) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_work & 15))
        return QGCM_E_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    return hip_rc(launch_deliver_coalesce(d_arena, stride, n, d_lens, d_peer, d_status, d_packed, packed_cap, d_frames,
                                          d_counts, d_work, (hipStream_t)stream));
}

int qgcm_route_chain_open_coalesced_host(qgcm_ctx *ctx, const uint8_t *h_arena, uint64_t stride, uint32_t n,
                                         uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                         uint8_t *h_out, uint64_t out_cap, qgcm_gso_frame *h_frames, uint64_t out[5]) {
    PackOut pk;
    if (!pack_out(pk, true, n, h_out, out_cap, h_frames, out)) return QGCM_E_ARG;
    return run_route_host(ctx, false, const_cast<uint8_t *>(h_arena), stride, n, h_lens, nullptr, h_peer, h_status, true,
                          plugins, &pk);
}

int qgcm_route_chain_open_gro_coalesced_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len,
                                             const qgcm_gro_buf *bufs, uint32_t n_bufs, uint64_t stride, uint32_t n,
                                             uint32_t *h_lens, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status,
                                             uint8_t *h_out, uint64_t out_cap, qgcm_gso_frame *h_frames,
                                             uint64_t out[5]) {
    PackOut pk;
    if (!pack_out(pk, true, n, h_out, out_cap, h_frames, out)) return QGCM_E_ARG;
    return run_route_gro_host(ctx, h_packed, packed_len, bufs, n_bufs, nullptr, stride, n, h_lens, h_peer, h_status, true,
                              plugins, &pk);
}

uint64_t qgcm_train_pack_work(uint32_t n) { return train_pack_work_bytes(n); }

int qgcm_train_pack(qgcm_ctx *ctx, const uint8_t *d_arena, uint64_t stride, uint32_t n, const uint32_t *d_order,
                    const qgcm_train *d_trains, const uint32_t *d_plan_counts, uint8_t *d_packed, uint64_t packed_cap,
                    qgcm_ptrain *d_ptrains, uint64_t *d_pcounts, void *d_work, void *stream) {
    if (!ctx || n > QGCM_MAX_BATCH || (stride & 3) || packed_cap > kTrainMaxCap || !d_pcounts) return QGCM_E_ARG;
    if (n && (!d_arena || !d_order || !d_trains || !d_plan_counts || !d_packed || !d_ptrains || !d_work || stride == 0))
        return QGCM_E_ARG;
    if (((uintptr_t)d_arena & 3) || ((uintptr_t)d_order & 3) || ((uintptr_t)d_trains & 15) || ((uintptr_t)d_plan_counts & 3) ||
        ((uintptr_t)d_packed & 15) || ((uintptr_t)d_ptrains & 15) || ((uintptr_t)d_pcounts & 7) || ((uintptr_t)d_work & 15))
        return QGCM_E_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    return hip_rc(launch_train_pack(d_arena, stride, n, d_order, d_trains, d_plan_counts, d_packed, packed_cap, d_ptrains,
                                    d_pcounts, d_work, (hipStream_t)stream));
}

int qgcm_route_chain_seal_packed_host(qgcm_ctx *ctx, const uint8_t *h_arena, uint64_t stride, uint32_t n,
                                      uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins,
                                      const qgcm_plan_limits *limits, uint32_t *h_peer, uint8_t *h_status,
                                      uint8_t *h_out, uint64_t out_cap, qgcm_ptrain *h_ptrains, uint32_t *h_order,
                                      uint64_t out[4]) {
    TrainOut tk;
    if (!train_out(tk, n, h_out, out_cap, h_ptrains, h_order, limits, out)) return QGCM_E_ARG;
    // the arena is only read: with `tk` the copy back never names it
    return run_route_host(ctx, true, const_cast<uint8_t *>(h_arena), stride, n, h_lens, h_nonces, h_peer, h_status, true,
                          plugins, nullptr, &tk);
}

int qgcm_frames_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_frame *d_frames, uint32_t n,
                        uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, uint32_t *d_peer, qgcm_desc *d_descs, void *stream) {
    return frames_resolve(ctx, d_packed, packed_len, d_frames, n, d_arena, stride, d_lens, d_peer, d_descs, (hipStream_t)stream);
}

int qgcm_frames_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_frame *frames, uint32_t n, uint8_t *arena,
                           uint64_t stride, uint32_t *lens) {
    return frames_unpack_checked(packed, packed_len, frames, n, arena, stride, lens);
}

int qgcm_route_chain_seal_frames_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_frame *frames,
                                      uint64_t stride, uint32_t n, uint32_t *h_lens, const uint8_t *h_nonces, uint32_t plugins,
                                      const qgcm_plan_limits *limits, uint32_t *h_peer, uint8_t *h_status, uint8_t *h_out,
                                      uint64_t out_cap, qgcm_ptrain *h_ptrains, uint32_t *h_order, uint64_t out[4]) {
    TrainOut tk;
    if (!train_out(tk, n, h_out, out_cap, h_ptrains, h_order, limits, out)) return QGCM_E_ARG;
    return run_route_frames_host(ctx, h_packed, packed_len, frames, stride, n, h_lens, h_nonces, plugins, h_peer, h_status, tk);
}

int qgcm_gso_resolve(qgcm_ctx *ctx, const uint8_t *d_packed, uint64_t packed_len, const qgcm_gso_frame *d_frames, uint32_t n_frames,
                     uint32_t n, uint8_t *d_arena, uint64_t stride, uint32_t *d_lens, uint32_t *d_peer, qgcm_desc *d_descs,
                     void *stream) {
    return gso_resolve(ctx, d_packed, packed_len, d_frames, n_frames, n, d_arena, stride, d_lens, d_peer, d_descs,
                       (hipStream_t)stream);
}

int qgcm_gso_unpack_cpu(const uint8_t *packed, uint64_t packed_len, const qgcm_gso_frame *frames, uint32_t n_frames, uint32_t n,
                        uint8_t *arena, uint64_t stride, uint32_t *lens) {
    return gso_unpack_checked(packed, packed_len, frames, n_frames, n, arena, stride, lens);
}

int qgcm_route_chain_seal_gso_host(qgcm_ctx *ctx, const uint8_t *h_packed, uint64_t packed_len, const qgcm_gso_frame *frames,
                                   uint32_t n_frames, uint64_t stride, uint32_t n, uint32_t *h_lens, const uint8_t *h_nonces,
                                   uint32_t plugins, const qgcm_plan_limits *limits, uint32_t *h_peer, uint8_t *h_status,
                                   uint8_t *h_out, uint64_t out_cap, qgcm_ptrain *h_ptrains, uint32_t *h_order, uint64_t out[4]) {
    TrainOut tk;
    if (!train_out(tk, n, h_out, out_cap, h_ptrains, h_order, limits, out)) return QGCM_E_ARG;
    return run_route_gso_host(ctx, h_packed, packed_len, frames, n_frames, stride, n, h_lens, h_nonces, plugins, h_peer, h_status, tk);
}

int qgcm_route_stats(qgcm_ctx *ctx, int dir, uint32_t peer, uint64_t out[4]) {
    if (!ctx || !out || (dir != QGCM_TX && dir != QGCM_RX)) return QGCM_E_ARG;
    if (peer != QGCM_NO_PEER && peer >= ctx_max_keys(ctx)) return QGCM_E_ARG;
    RouteState *r = ctx_route(ctx);
    const unsigned long long *src;
    {
        std::lock_guard<std::mutex> g(r->mu);
        if (!r->set) return QGCM_E_ARG;
        src = r->d_counters + (size_t)dir * r->dir_words + (peer == QGCM_NO_PEER ? 0 : 4 + 4ull * peer);
    }
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return QGCM_E_HIP;
    return hip_rc(hipMemcpy(out, src, 32, hipMemcpyDeviceToHost));
}

int qgcm_route_seal_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                         const uint8_t *h_nonces, uint32_t *h_peer, uint8_t *h_status) {
    return run_route_host(ctx, true, h_arena, stride, n, h_lens, h_nonces, h_peer, h_status);
}

int qgcm_route_open_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                         uint32_t *h_peer, uint8_t *h_status) {
    return run_route_host(ctx, false, h_arena, stride, n, h_lens, nullptr, h_peer, h_status);
}

int qgcm_route_chain_seal_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                               const uint8_t *h_nonces, uint32_t plugins, uint32_t *h_peer, uint8_t *h_status) {
    return run_route_host(ctx, true, h_arena, stride, n, h_lens, h_nonces, h_peer, h_status, true, plugins);
}

int qgcm_route_chain_open_host(qgcm_ctx *ctx, uint8_t *h_arena, uint64_t stride, uint32_t n, uint32_t *h_lens,
                               uint32_t plugins, uint32_t *h_peer, uint8_t *h_status) {
    return run_route_host(ctx, false, h_arena, stride, n, h_lens, nullptr, h_peer, h_status, true, plugins);
}

}  // extern "C"
