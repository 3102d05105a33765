// coalesce_kernels.hip -- delivered TCP segments of a routed batch coalesced into super-frames for the TUN write
// (include/qgcm.h "delivered TCP segments coalesced on routed batches"): the mirror of
// gso_kernels.hip.  After the incoming chain the delivered packets lie in slots of `stride` bytes; here every
// run of in-order segments of one flow, checksums verified, becomes one packet behind a virtio_net_hdr, and every
// other delivered packet a plain one, in the layout qgcm_tun_read_gso produces.
//
//   co_classify_kernel    candidate rule, both checksums, the header compare with slot i - 1    16 lanes a slot
//   co_head_tile_kernel   each 256-slot tile's last stretch head                                one lane a slot
//   co_head_spine_kernel  exclusive max-prefix of the tile heads, in place                      one workgroup
//   co_head_emit_kernel   the tile's scan again under its prefix: head[i]                       one lane a slot
//   co_frame_tile_kernel  each tile's {bytes, entries, coalesced, delivered}                    one lane a slot
//   co_frame_spine_kernel exclusive prefix of the tile sums, in place                           one workgroup
//   co_frame_emit_kernel  the tile's scan again: the table, each slot's entry and place, counts one lane a slot
//   co_copy_kernel        the bytes, 16 lanes a delivered slot                                  grid-stride
//
// No atomics, no counter to zero, no workgroup waits for another: both scans are reduce-then-scan over separate
// launches as in pack_kernels.hip, so calls on several streams share nothing but read-only inputs, and the host
// does not synchronise between the launches.  A frame's size is attributed to its last member, so the exclusive
// prefix is the same at every member and is where the frame's region starts.
//
// Classify.  The packet at slot + 4 is dword-aligned, and a ones'-complement sum does not care how its 16-bit
// words are grouped, so nothing is realigned: the 16-byte path loads aligned 16-byte pieces of the slot and adds
// each dword to the sum it belongs to by its index in the packet, the dword path the same a dword at a time.
// Everything is summed as little-endian dwords with the carry brought round (gso_kernels.hip); the IPv4 header's
// dwords go to the IPv4 sum, the addresses to both, the rest to the TCP sum, the checksum fields masked out, the
// bytes behind L masked to zero.  Both sums go round the slot's 16 lanes with four __shfl_xor steps.  The header's
// at most 30 dwords are compared with the neighbour's by lanes g and g + 16 under co_cmp_mask.  No load reaches
// past the dword (16-byte path: the 16-byte piece) that holds byte 4 + L - 1 of a delivered slot, which ends at
// or below stride; of the neighbour only header dwords below its own 4 + L are read.
//
// Copy.  Every byte of the packed area has exactly one writer.  The lead (six zeros, the vnet header) is one
// 16-byte store of lane 0 of the frame's first slot; the patched header dwords are stored by lanes g and g + 16 of
// that slot, a dword a lane; every member -- the first included -- moves its own payload to off + rel, which has
// any alignment, by destination granule (16 bytes, or a dword on the dword path): a granule it owns whole is one
// store, a granule it shares with a neighbouring member is stored as its whole dwords and at most three single
// bytes an end, and only source pieces that hold a needed byte are loaded.  The last member's range runs on to the
// 16-byte boundary, its bytes behind the packet zero.  An entry that did not fit is not copied.
#include "coalesce_core.h"
#include "gcm_internal.h"
#include "gro_copy.h"

namespace qgcm {
namespace {

constexpr uint32_t kCoTile = 256;  // slots per workgroup of the tile and emit kernels, one per lane
constexpr uint32_t kCoSpineThreads = 1024;
constexpr uint32_t kCoThreads = 256;                     // classify and copy
constexpr uint32_t kCoWave = 64;
constexpr uint32_t kCoSlots = kCoThreads / kGroLanes;    // slots of one workgroup per pass
constexpr uint32_t kCoMaxBlocks = 4096;                  // as pack_copy_kernel's grid

struct CoSum {
    uint64_t bytes;
    uint32_t entries, coalesced, delivered, pad;
};

struct CoArgs {
    const uint8_t *arena;
    uint64_t stride;
    uint32_t n;
    const uint32_t *lens, *peer;
    const uint8_t *status;  // NULL: every packet has status 1
    uint8_t *packed;
    uint64_t packed_cap;
    qgcm_gso_frame *frames;
    uint64_t *counts;
    uint32_t *cls, *head, *entry, *rel;  // n words each
    uint32_t *tile_head;                 // per tile
    CoSum *tile_sum;                     // per tile
};

__device__ __forceinline__ uint32_t add1c(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s + (s < b);
}

__device__ __forceinline__ uint32_t fold16(uint32_t s) {
    s = (s & 0xffffu) + (s >> 16);
    return (s & 0xffffu) + (s >> 16);
}

__device__ __forceinline__ uint32_t sum_lanes(uint32_t v) {
#pragma unroll
    for (uint32_t m = kGroLanes / 2; m; m >>= 1) v = add1c(v, (uint32_t)__shfl_xor((int)v, (int)m, (int)kGroLanes));
    return v;
}

__device__ __forceinline__ uint32_t or_lanes(uint32_t v) {
#pragma unroll
    for (uint32_t m = kGroLanes / 2; m; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, (int)m, (int)kGroLanes);
    return v;
}

// packet dword w (value v, bytes behind L already zero) into the sum it belongs to
__device__ __forceinline__ void co_acc(uint32_t w, uint32_t v, uint32_t j0, uint32_t &ip, uint32_t &l4) {
    if (w < j0) {
        if (w == 2) v &= 0xffffu;
        ip = add1c(ip, v);
        if (w == 3 || w == 4) l4 = add1c(l4, v);
    } else {
        if (w == j0 + 4) v &= 0xffff0000u;
        l4 = add1c(l4, v);
    }
}

__device__ __forceinline__ uint32_t keep_low(uint32_t v, int64_t keep) {
    return keep >= 4 ? v : keep <= 0 ? 0u : v & ((1u << (8 * (uint32_t)keep)) - 1u);
}

template <bool kWide>
__global__ void __launch_bounds__(kCoThreads) co_classify_kernel(CoArgs a) {
    const uint32_t g = threadIdx.x % kGroLanes;
    // the loop's bound is the wave's, so that all 64 lanes execute the shuffles
    const uint64_t wave0 = ((uint64_t)blockIdx.x * kCoThreads + threadIdx.x) / kCoWave * (kCoWave / kGroLanes);
    for (uint64_t base = wave0; base < a.n; base += (uint64_t)gridDim.x * kCoSlots) {
        const uint64_t i = base + (threadIdx.x % kCoWave) / kGroLanes;
        uint32_t cls = 0, L = 0, ihl = 0, w1 = 0, w2 = 0, t4 = 0;
        const uint32_t *p = nullptr;
        if (i < a.n) {
            L = a.lens[i];
            if (pack_delivered(a.status ? a.status[i] : 1u, L, a.stride)) {
                cls = kCoDelivered;
                p = reinterpret_cast<const uint32_t *>(a.arena + i * a.stride + kGsoPacketStart);
                if (L >= 40) {
                    w1 = p[1];
                    w2 = p[2];
                    uint32_t c = 0;
                    if (co_ip_ok(L, p[0], w1, w2, ihl) && co_tcp_ok(L, ihl, p[(ihl >> 2) + 3], c)) {
                        cls |= c;
                        t4 = p[(ihl >> 2) + 4];
                    }
                }
            }
        }
        const bool header = cls & kCoHeader;
        const uint32_t j0 = ihl >> 2, words = header ? (L + 3) >> 2 : 0;
        uint32_t ip = 0, l4 = 0;
        if (kWide) {
            // slot piece q holds packet dwords 4q - 1 .. 4q + 2
            const uint4 *s16 = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(p) - kGsoPacketStart);
            const uint32_t pieces = header ? (uint32_t)((kGsoPacketStart + L + 15) >> 4) : 0;  // those below 4 + L
            for (uint32_t q = g; q < pieces; q += kGroLanes) {
                const uint4 v = s16[q];
                const int64_t w = 4ll * q - 1, left = (int64_t)L - 4 * w;
                if (q) co_acc((uint32_t)w, keep_low(v.x, left), j0, ip, l4);
                if (w + 1 < words) co_acc((uint32_t)w + 1, keep_low(v.y, left - 4), j0, ip, l4);
                if (w + 2 < words) co_acc((uint32_t)w + 2, keep_low(v.z, left - 8), j0, ip, l4);
                if (w + 3 < words) co_acc((uint32_t)w + 3, keep_low(v.w, left - 12), j0, ip, l4);
            }
        } else {
            for (uint32_t w = g; w < words; w += kGroLanes) co_acc(w, keep_low(p[w], (int64_t)L - 4ll * w), j0, ip, l4);
        }
        // the pseudo-header's protocol and TCP length
        if (g == 0 && header) l4 = add1c(l4, 6u << 8 | co_swap16(L - ihl) << 16);
        ip = sum_lanes(ip);
        l4 = sum_lanes(l4);
        if (header && (~fold16(ip) & 0xffffu) == w2 >> 16 && (~fold16(l4) & 0xffffu) == (t4 & 0xffffu)) cls |= kCoCand;
        // the header compare with slot i - 1: it is delivered and holds as many header bytes
        const uint32_t hdr = co_hdr(cls);
        uint32_t diff = 1;
        if (header && i > 0) {
            const uint32_t L_prev = a.lens[i - 1];
            if (pack_delivered(a.status ? a.status[i - 1] : 1u, L_prev, a.stride) && L_prev >= hdr && a.peer[i] == a.peer[i - 1]) {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(p) - a.stride);
                diff = 0;
                if (g < hdr >> 2) diff |= (p[g] ^ q[g]) & co_cmp_mask(g, j0);
                if (g + kGroLanes < hdr >> 2) diff |= (p[g + kGroLanes] ^ q[g + kGroLanes]) & co_cmp_mask(g + kGroLanes, j0);
                if (g == 0 && !co_follows(q[1], q[j0 + 1], q[j0 + 3], L_prev - hdr, w1, p[j0 + 1])) diff = 1;
            }
        }
        diff = or_lanes(diff);
        if (header && !diff) cls |= kCoHdrLink;
        if (g == 0 && i < a.n) a.cls[i] = cls;
    }
}

// inclusive scans over the workgroup's kThreads lanes
template <uint32_t kThreads>
__device__ inline void co_scan_max(uint32_t &v, uint32_t *sv) {
    const uint32_t t = threadIdx.x;
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        sv[t] = v;
        __syncthreads();
        if (t >= d) v = max(v, sv[t - d]);
        __syncthreads();
    }
}

template <uint32_t kThreads>
__device__ inline void co_scan_sum(CoSum &v, CoSum *sv) {
    const uint32_t t = threadIdx.x;
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        sv[t] = v;
        __syncthreads();
        if (t >= d) {
            const CoSum o = sv[t - d];
            v.bytes += o.bytes;
            v.entries += o.entries;
            v.coalesced += o.coalesced;
            v.delivered += o.delivered;
        }
        __syncthreads();
    }
}

// the class word of slot x, 0 outside the batch
struct CoClsAt {
    const uint32_t *cls;
    uint32_t n;
    __device__ __forceinline__ uint32_t operator()(int64_t x) const { return x < 0 || x >= (int64_t)n ? 0u : cls[x]; }
};

struct CoHeadAt {
    const uint32_t *head;
    __device__ __forceinline__ int64_t operator()(int64_t x) const { return (int64_t)head[x]; }
};

// a lane's slot as a stretch head: its index when no eq joins it to slot i - 1, else 0
__device__ inline uint32_t co_head_item(const CoArgs &a, uint32_t i) {
    if (i == 0 || i >= a.n) return 0;
    return co_eq(a.cls[i - 1], a.cls[i]) ? 0u : i;
}

__global__ void __launch_bounds__(kCoTile) co_head_tile_kernel(CoArgs a) {
    __shared__ uint32_t sv[kCoTile];
    uint32_t v = co_head_item(a, blockIdx.x * kCoTile + threadIdx.x);
    co_scan_max<kCoTile>(v, sv);
    if (threadIdx.x == kCoTile - 1) a.tile_head[blockIdx.x] = v;
}

__global__ void __launch_bounds__(kCoSpineThreads) co_head_spine_kernel(uint32_t *tiles, uint32_t ntiles) {
    __shared__ uint32_t sv[kCoSpineThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kCoSpineThreads - 1) / kCoSpineThreads;
    const uint32_t lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    uint32_t v = 0;
    for (uint32_t k = lo; k < hi; ++k) v = max(v, tiles[k]);
    co_scan_max<kCoSpineThreads>(v, sv);
    __syncthreads();
    sv[t] = v;
    __syncthreads();
    uint32_t run = t ? sv[t - 1] : 0u;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t x = tiles[k];
        tiles[k] = run;
        run = max(run, x);
    }
}

__global__ void __launch_bounds__(kCoTile) co_head_emit_kernel(CoArgs a) {
    __shared__ uint32_t sv[kCoTile];
    const uint32_t i = blockIdx.x * kCoTile + threadIdx.x;
    uint32_t v = co_head_item(a, i);
    co_scan_max<kCoTile>(v, sv);
    if (i < a.n) a.head[i] = max(v, a.tile_head[blockIdx.x]);
}

// A lane's slot in its frame: what it adds to the sums (a frame's size at its last member) and its role
struct CoItem {
    CoSum add;
    CoRole role;
    uint32_t cls, len;
};

__device__ inline CoItem co_frame_item(const CoArgs &a, uint32_t i) {
    CoItem it{CoSum{0, 0, 0, 0, 0}, CoRole{false, 0, 0, 0}, 0, 0};
    if (i >= a.n) return it;
    it.cls = a.cls[i];
    if (!(it.cls & kCoDelivered)) return it;
    it.add.delivered = 1;
    it.role = co_role(CoClsAt{a.cls, a.n}, CoHeadAt{a.head}, (int64_t)i);
    if (!it.role.end) return it;
    it.len = it.role.count == 1 ? a.lens[i] : co_hdr(it.cls) + it.role.payload;
    it.add.bytes = co_region(it.len);
    it.add.entries = 1;
    it.add.coalesced = it.role.count > 1;
    return it;
}

__global__ void __launch_bounds__(kCoTile) co_frame_tile_kernel(CoArgs a) {
    __shared__ CoSum sv[kCoTile];
    CoSum v = co_frame_item(a, blockIdx.x * kCoTile + threadIdx.x).add;
    co_scan_sum<kCoTile>(v, sv);
    if (threadIdx.x == kCoTile - 1) a.tile_sum[blockIdx.x] = v;
}

__global__ void __launch_bounds__(kCoSpineThreads) co_frame_spine_kernel(CoSum *tiles, uint32_t ntiles) {
    __shared__ CoSum sv[kCoSpineThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (ntiles + kCoSpineThreads - 1) / kCoSpineThreads;
    const uint32_t lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    CoSum v{0, 0, 0, 0, 0};
    for (uint32_t k = lo; k < hi; ++k) {
        const CoSum x = tiles[k];
        v.bytes += x.bytes;
        v.entries += x.entries;
        v.coalesced += x.coalesced;
        v.delivered += x.delivered;
    }
    const CoSum own = v;
    co_scan_sum<kCoSpineThreads>(v, sv);
    CoSum run{v.bytes - own.bytes, v.entries - own.entries, v.coalesced - own.coalesced, v.delivered - own.delivered, 0};
    for (uint32_t k = lo; k < hi; ++k) {
        const CoSum x = tiles[k];
        tiles[k] = run;
        run.bytes += x.bytes;
        run.entries += x.entries;
        run.coalesced += x.coalesced;
        run.delivered += x.delivered;
    }
}

__global__ void __launch_bounds__(kCoTile) co_frame_emit_kernel(CoArgs a) {
    __shared__ CoSum sv[kCoTile];
    const uint32_t i = blockIdx.x * kCoTile + threadIdx.x;
    const CoItem it = co_frame_item(a, i);
    CoSum v = it.add;
    co_scan_sum<kCoTile>(v, sv);
    if (i >= a.n) return;
    const CoSum before = a.tile_sum[blockIdx.x];
    if (it.cls & kCoDelivered) {
        // the exclusive prefix: the same at every member of a frame
        const uint32_t k = before.entries + v.entries - it.add.entries;
        a.entry[i] = k;
        a.rel[i] = it.role.rel;
        if (it.role.end) {
            const uint64_t start = before.bytes + v.bytes - it.add.bytes;
            const qgcm_gso_frame f = co_entry(it.cls, it.len, it.role, i, start, a.packed_cap, a.peer[i - (it.role.count - 1)]);
            uint4 *dst = reinterpret_cast<uint4 *>(a.frames + k);
            dst[0] = make_uint4(f.off, f.len, f.first, f.count);
            dst[1] = make_uint4(f.gso_size | (uint32_t)f.hdr_len << 16, f.l4_off | (uint32_t)f.csum_off << 16, f.kind, f.reserved);
        }
    }
    if (i == a.n - 1u) {
        a.counts[0] = before.entries + v.entries;
        a.counts[1] = before.bytes + v.bytes;
        a.counts[2] = before.coalesced + v.coalesced;
        a.counts[3] = before.delivered + v.delivered;
    }
}

// destination dword at packed byte x (a multiple of 4) of a member whose bytes are [lo, hi): whole when it is the
// member's own, else the bytes that are
__device__ __forceinline__ void co_put(uint8_t *packed, uint64_t x, uint32_t w, uint64_t lo, uint64_t hi) {
    if (x >= lo && x + 4 <= hi) {
        *reinterpret_cast<uint32_t *>(packed + x) = w;
        return;
    }
    const uint64_t from = x > lo ? x : lo, to = x + 4 < hi ? x + 4 : hi;
    for (uint64_t b = from; b < to; ++b) packed[b] = (uint8_t)(w >> (8 * (uint32_t)(b - x)));
}

// packed bytes [lo, hi) by the 16 lanes of a slot, lane g of them: [lo, data_hi) from s0 + [lo, data_hi) (s0: the
// address packed byte 0 would come from, any alignment), zeros behind.  A source piece is loaded only when it
// holds a byte of [lo, data_hi).
template <bool kWide>
__device__ __forceinline__ void co_copy_span(uint8_t *packed, uint64_t lo, uint64_t data_hi, uint64_t hi, uintptr_t s0, uint32_t g) {
    if (kWide) {
        const uint32_t sh = (uint32_t)(s0 & 15u);
        const bool q2 = sh & 8u, q1 = sh & 4u;
        const uint32_t r = sh & 3u;
        for (uint64_t at = 16 * ((lo >> 4) + g); at < hi; at += 16 * kGroLanes) {
            const uint64_t need_lo = at > lo ? at : lo, need_hi = at + 16 < data_hi ? at + 16 : data_hi;
            const uintptr_t blk = s0 + at - sh;  // the 16-byte piece that holds the source of packed byte `at`
            uint4 l = make_uint4(0, 0, 0, 0), h = make_uint4(0, 0, 0, 0);
            if (need_lo < need_hi) {
                if (s0 + need_lo < blk + 16) l = *reinterpret_cast<const uint4 *>(blk);
                if (s0 + need_hi > blk + 16) h = *reinterpret_cast<const uint4 *>(blk + 16);
            }
            const uint32_t a0 = q2 ? l.z : l.x, a1 = q2 ? l.w : l.y, a2 = q2 ? h.x : l.z, a3 = q2 ? h.y : l.w,
                           a4 = q2 ? h.z : h.x, a5 = q2 ? h.w : h.y;
            const uint32_t b0 = q1 ? a1 : a0, b1 = q1 ? a2 : a1, b2 = q1 ? a3 : a2, b3 = q1 ? a4 : a3, b4 = q1 ? a5 : a4;
            uint4 out = make_uint4(funnel(b1, b0, r), funnel(b2, b1, r), funnel(b3, b2, r), funnel(b4, b3, r));
            const int64_t keep = (int64_t)data_hi - (int64_t)at;
            out.x = keep_low(out.x, keep);
            out.y = keep_low(out.y, keep - 4);
            out.z = keep_low(out.z, keep - 8);
            out.w = keep_low(out.w, keep - 12);
            if (at >= lo && at + 16 <= hi) {
                *reinterpret_cast<uint4 *>(packed + at) = out;
            } else {
                if (at + 4 > lo) co_put(packed, at, out.x, lo, hi);
                if (at + 8 > lo && at + 4 < hi) co_put(packed, at + 4, out.y, lo, hi);
                if (at + 12 > lo && at + 8 < hi) co_put(packed, at + 8, out.z, lo, hi);
                if (at + 12 < hi) co_put(packed, at + 12, out.w, lo, hi);
            }
        }
    } else {
        const uint32_t sh = (uint32_t)(s0 & 3u);
        for (uint64_t at = 4 * ((lo >> 2) + g); at < hi; at += 4 * kGroLanes) {
            const uint64_t need_lo = at > lo ? at : lo, need_hi = at + 4 < data_hi ? at + 4 : data_hi;
            const uintptr_t blk = s0 + at - sh;
            uint32_t l = 0, h = 0;
            if (need_lo < need_hi) {
                if (s0 + need_lo < blk + 4) l = *reinterpret_cast<const uint32_t *>(blk);
                if (s0 + need_hi > blk + 4) h = *reinterpret_cast<const uint32_t *>(blk + 4);
            }
            co_put(packed, at, keep_low(funnel(h, l, sh), (int64_t)data_hi - (int64_t)at), lo, hi);
        }
    }
}

template <bool kWide>
__global__ void __launch_bounds__(kCoThreads) co_copy_kernel(CoArgs a) {
    const uint32_t g = threadIdx.x % kGroLanes;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * kCoThreads + threadIdx.x) / kCoWave * (kCoWave / kGroLanes);
    for (uint64_t base = wave0; base < a.n; base += (uint64_t)gridDim.x * kCoSlots) {
        const uint64_t i = base + (threadIdx.x % kCoWave) / kGroLanes;
        const uint32_t cls = i < a.n ? a.cls[i] : 0u;
        // an undelivered slot and an entry that did not fit have nothing to move: an empty range, no early way
        // out, so that all 64 lanes execute the shuffles
        uint32_t off = kCoNoRoom, len = 0, first = 0, count = 0, rel = 0;
        if (cls & kCoDelivered) {
            const uint4 f = *reinterpret_cast<const uint4 *>(a.frames + a.entry[i]);  // {off, len, first, count}
            off = f.x;
            len = f.y;
            first = f.z;
            count = f.w;
            rel = a.rel[i];
        }
        const bool fits = off != kCoNoRoom, merged = fits && count > 1, lead = fits && i == first;
        const uint8_t *pkt = a.arena + i * a.stride + kGsoPacketStart;  // dereferenced under `fits` only
        const uint32_t hdr = co_hdr(cls), ihl = co_ihl(cls), j0 = ihl >> 2;
        // the member's own bytes: a plain packet whole, a merged one's payload; the last member pads the frame
        uint64_t lo = 0, data_hi = 0, hi = 0;
        uintptr_t s0 = 0;
        if (fits) {
            lo = (uint64_t)off + (merged ? rel : 0u);
            data_hi = lo + (merged ? co_P(cls) : len);
            hi = i == (uint64_t)first + count - 1 ? (uint64_t)off + co_round16(len) : data_hi;
            s0 = (uintptr_t)pkt + (merged ? hdr : 0u) - (uintptr_t)lo;
        }
        co_copy_span<kWide>(a.packed, lo, data_hi, hi, s0, g);
        // the first member of a merged frame: its header's dwords g and g + 16, patched
        const bool head = merged && lead;
        const uint32_t words = head ? hdr >> 2 : 0;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(pkt);
        uint32_t h0 = 0, h1 = 0, ip = 0, l4 = 0;
        if (g < words) {
            h0 = p[g];
            if (g == 0) h0 = (h0 & 0xffffu) | co_swap16(len) << 16;
            if (g == 2) h0 &= 0xffffu;
            if (g < j0) ip = h0;
            if (g == 3 || g == 4) l4 = h0;
            if (g == 0) l4 = 6u << 8 | co_swap16(len - ihl) << 16;  // (dword 0 is no part of the pseudo-header)
        }
        if (g + kGroLanes < words) h1 = p[g + kGroLanes];
        ip = sum_lanes(ip);
        l4 = sum_lanes(l4);
        if (head) {
            const uint32_t psh = a.cls[first + count - 1] & kCoPsh ? 0x0800u : 0u;
            if (g == 2) h0 |= (~fold16(ip) & 0xffffu) << 16;
            if (g == j0 + 3) h0 = (h0 & ~0x0800u) | psh;
            if (g + kGroLanes == j0 + 3) h1 = (h1 & ~0x0800u) | psh;
            if (g == j0 + 4) h0 = (h0 & 0xffff0000u) | fold16(l4);
            if (g + kGroLanes == j0 + 4) h1 = (h1 & 0xffff0000u) | fold16(l4);
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.packed + off);
            if (g < words) dst[g] = h0;
            if (g + kGroLanes < words) dst[g + kGroLanes] = h1;
        }
        if (lead && g == 0) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (merged) {
                const uint4 t = *(reinterpret_cast<const uint4 *>(a.frames + a.entry[i]) + 1);  // {gso_size | hdr_len << 16, ..}
                v = make_uint4(0, 1u << 16 | 1u << 24, t.x >> 16 | t.x << 16, t.y);
            }
            *reinterpret_cast<uint4 *>(a.packed + off - kCoLead) = v;
        }
    }
}

inline uint32_t co_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kCoTile - 1) / kCoTile); }
inline uint64_t co_round256(uint64_t b) { return (b + 255) & ~(uint64_t)255; }

}  // namespace

uint64_t deliver_coalesce_work_bytes(uint32_t n) {
    const uint64_t nt = co_tiles(n);
    return co_round256(4ull * n) * 4 + co_round256(4 * nt) + co_round256(sizeof(CoSum) * nt) + 256;
}

hipError_t launch_deliver_coalesce(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                                   const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_gso_frame *frames,
                                   uint64_t *counts, void *work, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(counts, 0, 32, s);
    const uint32_t ntiles = co_tiles(n);
    uint8_t *w = static_cast<uint8_t *>(work);
    const uint64_t per = co_round256(4ull * n);
    CoArgs a{arena, stride, n, lens, peer, status, packed, packed_cap, frames, counts,
             reinterpret_cast<uint32_t *>(w), reinterpret_cast<uint32_t *>(w + per), reinterpret_cast<uint32_t *>(w + 2 * per),
             reinterpret_cast<uint32_t *>(w + 3 * per), reinterpret_cast<uint32_t *>(w + 4 * per),
             reinterpret_cast<CoSum *>(w + 4 * per + co_round256(4ull * ntiles))};
    const bool wide = (stride & 15) == 0 && ((uintptr_t)arena & 15) == 0;
    const uint64_t blocks = ((uint64_t)n + kCoSlots - 1) / kCoSlots;
    const dim3 grid((uint32_t)(blocks < kCoMaxBlocks ? blocks : kCoMaxBlocks));
    if (wide)
        hipLaunchKernelGGL(co_classify_kernel<true>, grid, dim3(kCoThreads), 0, s, a);
    else
        hipLaunchKernelGGL(co_classify_kernel<false>, grid, dim3(kCoThreads), 0, s, a);
    hipLaunchKernelGGL(co_head_tile_kernel, dim3(ntiles), dim3(kCoTile), 0, s, a);
    hipLaunchKernelGGL(co_head_spine_kernel, dim3(1), dim3(kCoSpineThreads), 0, s, a.tile_head, ntiles);
    hipLaunchKernelGGL(co_head_emit_kernel, dim3(ntiles), dim3(kCoTile), 0, s, a);
    hipLaunchKernelGGL(co_frame_tile_kernel, dim3(ntiles), dim3(kCoTile), 0, s, a);
    hipLaunchKernelGGL(co_frame_spine_kernel, dim3(1), dim3(kCoSpineThreads), 0, s, a.tile_sum, ntiles);
    hipLaunchKernelGGL(co_frame_emit_kernel, dim3(ntiles), dim3(kCoTile), 0, s, a);
    if (wide)
        hipLaunchKernelGGL(co_copy_kernel<true>, grid, dim3(kCoThreads), 0, s, a);
    else
        hipLaunchKernelGGL(co_copy_kernel<false>, grid, dim3(kCoThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
