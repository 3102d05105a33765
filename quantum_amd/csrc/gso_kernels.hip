// gso_kernels.hip -- TUN super-frames cut into slots and resolved in one launch (include/qgcm.h "TUN super-frames
// segmented on routed batches").
//
// frames_resolve_kernel (frames_kernels.hip) for a table whose entries name runs of slots: a TCP or UDP_L4
// super-frame as a queue opened with IFF_VNET_HDR hands it over becomes count packets, each with the frame's
// headers patched (lengths, id, sequence number, flags) and its IPv4 and L4 checksums computed here, over bytes
// the copy moves anyway.  A packet that only needs its checksum completed (CSUM) and a plain one ride along.
//
// Work division: a wave takes 64 consecutive slots a pass, in two phases, and a grid-stride loop of at most
// kGsoMaxBlocks workgroups of four waves walks the batch -- gro_resolve_kernel's shape.
//   Resolve: one lane a slot, 64 independent chains in flight a wave (the finding recorded in frames_kernels.hip:
//   the lookup is never a copy lane's).  The slot's entry by gso_find (gso_core.h: gro_find over this table), the
//   validity rule, k, P_k and the payload's place, the destination address -- Packet[16:20] lies in the header
//   every segment shares, the aligned dword at packed + off + 16 -- the probe of the route table (route_core.h),
//   then lens, peer and the descriptor as coalesced stores.  A slot no entry names writes nothing.
//   Copy: kGroLanes = 16 lanes a slot, four slots at a time, 16 turns; the lanes of a slot read its five words of
//   state from the lane that resolved it (ds_bpermute through __shfl, no LDS allocation, no barrier).
//
// The payload copy is gro_copy.h's realignment with a start offset inside the slot.  The payload source off +
// hdr_len + k * gso_size has any alignment, its destination slot + 4 + hdr_len is dword-aligned.  Wide path
// (stride and arena 16-B aligned): the lanes divide the slot by destination granule from the one that holds the
// payload's first byte; a granule is two aligned 16-byte loads that straddle its source bytes -- each issued only
// when it holds a payload byte the granule needs, so nothing is read outside [off, off + len) rounded out to
// 16-byte boundaries -- the dword select and v_alignbyte_b32, and one aligned 16-byte store, or dwords and at most
// three single bytes in the first and the last granule.  Dword path: the same a dword at a time.  No byte loads.
//
// Checksums.  A ones'-complement sum does not care about byte order, so everything is summed as the little-endian
// dwords the lanes hold, 32 bits wide with the carry brought round, and folded to 16 bits at the end.  A lane adds
// every destination dword it has realigned, bytes outside the payload masked to zero (which also pads an odd
// payload), whether or not the slot's clamp lets it store them: the checksum is the whole packet's.  The header's
// dwords (at most 30) belong to lanes g and g + 16 of the slot: each loads its two from the frame, patches them
// with the checksum fields zero and adds them to the IPv4 sum or the L4 sum (addresses to both: the pseudo-header),
// lane 0 adds protocol and L4 length.  Both sums go round the slot's 16 lanes with four __shfl_xor steps each, so
// every lane holds the totals, and the lanes that own the checksum dwords put them in.  The header is written
// last, a dword a lane, consecutive lanes consecutive dwords; no lane stores a dword another lane stores.  A CSUM
// packet's field lies inside the copied bytes: the lane that meets its dword keeps it in a register instead of
// storing it, and stores it with the field filled once the sum is known.  No LDS, no barrier, no atomics.
//
// The shuffles are executed by all 64 lanes: nothing between the top of a turn and its last shuffle leaves early,
// a slot without work is a slot of zero bytes.
//
// Memory safety on any table: gso_find reads the table below n_frames; an entry that is not valid (gso_core.h,
// from the entry alone) reads and writes no byte of packed area or arena; of a valid one every load holds a byte
// of [off, off + len) with off + len <= packed_len and lies on its boundary, so no read passes the 16-byte boundary
// behind packed_len; every store lies below min(4 + L, stride) of slot i < first + count <= n.  A slot is a function
// of its index -- lane i alone decides from which entry slot i is written -- so there is no write-write race on a
// table that does not ascend.
//
// Tried: this form only.  2^20 slots of 1536 bytes against frames_resolve_kernel on the same packets already
// segmented: 994.5 against 782.8 us from 45-segment TCP frames of gso_size 1348, 896.1 against 691.7 from mixed
// frames, 304.9 against 224.0 from lone 64-byte PLAIN entries -- slower in every round; the host pipeline is level
// (66.31 against 66.35 ms at 2^20 packets).  95 VGPRs on the 16-byte path, 80 on the dword path, no
// scratch: 5 and 6 waves a SIMD where frames_resolve_kernel has 7 and gro_resolve_kernel, whose copy this is, 8; a
// bound of 7 waves spills 72 bytes a lane.  Eight lanes a slot with several granules in flight, and the IPv4
// header's sum taken once by the resolving lane, are not measured.
#include "gcm_internal.h"
#include "gro_copy.h"
#include "gso_core.h"
#include "route_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kGsoThreads = 256;
constexpr uint32_t kGsoWave = 64;                       // slots of one wave per pass
constexpr uint32_t kGsoGroups = kGsoWave / kGroLanes;   // slots copied at a time
constexpr uint32_t kGsoTurns = kGsoWave / kGsoGroups;   // turns of the copy
constexpr uint32_t kGsoWaves = kGsoThreads / kGsoWave;  // waves of one workgroup
// 8192 waves, as frames_resolve_kernel's grid; the grid-stride loop takes batches of more than 2^19 slots
constexpr uint32_t kGsoMaxBlocks = 2048;

// what a copy lane knows of its slot (the five words shuffled from the resolving lane, taken apart)
enum GsoMode : uint32_t { kNone = 0, kPlain = 1, kCsum = 2, kTcp = 3, kUdp = 4 };

// a + b with the carry brought round: the ones'-complement sum, 32 bits wide
__device__ __forceinline__ uint32_t add1c(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s + (s < b);
}

__device__ __forceinline__ uint32_t fold_not16(uint32_t s) {
    s = (s & 0xffffu) + (s >> 16);
    s = (s & 0xffffu) + (s >> 16);
    return ~s & 0xffffu;
}

__device__ __forceinline__ uint32_t swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }

// the sum over the slot's kGroLanes lanes, in every one of them
__device__ __forceinline__ uint32_t sum_lanes(uint32_t v) {
#pragma unroll
    for (uint32_t m = kGroLanes / 2; m; m >>= 1) v = add1c(v, (uint32_t)__shfl_xor((int)v, (int)m, (int)kGroLanes));
    return v;
}

struct SegCopy {
    uint8_t *slot;
    uint32_t from;             // slot bytes [from, to) take the payload: from = 4 + hdr_len, below 2^8
    uint64_t to, limit;        // ... and only those below limit are stored
    uint32_t sum_from;         // slot bytes [sum_from, to) are summed: from, or 4 + l4_off, below 2^17
    uint32_t field;            // the dword (slot byte, a multiple of 4) that is kept back, or ~0
    uint32_t sum = 0, kept = 0;
    bool has_kept = false;

    // destination dword at slot byte x (a multiple of 4; x + 4 > from, x < to) realigned as w
    __device__ __forceinline__ void dword(uint64_t x, uint32_t w) {
        if (x + 4 > sum_from) {
            uint32_t m = ~0u;
            if (x < sum_from) m &= ~0u << (8 * (uint32_t)(sum_from - x));
            if (to - x < 4) m &= ~(~0u << (8 * (uint32_t)(to - x)));
            sum = add1c(sum, w & m);
        }
        if (x < from || x >= limit) return;
        if (x == field) {
            kept = w;
            has_kept = true;
            return;
        }
        const uint64_t end = to < limit ? to : limit;
        if (end - x >= 4)
            *reinterpret_cast<uint32_t *>(slot + x) = w;
        else
            store_tail_bytes(slot + x, w, (uint32_t)(end - x));
    }
};

// slot bytes [c.from, c.to) from s0 + [c.from, c.to) (s0: the address slot byte 0 would come from, any alignment)
// by the kGroLanes lanes of the slot, lane g of them; slot 16-B aligned
__device__ __forceinline__ void copy_seg16(SegCopy &c, uintptr_t s0, uint32_t g) {
    if (c.from >= c.to) return;  // nothing to copy: no piece holds a byte that is needed, so none is loaded
    const uint32_t sh = (uint32_t)(s0 & 15u);
    const bool q2 = sh & 8u, q1 = sh & 4u;
    const uint32_t r = sh & 3u;
    for (uint64_t at = 16 * (uint64_t)((c.from >> 4) + g); at < c.to; at += 16 * kGroLanes) {
        const uint64_t need_lo = at > c.from ? at : (uint64_t)c.from, need_hi = at + 16 < c.to ? at + 16 : c.to;
        const uintptr_t blk = s0 + at - sh;  // the 16-byte piece that holds the source of slot byte `at`
        uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
        if (s0 + need_lo < blk + 16) lo = *reinterpret_cast<const uint4 *>(blk);
        if (s0 + need_hi > blk + 16) hi = *reinterpret_cast<const uint4 *>(blk + 16);
        // dwords q .. q + 4 of {lo, hi}, q = sh >> 2
        const uint32_t a0 = q2 ? lo.z : lo.x, a1 = q2 ? lo.w : lo.y, a2 = q2 ? hi.x : lo.z, a3 = q2 ? hi.y : lo.w,
                       a4 = q2 ? hi.z : hi.x, a5 = q2 ? hi.w : hi.y;
        const uint32_t b0 = q1 ? a1 : a0, b1 = q1 ? a2 : a1, b2 = q1 ? a3 : a2, b3 = q1 ? a4 : a3, b4 = q1 ? a5 : a4;
        const uint4 out = make_uint4(funnel(b1, b0, r), funnel(b2, b1, r), funnel(b3, b2, r), funnel(b4, b3, r));
        if (at >= c.from && at >= c.sum_from && at + 16 <= c.to && at + 16 <= c.limit && (c.field & ~15u) != at) {
            c.sum = add1c(add1c(c.sum, out.x), add1c(out.y, add1c(out.z, out.w)));
            *reinterpret_cast<uint4 *>(c.slot + at) = out;
        } else {
            if (at + 4 > c.from) c.dword(at, out.x);
            if (at + 8 > c.from && at + 4 < c.to) c.dword(at + 4, out.y);
            if (at + 12 > c.from && at + 8 < c.to) c.dword(at + 8, out.z);
            if (at + 12 < c.to) c.dword(at + 12, out.w);
        }
    }
}

// the same in dwords, for a slot that is only 4-B aligned
__device__ __forceinline__ void copy_seg4(SegCopy &c, uintptr_t s0, uint32_t g) {
    if (c.from >= c.to) return;
    const uint32_t sh = (uint32_t)(s0 & 3u);
    for (uint64_t at = 4 * (uint64_t)((c.from >> 2) + g); at < c.to; at += 4 * kGroLanes) {
        const uint64_t need_lo = at > c.from ? at : (uint64_t)c.from, need_hi = at + 4 < c.to ? at + 4 : c.to;
        const uintptr_t blk = s0 + at - sh;
        uint32_t lo = 0, hi = 0;
        if (s0 + need_lo < blk + 4) lo = *reinterpret_cast<const uint32_t *>(blk);
        if (s0 + need_hi > blk + 4) hi = *reinterpret_cast<const uint32_t *>(blk + 4);
        c.dword(at, funnel(hi, lo, sh));
    }
}

// what a lane needs to patch a header dword of a TCP4 / UDP4 segment
struct HdrPatch {
    const uint32_t *hdr;  // the frame's header: packed + off, 16-B aligned
    uint32_t words, j0;   // hdr_len / 4, l4_off / 4
    uint32_t len16, l4len16, k, seq_add;
    bool tcp, last;

    // dword j (j < words) patched, its checksum field zero; added to the sums it belongs to
    __device__ __forceinline__ uint32_t word(uint32_t j, uint32_t &ip_sum, uint32_t &l4_sum) const {
        uint32_t w = hdr[j];
        if (j == 0) {
            w = (w & 0xffffu) | swap16(len16) << 16;
        } else if (j == 1) {
            w = (w & 0xffff0000u) | swap16((swap16(w) + k) & 0xffffu);
        } else if (j == 2) {
            w &= 0xffffu;
        } else if (tcp) {
            if (j == j0 + 1)
                w = __builtin_bswap32(__builtin_bswap32(w) + seq_add);
            else if (j == j0 + 3 && !last)
                w &= ~0x0900u;  // FIN and PSH, byte 13 of the TCP header
            else if (j == j0 + 4)
                w &= 0xffff0000u;
        } else if (j == j0 + 1) {
            w = swap16(l4len16);
        }
        if (j < j0) ip_sum = add1c(ip_sum, w);
        if (j >= j0 || j == 3 || j == 4) l4_sum = add1c(l4_sum, w);
        return w;
    }
};

template <bool kWide>
__global__ void __launch_bounds__(kGsoThreads) gso_resolve_kernel(GsoArgs a) {
    const uint32_t lane = threadIdx.x % kGsoWave, g = lane % kGroLanes, q = lane / kGroLanes;
    const uint64_t waves = (uint64_t)gridDim.x * kGsoWaves;
    for (uint64_t base = ((uint64_t)blockIdx.x * kGsoWaves + threadIdx.x / kGsoWave) * kGsoWave; base < a.n; base += waves * kGsoWave) {
        // resolve: lane `lane` has slot base + lane
        const uint64_t i = base + lane;
        // the slot's state for its copy lanes: the frame's place, the payload's place in it and its bytes (the
        // whole packet for PLAIN and CSUM), k | last << 11 | hit << 12 | mode << 13 | hdr_len << 16, l4_off |
        // csum_off << 16.  Mode kNone: an unnamed slot, a void entry and every slot at or past n
        uint32_t s_off = 0, s_rel = 0, s_bytes = 0, s_info = 0, s_l4 = 0;
        if (i < a.n) {
            const qgcm_gso_frame f = a.frames[gso_find(a.frames, a.n_frames, a.n, i)];
            const bool valid = gso_valid(f, a.packed_len, a.n);
            const uint64_t slot_off = i * a.stride;
            if (valid && i >= f.first && i - f.first < f.count) {
                const uint32_t k = (uint32_t)(i - f.first);
                uint32_t mode, len, hdr = 0;
                if (f.kind == QGCM_GSO_PLAIN || f.kind == QGCM_GSO_CSUM) {
                    mode = f.kind == QGCM_GSO_PLAIN ? kPlain : kCsum;
                    len = s_bytes = f.len;
                } else {
                    mode = f.kind == QGCM_GSO_TCP4 ? kTcp : kUdp;
                    hdr = f.hdr_len;
                    s_bytes = gso_seg_payload(f, k);
                    s_rel = hdr + k * (uint32_t)f.gso_size;
                    len = hdr + s_bytes;
                }
                uint32_t peer = QGCM_NO_PEER;
                // Packet[16:20] must exist, and the sealed datagram must fit the slot (route_resolve_kernel's rule);
                // f.len >= len >= 20, so the dword lies inside the frame
                if (len >= 20 && 4ull + len + QGCM_OVERHEAD <= a.stride) {
                    const uint32_t addr = *reinterpret_cast<const uint32_t *>(a.packed + f.off + 16);
                    const uint32_t key = ((addr ^ a.net) & a.mask) == 0 ? addr : a.gateway;  // router.go:25-30
                    peer = route_lookup(a.table, a.cap_mask, key);
                }
                s_off = f.off;
                s_info = k | (uint32_t)(k + 1 == f.count) << 11 | (uint32_t)(peer != QGCM_NO_PEER) << 12 | mode << 13 | hdr << 16;
                s_l4 = f.l4_off | (uint32_t)f.csum_off << 16;
                a.lens[i] = len;
                a.peer[i] = peer;
                *reinterpret_cast<uint4 *>(a.descs + i) = make_uint4((uint32_t)slot_off, (uint32_t)(slot_off >> 32), len, peer);
            } else if (!valid && i == f.first && f.count >= 1) {
                // a void entry: a packet of length 0 that no route resolves; its slot is not touched
                a.lens[i] = 0;
                a.peer[i] = QGCM_NO_PEER;
                *reinterpret_cast<uint4 *>(a.descs + i) = make_uint4((uint32_t)slot_off, (uint32_t)(slot_off >> 32), 0, QGCM_NO_PEER);
            }
        }
        // copy: turn t takes slots base + kGsoGroups t + q, q = 0..kGsoGroups-1, kGroLanes lanes each
        for (uint32_t t = 0; t < kGsoTurns; ++t) {
            const uint32_t src_lane = kGsoGroups * t + q;
            const uint32_t f_off = __shfl(s_off, src_lane, kGsoWave), f_rel = __shfl(s_rel, src_lane, kGsoWave);
            const uint32_t f_bytes = __shfl(s_bytes, src_lane, kGsoWave), f_info = __shfl(s_info, src_lane, kGsoWave);
            const uint32_t f_l4 = __shfl(s_l4, src_lane, kGsoWave);
            const uint32_t mode = (f_info >> 13) & 7u, hdr = f_info >> 16, l4_off = f_l4 & 0xffffu;
            const bool hit = f_info & (1u << 12), split = mode >= kTcp;
            uint8_t *slot = a.arena + (base + src_lane) * a.stride;  // dereferenced under a mode only
            SegCopy c;
            c.slot = slot;
            c.from = (uint32_t)kGsoPacketStart + hdr;
            c.to = mode == kNone ? c.from : (uint64_t)c.from + f_bytes;  // (a slot without work: an empty range)
            c.limit = a.stride;
            c.sum_from = mode == kCsum ? (uint32_t)kGsoPacketStart + l4_off : c.from;
            c.field = mode == kCsum ? ((uint32_t)kGsoPacketStart + l4_off + (f_l4 >> 16)) & ~3u : ~0u;
            const uintptr_t s0 = (uintptr_t)a.packed + f_off + f_rel - c.from;
            if (kWide)
                copy_seg16(c, s0, g);
            else
                copy_seg4(c, s0, g);
            // the header's dwords g and g + 16, patched, and what they add to the sums
            uint32_t ip_sum = 0, l4_sum = c.sum, h0 = 0, h1 = 0;
            HdrPatch p;
            p.hdr = reinterpret_cast<const uint32_t *>(a.packed + f_off);
            p.words = split ? hdr >> 2 : 0;
            p.j0 = l4_off >> 2;
            p.len16 = (hdr + f_bytes) & 0xffffu;
            p.l4len16 = (hdr + f_bytes - l4_off) & 0xffffu;
            p.k = f_info & 0x7ffu;
            p.seq_add = f_rel - hdr;  // k * gso_size
            p.tcp = mode == kTcp;
            p.last = f_info & (1u << 11);
            if (g < p.words) h0 = p.word(g, ip_sum, l4_sum);
            if (g + kGroLanes < p.words) h1 = p.word(g + kGroLanes, ip_sum, l4_sum);
            // the pseudo-header's protocol and L4 length
            if (g == 0 && split) l4_sum = add1c(l4_sum, (p.tcp ? 6u : 17u) << 8 | swap16(p.l4len16) << 16);
            ip_sum = sum_lanes(ip_sum);
            l4_sum = sum_lanes(l4_sum);
            uint32_t l4_c = fold_not16(l4_sum);
            if (mode != kTcp && l4_c == 0) l4_c = 0xffffu;
            if (c.has_kept) {
                // the CSUM packet's field, in the low or the high half of its dword
                const uint32_t w = (kGsoPacketStart + l4_off + (f_l4 >> 16)) & 2u ? (c.kept & 0xffffu) | l4_c << 16
                                                                                 : (c.kept & 0xffff0000u) | l4_c;
                const uint64_t end = c.to < c.limit ? c.to : c.limit;
                if (end - c.field >= 4)
                    *reinterpret_cast<uint32_t *>(slot + c.field) = w;
                else
                    store_tail_bytes(slot + c.field, w, (uint32_t)(end - c.field));
            }
            if (split) {
                const uint32_t at_csum = p.tcp ? p.j0 + 4 : p.j0 + 1;
                const uint32_t put = p.tcp ? l4_c : l4_c << 16;
                if (g == 2) h0 |= fold_not16(ip_sum) << 16;
                if (g == at_csum) h0 |= put;
                if (g + kGroLanes == at_csum) h1 |= put;
                // a header dword is stored whole or not at all: hdr_len and stride are multiples of 4
                if (g < p.words && kGsoPacketStart + 4ull * g < c.limit) reinterpret_cast<uint32_t *>(slot + kGsoPacketStart)[g] = h0;
                if (g + kGroLanes < p.words && kGsoPacketStart + 4ull * (g + kGroLanes) < c.limit)
                    reinterpret_cast<uint32_t *>(slot + kGsoPacketStart)[g + kGroLanes] = h1;
            }
            if (g == 0 && hit) *reinterpret_cast<uint32_t *>(slot) = a.own_ip;  // outgoing.go:30
        }
    }
}

}  // namespace

hipError_t launch_gso_resolve(const GsoArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_frames == 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)a.n + kGsoThreads - 1) / kGsoThreads;
    const dim3 grid((uint32_t)(blocks < kGsoMaxBlocks ? blocks : kGsoMaxBlocks));
    if ((a.stride & 15) == 0 && ((uintptr_t)a.arena & 15) == 0)
        hipLaunchKernelGGL(gso_resolve_kernel<true>, grid, dim3(kGsoThreads), 0, s, a);
    else
        hipLaunchKernelGGL(gso_resolve_kernel<false>, grid, dim3(kGsoThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
