// gro_resolve_kernels.hip -- coalesced receive buffers unpacked into slots and resolved in one launch
// (include/qgcm.h "coalesced receive on routed batches").
//
// The fusion of gro_unpack_kernel (gro_kernels.hip) and route_resolve_kernel<incoming> (route_kernels.hip).  The
// pair's second launch reads one dword at slot + 0 of every slot the first has just written; here the sender's
// address is taken from the packed area, where it is the first four bytes of the datagram, before the copy, so
// the slots are only written, and lens, peer and descs are coalesced stores.
//
// Work division: a wave takes 64 consecutive slots a pass, in two phases, and a grid-stride loop of at most
// kGrrMaxBlocks workgroups of four waves walks the batch.
//   Resolve: one lane a slot, 64 independent chains in flight a wave.  The slot's buffer by gro_find
//   (gro_core.h: the search gro_unpack_kernel runs), then k, L and the source offset, the header, the probe of
//   the route table (route_core.h: the code route_resolve_kernel runs), then lens (named slots only), peer and
//   the descriptor as one 16-byte store.  A slot that no unskipped buffer names keeps its length and its bytes
//   and is resolved from them, as the pair's second launch would: its header is the aligned dword at slot + 0.
//   Copy: kGroLanes = 16 lanes a slot, four slots at a time, 16 turns; the lanes of a slot read its source offset
//   (in two halves: off + k * seg_len can pass 32 bits) and its byte count from the lane that resolved it
//   (ds_bpermute through __shfl, no LDS allocation, no barrier).  An unnamed slot has a byte count of 0.  The
//   copy itself is gro_unpack_kernel's (gro_copy.h): copy_slot16 where stride and arena are 16-B aligned, else
//   copy_slot4.
//
// The header load.  A named datagram is readable when 4 <= L <= stride; its header is bytes [src, src + 4) of
// the packed area, src = off + k * seg_len at any alignment: one aligned dword load at src & ~3, a second at
// (src & ~3) + 4 only when src & 3, the two combined with v_alignbyte_b32.  L >= 4 puts src + 3 below
// off + len <= packed_len (the buffer is not skipped), and an aligned dword never crosses a 16-byte boundary, so
// both dwords -- the one that holds byte src and, when src & 3, the one that holds byte src + 3 -- lie below the
// 16-byte boundary behind packed_len, inside the rounded-up allocation the caller promises.  No test can see an
// over-read inside a caching allocator's block: this argument is the check.
//
// Memory safety on any table: gro_find reads the table below n_bufs only; a slot is named only when its buffer
// is not skipped (off + len <= packed_len, first + count <= n), so every copied byte lies below packed_len and
// copy_slot16 / copy_slot4 keep their reads below the 16-byte boundary behind it; every store goes to slot i < n
// or to entry i < n of lens, peer, descs.  A slot is a function of its index -- lane i decides alone from which
// buffer slot i is written -- so there is no write-write race even on a table that does not ascend.  No atomics,
// no LDS, no scratch.
//
// Tried: this form only -- 16 lanes a slot and one granule in flight a lane, what gro_unpack_kernel has.  2^20
// datagrams into slots of 1536 bytes against the pair of launches: 786.0 against 792.4 us at 1382 bytes in
// 45-segment buffers (the unpack alone 648.0), 534.2 against 546.0 for lengths 64..1472, 179.1 against 215.7 for
// lone 64-byte datagrams; but the host pipeline, whose chunks are 65536 slots -- 1024 waves here, 16384 for the
// unpack -- measured 1-2 % slower with it, so the pipelines run it only under QGCM_GRO_FUSED=1.
// Fewer lanes a slot (eight, as frames_resolve_kernel) and several loads in flight before the first store are
// not measured.
#include "gcm_internal.h"
#include "gro_copy.h"
#include "gro_core.h"
#include "route_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kGrrThreads = 256;
constexpr uint32_t kGrrWave = 64;                        // slots of one wave per pass
constexpr uint32_t kGrrGroups = kGrrWave / kGroLanes;    // slots copied at a time
constexpr uint32_t kGrrTurns = kGrrWave / kGrrGroups;    // turns of the copy
constexpr uint32_t kGrrWaves = kGrrThreads / kGrrWave;   // waves of one workgroup
// 8192 waves, as frames_resolve_kernel's grid; the grid-stride loop takes batches of more than 2^19 slots
constexpr uint32_t kGrrMaxBlocks = 2048;

template <bool kWide>
__global__ void __launch_bounds__(kGrrThreads) gro_resolve_kernel(GroResolveArgs a) {
    const uint32_t lane = threadIdx.x % kGrrWave, g = lane % kGroLanes, q = lane / kGroLanes;
    const uint64_t waves = (uint64_t)gridDim.x * kGrrWaves;
    for (uint64_t base = ((uint64_t)blockIdx.x * kGrrWaves + threadIdx.x / kGrrWave) * kGrrWave; base < a.n; base += waves * kGrrWave) {
        // resolve: lane `lane` has slot base + lane
        const uint64_t i = base + lane;
        uint64_t src = 0;
        uint32_t bytes = 0;  // to copy: 0 for an unnamed slot, an empty datagram and every slot at or past n
        if (i < a.n) {
            const qgcm_gro_buf b = a.bufs[gro_find(a.bufs, a.n_bufs, a.n, i)];
            const uint64_t count = gro_count(b.len, b.seg_len);
            const bool named = i >= b.first && i - b.first < count && !gro_buf_skipped(b, count, a.packed_len, a.n);
            const uint64_t slot_off = i * a.stride;
            uint32_t len, addr = 0;
            bool readable;
            if (named) {
                const uint64_t k = i - b.first;
                len = gro_seg_bytes(b.len, b.seg_len, count, k);
                src = b.off + k * b.seg_len;
                bytes = len < a.stride ? len : (uint32_t)a.stride;
                readable = len >= 4 && len <= a.stride;
                if (readable) {
                    // bytes [src, src + 4): src + 3 < off + len <= packed_len (the header comment)
                    const uint32_t r = (uint32_t)src & 3u;
                    const uint32_t *w = reinterpret_cast<const uint32_t *>(a.packed + (src - r));
                    const uint32_t w0 = w[0];
                    uint32_t w1 = 0;
                    if (r) w1 = w[1];
                    addr = funnel(w1, w0, r);
                }
                a.lens[i] = len;
            } else {
                len = a.lens[i];
                readable = len >= 4 && len <= a.stride;
                if (readable) addr = *reinterpret_cast<const uint32_t *>(a.arena + slot_off);
            }
            uint32_t peer = QGCM_NO_PEER;
            if (readable) {
                const uint32_t key = ((addr ^ a.net) & a.mask) == 0 ? addr : a.gateway;  // router.go:25-30
                peer = route_lookup(a.table, a.cap_mask, key);
            }
            a.peer[i] = peer;
            *reinterpret_cast<uint4 *>(a.descs + i) =
                make_uint4((uint32_t)slot_off, (uint32_t)(slot_off >> 32), len >= 4 ? len - 4 : 0, peer);
        }
        // copy: turn t takes slots base + kGrrGroups t + q, q = 0..kGrrGroups-1, kGroLanes lanes each
        const uint32_t src_lo = (uint32_t)src, src_hi = (uint32_t)(src >> 32);
        for (uint32_t t = 0; t < kGrrTurns; ++t) {
            const uint32_t from = kGrrGroups * t + q;
            const uint32_t f_lo = __shfl(src_lo, from, kGrrWave), f_hi = __shfl(src_hi, from, kGrrWave);
            const uint32_t f_bytes = __shfl(bytes, from, kGrrWave);
            if (f_bytes == 0) continue;
            const uint8_t *from_src = a.packed + (((uint64_t)f_hi << 32) | f_lo);
            uint8_t *dst = a.arena + (base + from) * a.stride;
            if (kWide)
                copy_slot16(dst, from_src, f_bytes, g);
            else
                copy_slot4(dst, from_src, f_bytes, g);
        }
    }
}

}  // namespace

hipError_t launch_gro_resolve(const GroResolveArgs &a, hipStream_t s) {
    if (a.n == 0 || a.n_bufs == 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)a.n + kGrrThreads - 1) / kGrrThreads;
    const dim3 grid((uint32_t)(blocks < kGrrMaxBlocks ? blocks : kGrrMaxBlocks));
    if ((a.stride & 15) == 0 && ((uintptr_t)a.arena & 15) == 0)
        hipLaunchKernelGGL(gro_resolve_kernel<true>, grid, dim3(kGrrThreads), 0, s, a);
    else
        hipLaunchKernelGGL(gro_resolve_kernel<false>, grid, dim3(kGrrThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
