// gro_kernels.hip -- coalesced receive buffers unpacked into slots (include/qgcm.h "coalesced receive on
// routed batches").
//
// A segmented copy from arbitrarily aligned sources to aligned slots: datagram k of a buffer starts at
// off + k * seg_len of the packed area, so with a seg_len of 1382 the source walks through every even
// residue of 16 while every slot starts on its boundary.
//
// Work division: kGroLanes = 16 lanes per slot, four slots per wave, 16 slots per workgroup, a grid-stride
// loop over the slots.  16 lanes move 256 B per pass: a 1382-byte datagram is 87 pieces of 16 B in six
// passes (91 % of the lanes busy; a whole wave per slot would leave a third of its second pass idle), a
// 64-byte one keeps 4 of its 16 lanes busy where a wave per slot would keep 4 of 64.  Every slot finds its
// buffer by a search over `first` (ascending in every table the receive call writes; n_bufs <= n, the table
// is small against the bytes and stays in cache), the same steps for the 16 lanes of a slot: a first guess
// at i * n_bufs / n, exact for buffers of equal counts (whole trains, or lone datagrams), a bracket grown
// from there in doubling steps, then a binary search inside it -- two table reads where the guess is right,
// against log2(n_bufs) dependent ones from a plain binary search, which cost lone 64-byte datagrams 240 us
// per 2^20 against 93-95 us now.
// A table whose `first` values do not ascend stays memory-safe -- every index is checked against
// n_bufs, every source byte against packed_len, every slot against n -- and which of its slots are written
// is then unspecified.
//
// 16-byte path (stride and arena 16-B aligned): per piece two aligned 16-byte loads that straddle the
// source bytes, realigned in registers -- a dword select for bits 2-3 of the source address, the byte-align
// funnel shift (v_alignbyte_b32) for bits 0-1 -- and one aligned 16-byte store.  The second load is the next
// lane's first, so it is served on chip.  It is issued only when a byte of it is needed, which keeps every
// read below the 16-byte boundary behind the buffer's end.  The last piece of a datagram stores its whole
// dwords and then at most three single bytes, so the slot's tail keeps its bytes.  No byte loads.
// Dword path (a stride that is only a multiple of 4): the same with aligned dword loads and stores.
#include "gcm_internal.h"
#include "gro_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kGroThreads = 256;
constexpr uint32_t kGroLanes = 16;                          // lanes of one slot
constexpr uint32_t kGroSlots = kGroThreads / kGroLanes;     // slots of one workgroup per pass
// twice the threads the 256 CUs hold at once; the grid-stride loop takes batches of more than 65536 slots
constexpr uint32_t kGroMaxBlocks = 4096;

struct GroArgs {
    const uint8_t *packed;
    uint64_t packed_len;
    const qgcm_gro_buf *bufs;
    uint32_t n_bufs, n;
    uint8_t *arena;
    uint64_t stride;
    uint32_t *lens;
};

// ({hi, lo} >> 8 * (shift & 3)) & 0xffffffff
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t shift) {
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
}

// the last `nb` (1..3) bytes of a piece, from the low end of w
__device__ __forceinline__ void store_tail_bytes(uint8_t *dst, uint32_t w, uint32_t nb) {
    dst[0] = (uint8_t)w;
    if (nb > 1) dst[1] = (uint8_t)(w >> 8);
    if (nb > 2) dst[2] = (uint8_t)(w >> 16);
}

// bytes [0, bytes) of dst (16-B aligned) from src (any alignment; src - (src & 15) is 16-B aligned), by the
// kGroLanes lanes of a slot, lane g of them
__device__ __forceinline__ void copy_slot16(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes,
                                            uint32_t g) {
    const uint32_t sh = (uint32_t)((uintptr_t)src & 15u);
    const uint4 *__restrict__ s16 = reinterpret_cast<const uint4 *>(src - sh);
    const bool q2 = sh & 8u, q1 = sh & 4u;
    const uint32_t r = sh & 3u;
    for (uint32_t at = 16 * g; at < bytes; at += 16 * kGroLanes) {
        const uint32_t nb = bytes - at < 16 ? bytes - at : 16;
        const uint4 lo = s16[at >> 4];
        uint4 hi = make_uint4(0, 0, 0, 0);
        if (sh + nb > 16) hi = s16[(at >> 4) + 1];
        // dwords q .. q + 4 of {lo, hi}, q = sh >> 2
        const uint32_t a0 = q2 ? lo.z : lo.x, a1 = q2 ? lo.w : lo.y, a2 = q2 ? hi.x : lo.z, a3 = q2 ? hi.y : lo.w,
                       a4 = q2 ? hi.z : hi.x, a5 = q2 ? hi.w : hi.y;
        const uint32_t b0 = q1 ? a1 : a0, b1 = q1 ? a2 : a1, b2 = q1 ? a3 : a2, b3 = q1 ? a4 : a3, b4 = q1 ? a5 : a4;
        const uint4 out = make_uint4(funnel(b1, b0, r), funnel(b2, b1, r), funnel(b3, b2, r), funnel(b4, b3, r));
        uint8_t *d = dst + at;
        if (nb == 16) {
            *reinterpret_cast<uint4 *>(d) = out;
        } else {
            uint32_t *d32 = reinterpret_cast<uint32_t *>(d);
            const uint32_t whole = nb >> 2;
            if (whole > 0) d32[0] = out.x;
            if (whole > 1) d32[1] = out.y;
            if (whole > 2) d32[2] = out.z;
            if (nb & 3u) store_tail_bytes(d + 4 * whole, whole == 0 ? out.x : whole == 1 ? out.y : whole == 2 ? out.z : out.w, nb & 3u);
        }
    }
}

// the same in dwords, for a dst that is only 4-B aligned
__device__ __forceinline__ void copy_slot4(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes,
                                           uint32_t g) {
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(src - sh);
    for (uint32_t at = 4 * g; at < bytes; at += 4 * kGroLanes) {
        const uint32_t nb = bytes - at < 4 ? bytes - at : 4;
        const uint32_t lo = s4[at >> 2];
        uint32_t hi = 0;
        if (sh + nb > 4) hi = s4[(at >> 2) + 1];
        const uint32_t out = funnel(hi, lo, sh);
        if (nb == 4)
            *reinterpret_cast<uint32_t *>(dst + at) = out;
        else
            store_tail_bytes(dst + at, out, nb);
    }
}

template <bool kWide>
__global__ void __launch_bounds__(kGroThreads) gro_unpack_kernel(GroArgs a) {
    const uint32_t g = threadIdx.x % kGroLanes;
    for (uint64_t i = (uint64_t)blockIdx.x * kGroSlots + threadIdx.x / kGroLanes; i < a.n;
         i += (uint64_t)gridDim.x * kGroSlots) {
        // the last buffer whose first is at or below i, kept in [lo, hi): bufs[lo].first <= i unless lo is 0,
        // bufs[hi].first > i unless hi is n_bufs.  Buffers of equal counts would put slot i into buffer
        // i * n_bufs / n; the bracket is grown from there in doubling steps, then halved.
        uint32_t lo = 0, hi = a.n_bufs;
        const uint32_t guess = (uint32_t)(i * a.n_bufs / a.n);
        if (a.bufs[guess].first <= i) {
            lo = guess;
            uint32_t step = 1;
            while (hi - lo > step && a.bufs[lo + step].first <= i) {
                lo += step;
                step <<= 1;
            }
            if (hi - lo > step) hi = lo + step;
        } else {
            hi = guess;
            uint32_t step = 1;
            while (step <= hi && a.bufs[hi - step].first > i) {
                hi -= step;
                step <<= 1;
            }
            lo = step <= hi ? hi - step : 0;
        }
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (a.bufs[mid].first <= i)
                lo = mid;
            else
                hi = mid;
        }
        const qgcm_gro_buf b = a.bufs[lo];
        const uint64_t count = gro_count(b.len, b.seg_len);
        if (i < b.first || i - b.first >= count || gro_buf_skipped(b, count, a.packed_len, a.n)) continue;
        const uint64_t k = i - b.first;
        const uint32_t L = gro_seg_bytes(b.len, b.seg_len, count, k);
        if (g == 0) a.lens[i] = L;
        const uint32_t bytes = L < a.stride ? L : (uint32_t)a.stride;
        const uint8_t *src = a.packed + b.off + k * b.seg_len;
        uint8_t *dst = a.arena + i * a.stride;
        if (kWide)
            copy_slot16(dst, src, bytes, g);
        else
            copy_slot4(dst, src, bytes, g);
    }
}

}  // namespace

hipError_t launch_gro_unpack(const uint8_t *packed, uint64_t packed_len, const qgcm_gro_buf *bufs, uint32_t n_bufs,
                             uint32_t n, uint8_t *arena, uint64_t stride, uint32_t *lens, hipStream_t s) {
    if (n == 0 || n_bufs == 0) return hipSuccess;
    GroArgs a{packed, packed_len, bufs, n_bufs, n, arena, stride, lens};
    const uint64_t blocks = ((uint64_t)n + kGroSlots - 1) / kGroSlots;
    const dim3 grid((uint32_t)(blocks < kGroMaxBlocks ? blocks : kGroMaxBlocks));
    if ((stride & 15) == 0 && ((uintptr_t)arena & 15) == 0)
        hipLaunchKernelGGL(gro_unpack_kernel<true>, grid, dim3(kGroThreads), 0, s, a);
    else
        hipLaunchKernelGGL(gro_unpack_kernel<false>, grid, dim3(kGroThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace qgcm
