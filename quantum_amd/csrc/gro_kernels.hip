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
#include "gro_copy.h"  // kGroLanes, copy_slot16, copy_slot4: shared with gro_resolve_kernels.hip
#include "gro_core.h"

namespace qgcm {
namespace {

constexpr uint32_t kGroThreads = 256;
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

template <bool kWide>
__global__ void __launch_bounds__(kGroThreads) gro_unpack_kernel(GroArgs a) {
    const uint32_t g = threadIdx.x % kGroLanes;
    for (uint64_t i = (uint64_t)blockIdx.x * kGroSlots + threadIdx.x / kGroLanes; i < a.n;
         i += (uint64_t)gridDim.x * kGroSlots) {
        const uint32_t lo = gro_find(a.bufs, a.n_bufs, a.n, i);  // gro_core.h
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
