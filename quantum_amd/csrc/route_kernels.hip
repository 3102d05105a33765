// route_kernels.hip -- the router and the link metrics of a packet batch on gfx950 (include/qgcm.h "routes
// resolved on the GPU").
//
// route_resolve_kernel: one lane per packet.  worker/outgoing.go:28-35 / worker/incoming.go:28-34 ->
// router/router.go:21-31: the address (Packet[16:20] outgoing, Raw[0:4] incoming) when it lies in the
// network, else the gateway, looked up in an open-addressing table of 8-byte {ip, peer} entries (linear
// probing, power-of-two capacity, peer == QGCM_NO_PEER = empty).  A hit writes the peer index, the seal /
// open descriptor and, outgoing, own_ip into Raw[0:4]; a miss writes QGCM_NO_PEER in both and leaves the
// slot alone.  Each entry is read with one 8-byte load, each descriptor written with one 16-byte store.
//
// route_account_kernel: metric/aggregator.go:24-68 for a batch.  Sums are exact integers (64-bit atomic
// adds), combined before they reach global memory: packets of a wave that share a link are summed in the
// wave (two rounds: the links of the wave's first lanes -- with skewed traffic the hot link is one of
// them almost always), the rest and the waves' sums go through a 256-entry table in LDS keyed by peer
// (entry peer & 255; a second peer on a taken entry goes to global memory directly), and a workgroup
// walks several 256-packet tiles before it flushes the table, so a hot link costs two global atomics per
// workgroup, not per packet.  The byte counts come from the descriptors (qgcm_route_account) or from an array
// (qgcm_route_account_bytes): one kernel, a template parameter.
#include "gcm_internal.h"
#include "route_core.h"  // route_lookup: shared with frames_kernels.hip

namespace qgcm {
namespace {

constexpr uint32_t kRouteThreads = 256;
constexpr uint32_t kAcctSlots = 256;    // LDS link entries per workgroup
constexpr uint32_t kAcctRounds = 2;     // in-wave combining rounds
constexpr uint32_t kAcctWgsPerCu = 8;

template <bool kOutgoing>
__global__ void __launch_bounds__(kRouteThreads) route_resolve_kernel(RouteArgs a) {
    const uint32_t i = blockIdx.x * kRouteThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t len = a.lens[i];
    const uint64_t off = (uint64_t)i * a.stride;
    uint8_t *slot = a.arena + off;
    uint32_t peer = QGCM_NO_PEER, dlen;
    bool readable;
    if (kOutgoing) {
        // Packet[16:20] must exist, and the sealed datagram must fit the slot
        readable = len >= 20 && 4ull + len + QGCM_OVERHEAD <= a.stride;
        dlen = len;
    } else {
        readable = len >= 4 && len <= a.stride;
        dlen = len >= 4 ? len - 4 : 0;
    }
    if (readable) {
        const uint32_t addr = *reinterpret_cast<const uint32_t *>(slot + (kOutgoing ? 20 : 0));
        const uint32_t key = ((addr ^ a.net) & a.mask) == 0 ? addr : a.gateway;  // router.go:25-30
        peer = route_lookup(a.table, a.cap_mask, key);
        if (kOutgoing && peer != QGCM_NO_PEER) *reinterpret_cast<uint32_t *>(slot) = a.own_ip;  // outgoing.go:30
    }
    a.peer[i] = peer;
    *reinterpret_cast<uint4 *>(a.descs + i) = make_uint4((uint32_t)off, (uint32_t)(off >> 32), dlen, peer);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct AcctLds {
    uint32_t tag[kAcctSlots];
    unsigned long long cnt[kAcctSlots][4];
    unsigned long long tot[4];
};

// {Packets, Bytes, DroppedPackets, DroppedBytes} of one link into the workgroup's table, or past it
__device__ __forceinline__ void acct_add(AcctLds &l, unsigned long long *links, uint32_t peer, unsigned long long pk,
                                         unsigned long long by, unsigned long long dp, unsigned long long db) {
    const uint32_t e = peer & (kAcctSlots - 1);
    const uint32_t old = atomicCAS(&l.tag[e], QGCM_NO_PEER, peer);
    unsigned long long *dst = (old == QGCM_NO_PEER || old == peer) ? l.cnt[e] : links + 4ull * peer;
    if (pk) atomicAdd(dst + 0, pk);
    if (by) atomicAdd(dst + 1, by);
    if (dp) atomicAdd(dst + 2, dp);
    if (db) atomicAdd(dst + 3, db);
}

// kBytes: the byte count of packet i is a.bytes[i] as it stands (qgcm_route_account_bytes: the plugin chain
// knows what each packet ended up as) instead of the descriptor's length +- tag and nonce
template <bool kBytes>
__global__ void __launch_bounds__(kRouteThreads) route_account_kernel(RouteAccountArgs a, uint32_t ntiles) {
    __shared__ AcctLds l;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    l.tag[tid] = QGCM_NO_PEER;
#pragma unroll
    for (int k = 0; k < 4; ++k) l.cnt[tid][k] = 0;
    if (tid < 4) l.tot[tid] = 0;
    __syncthreads();
    unsigned long long *links = a.counters + 4;  // [0, 4): the totals; link p at 4 + 4 p
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * kRouteThreads + tid;  // ntiles * 256 < 2^31 + 256
        const bool in = i < a.n;
        uint32_t p = in ? a.peer[i] : QGCM_NO_PEER;
        if (p >= a.max_keys) p = QGCM_NO_PEER;  // never index past the link counters
        const bool resolved = in && p != QGCM_NO_PEER;
        bool ok = false;
        unsigned long long by = 0, db = 0;
        if (resolved && kBytes) {
            ok = a.status ? a.status[i] == 1 : true;
            (ok ? by : db) = a.bytes[i];
        } else if (resolved) {
            const uint32_t len = reinterpret_cast<const uint4 *>(a.descs + i)->z;
            ok = a.status ? a.status[i] == 1 : true;
            if (a.dir == QGCM_RX && len < QGCM_OVERHEAD) ok = false;  // shorter than tag and nonce: open rejects it
            if (ok) by = a.dir == QGCM_TX ? 4ull + len + QGCM_OVERHEAD : 4ull + len - QGCM_OVERHEAD;  // encryption.go:36-37
            else db = 4ull + len;  // Apply returned its input: the length it came with
        }
        // totals: the whole wave in one go
        const unsigned long long t_pk = __popcll(__ballot(resolved && ok));
        const unsigned long long t_dp = __popcll(__ballot(in && !(resolved && ok)));  // unresolved: bytes 0
        const unsigned long long t_by = wave_sum(by), t_db = wave_sum(db);
        if (lane == 0) {
            if (t_pk) atomicAdd(&l.tot[0], t_pk);
            if (t_by) atomicAdd(&l.tot[1], t_by);
            if (t_dp) atomicAdd(&l.tot[2], t_dp);
            if (t_db) atomicAdd(&l.tot[3], t_db);
        }
        // links: what shares a link with the wave's first lanes is summed in the wave
        bool act = resolved;
        unsigned long long rem = __ballot(act);
        for (uint32_t r = 0; r < kAcctRounds && rem; ++r) {
            const int leader = __ffsll((long long)rem) - 1;
            const uint32_t lp = __shfl(p, leader, 64);
            const bool m = act && p == lp;
            const unsigned long long mm = __ballot(m);
            if (__popcll(mm) > 1) {  // wave-uniform
                const unsigned long long s_by = wave_sum(m ? by : 0ull), s_db = wave_sum(m ? db : 0ull);
                const unsigned long long s_pk = __popcll(__ballot(m && ok)), s_dp = __popcll(__ballot(m && !ok));
                if ((int)lane == leader) acct_add(l, links, lp, s_pk, s_by, s_dp, s_db);
                if (m) act = false;
            }
            rem &= ~mm;
        }
        if (act) acct_add(l, links, p, ok ? 1 : 0, by, ok ? 0 : 1, db);
    }
    __syncthreads();
    const uint32_t tag = l.tag[tid];
    if (tag != QGCM_NO_PEER) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (l.cnt[tid][k]) atomicAdd(links + 4ull * tag + k, l.cnt[tid][k]);
    }
    if (tid < 4 && l.tot[tid]) atomicAdd(a.counters + tid, l.tot[tid]);
}

}  // namespace

hipError_t launch_route_resolve(bool outgoing, const RouteArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)a.n + kRouteThreads - 1) / kRouteThreads);
    if (outgoing)
        hipLaunchKernelGGL(route_resolve_kernel<true>, dim3(grid), dim3(kRouteThreads), 0, s, a);
    else
        hipLaunchKernelGGL(route_resolve_kernel<false>, dim3(grid), dim3(kRouteThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_account(const RouteAccountArgs &a, int num_cus, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t ntiles = (uint32_t)(((uint64_t)a.n + kRouteThreads - 1) / kRouteThreads);
    const uint32_t cap = (uint32_t)(num_cus > 0 ? num_cus : 1) * kAcctWgsPerCu;
    const dim3 grid(ntiles < cap ? ntiles : cap);
    if (a.bytes)
        hipLaunchKernelGGL(route_account_kernel<true>, grid, dim3(kRouteThreads), 0, s, a, ntiles);
    else
        hipLaunchKernelGGL(route_account_kernel<false>, grid, dim3(kRouteThreads), 0, s, a, ntiles);
    return hipGetLastError();
}

}  // namespace qgcm
