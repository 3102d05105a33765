// chain_kernels.hip -- the plugin chain of a routed packet batch on gfx950 (include/qgcm.h "plugin chain on
// routed batches"): the elementwise kernels that string resolve, the snappy codec, the
// descriptor seal / open and the accounting together under each peer's own plugin flags.
//
// main.go:41-51 runs compression then encryption outgoing and the reverse incoming; plugin/compression.go:31-33
// and plugin/encryption.go:17-19 pass a packet through when the peer does not list the plugin.  Per packet
// F = plugins & flags[peer].  One lane per packet everywhere; a packet's bytes are touched only by the codec
// and the seal / open, these kernels move a few bytes of lengths, statuses and descriptors each.
//
// The peer's flags are read ONCE per call, by the plan kernel, and travel with the packet in the work area
// (ChainArgs::flags): a qgcm_peer_plugins_set racing the call cannot compress a packet under one value and
// account it under another.
//
// outgoing:  plan -> [compress, gated] -> [descs] -> [seal] -> finish
// incoming:  plan -> [open] -> mid -> [uncompress, gated] -> [finish]
// A stage in brackets runs only when the node's own mask has the plugin; without compression the outgoing
// plan writes the seal descriptors itself, without encryption the incoming mid takes the flags itself, and
// without compression the incoming mid is the last kernel.
#include "gcm_internal.h"

namespace qgcm {
namespace {

constexpr uint32_t kChainThreads = 256;
constexpr uint32_t kComp = QGCM_PLUGIN_COMPRESSION, kEnc = QGCM_PLUGIN_ENCRYPTION;

// kChainResolved | F, or 0 for a packet no route resolved (a peer at or above max_keys counts as that)
__device__ __forceinline__ uint32_t snapshot(const ChainArgs &a, uint32_t peer) {
    if (peer >= a.max_keys) return 0;
    const uint32_t f = a.peer_plugins ? a.peer_plugins[peer] : kEnc;
    return kChainResolved | (a.plugins & f & (kComp | kEnc));
}

__device__ __forceinline__ void put_desc(const ChainArgs &a, uint32_t i, uint32_t len, uint32_t key) {
    const uint64_t off = (uint64_t)i * a.stride;
    *reinterpret_cast<uint4 *>(a.descs + i) = make_uint4((uint32_t)off, (uint32_t)(off >> 32), len, key);
}

__device__ __forceinline__ void verdict(const ChainArgs &a, uint32_t i, uint32_t len, uint32_t st, uint32_t bytes) {
    a.lens[i] = len;
    a.status[i] = (uint8_t)st;
    a.bytes[i] = bytes;
}

// flags and the compression gate; kDescs (a call without compression): the seal descriptors too
template <bool kDescs>
__global__ void __launch_bounds__(kChainThreads) chain_out_plan_kernel(ChainArgs a) {
    const uint32_t i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t peer = a.peer[i];
    const uint32_t fl = snapshot(a, peer);
    a.flags[i] = (uint8_t)fl;
    // the codec's room: a packet sealed afterwards leaves 28 B for tag and nonce (gate 2: limit_b)
    a.gate[i] = (fl & kComp) ? ((fl & kEnc) ? 2 : 1) : 0;
    a.cstat[i] = 0;
    if (kDescs) put_desc(a, i, a.lens[i], (fl & kEnc) ? peer : QGCM_NO_PEER);
}

// after the codec: the seal takes what F encrypts and the codec did not refuse
__global__ void __launch_bounds__(kChainThreads) chain_out_descs_kernel(ChainArgs a) {
    const uint32_t i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t fl = a.flags[i];
    const bool refused = a.gate[i] && a.cstat[i] != 1;
    put_desc(a, i, a.lens[i], (fl & kEnc) && !refused ? a.peer[i] : QGCM_NO_PEER);
}

__global__ void __launch_bounds__(kChainThreads) chain_out_finish_kernel(ChainArgs a) {
    const uint32_t i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t fl = a.flags[i], len = a.lens[i];  // the length as the codec left it
    if (!(fl & kChainResolved))
        verdict(a, i, 0, 0, 0);
    else if (a.gate[i] && a.cstat[i] != 1)
        verdict(a, i, 0, 0, 4 + len);  // the codec refused it: Length as the packet came
    else if (!(fl & kEnc))
        verdict(a, i, 4 + len, 1, 4 + len);  // passed through encryption
    else if (a.sstat[i] == 1)
        verdict(a, i, 4 + len + QGCM_OVERHEAD, 1, 4 + len + QGCM_OVERHEAD);
    else
        verdict(a, i, 0, 0, 4 + len);  // key slot unset: Apply returned its input
}

// flags and the open descriptors: only what F decrypts is opened (resolve wrote {i * stride, m - 4, peer})
__global__ void __launch_bounds__(kChainThreads) chain_in_plan_kernel(ChainArgs a) {
    const uint32_t i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t peer = a.peer[i], m = a.lens[i];
    const uint32_t fl = snapshot(a, peer);
    a.flags[i] = (uint8_t)fl;
    put_desc(a, i, m >= 4 ? m - 4 : 0, (fl & kEnc) ? peer : QGCM_NO_PEER);
}

// after the open: its verdicts, and the codec's gate "opened or passed through, and F has compression" with
// the packet length the codec takes; what F does not compress is delivered here.  kPlan (a call without
// encryption): takes the flags itself, nothing was opened.
template <bool kPlan>
__global__ void __launch_bounds__(kChainThreads) chain_in_mid_kernel(ChainArgs a) {
    const uint32_t i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t m = a.lens[i];
    uint32_t fl;
    if (kPlan) {
        fl = snapshot(a, a.peer[i]);
        a.flags[i] = (uint8_t)fl;
    } else {
        fl = a.flags[i];
    }
    uint32_t gate = 0;
    if (!(fl & kChainResolved) || m < 4) {  // (resolve leaves no datagram below 4 bytes resolved)
        verdict(a, i, 0, 0, 0);
    } else if ((fl & kEnc) && a.sstat[i] != 1) {
        verdict(a, i, 0, 0, m);  // Length as the datagram came: 4 + (m - 4)
    } else {
        const uint32_t len = (fl & kEnc) ? m - 4 - QGCM_OVERHEAD : m - 4;  // an opened packet has m - 4 >= 28
        if (fl & kComp) {
            gate = 1;
            a.lens[i] = len;  // what the codec reads; chain_in_finish_kernel has the last word
        } else {
            verdict(a, i, len, 1, 4 + len);
        }
    }
    a.gate[i] = (uint8_t)gate;
    a.cstat[i] = 0;
}

__global__ void __launch_bounds__(kChainThreads) chain_in_finish_kernel(ChainArgs a) {
    const uint32_t i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= a.n || !a.gate[i]) return;
    const uint32_t len = a.lens[i];  // decoded: the packet's length; failed: the length it entered the codec with
    if (a.cstat[i] == 1)
        verdict(a, i, len, 1, 4 + len);
    else
        verdict(a, i, 0, 0, 4 + len);
}

}  // namespace

hipError_t launch_chain(ChainStage stage, bool fused, const ChainArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)a.n + kChainThreads - 1) / kChainThreads)), block(kChainThreads);
    switch (stage) {
    case kChainOutPlan:
        if (fused)
            hipLaunchKernelGGL(chain_out_plan_kernel<true>, grid, block, 0, s, a);
        else
            hipLaunchKernelGGL(chain_out_plan_kernel<false>, grid, block, 0, s, a);
        break;
    case kChainOutDescs:
        hipLaunchKernelGGL(chain_out_descs_kernel, grid, block, 0, s, a);
        break;
    case kChainOutFinish:
        hipLaunchKernelGGL(chain_out_finish_kernel, grid, block, 0, s, a);
        break;
    case kChainInPlan:
        hipLaunchKernelGGL(chain_in_plan_kernel, grid, block, 0, s, a);
        break;
    case kChainInMid:
        if (fused)
            hipLaunchKernelGGL(chain_in_mid_kernel<true>, grid, block, 0, s, a);
        else
            hipLaunchKernelGGL(chain_in_mid_kernel<false>, grid, block, 0, s, a);
        break;
    case kChainInFinish:
        hipLaunchKernelGGL(chain_in_finish_kernel, grid, block, 0, s, a);
        break;
    }
    return hipGetLastError();
}

}  // namespace qgcm
