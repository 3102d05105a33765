// frames_core.h -- the frame table of include/qgcm.h ("outgoing frames packed on routed batches") as plain
// C++: when a frame is valid, the table checks of the host entry points and the host unpack.  No HIP, no
// allocation: qgcm_frames_unpack_cpu runs it, frames_kernels.hip shares the validity rule with it, route.cpp
// checks its tables with it, and tests/cpp_frames builds it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgcm.h"

#if defined(__HIPCC__)
#define QGCM_FRAMES_HD __host__ __device__
#else
#define QGCM_FRAMES_HD
#endif

namespace qgcm {

constexpr uint64_t kFramePacketStart = 4;  // common.PacketStart: the frame lands at Raw[4:]
constexpr uint64_t kFrameRoom = 65536;     // qgcm_tun_read_packed reads only with this much room: no frame is cut

// A frame is valid when it starts on a 16-byte boundary and ends inside the packed area (64-bit: off and len
// are whatever the table says).
QGCM_FRAMES_HD inline bool frame_valid(uint32_t off, uint32_t len, uint64_t packed_len) {
    return (off & 15u) == 0 && (uint64_t)off + len <= packed_len;
}

// The bytes of a frame of `len` that a slot of `stride` holds (stride >= 8).
QGCM_FRAMES_HD inline uint32_t frame_slot_bytes(uint32_t len, uint64_t stride) {
    return len < stride - kFramePacketStart ? len : (uint32_t)(stride - kFramePacketStart);
}

// What qgcm_frames_unpack_cpu asks of a table: every frame valid.
inline bool frames_table_ok(const qgcm_frame *frames, uint32_t n, uint64_t packed_len) {
    for (uint32_t i = 0; i < n; ++i)
        if (!frame_valid(frames[i].off, frames[i].len, packed_len)) return false;
    return true;
}

// What qgcm_route_chain_seal_frames_host asks: every frame valid, and the offsets ascending without overlap, so
// a run of frames spans [off of its first, end of its last).
inline bool frames_table_ascends(const qgcm_frame *frames, uint32_t n, uint64_t packed_len) {
    uint64_t end = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!frame_valid(frames[i].off, frames[i].len, packed_len) || frames[i].off < end) return false;
        end = (uint64_t)frames[i].off + frames[i].len;
    }
    return true;
}

// The unpack by the host for a table that passed frames_table_ok: lens[i] = len and Raw[4 : 4 + min(len,
// stride - 4)) of slot i for every frame; nothing else is written.
inline void frames_unpack_cpu(const uint8_t *packed, const qgcm_frame *frames, uint32_t n, uint8_t *arena, uint64_t stride,
                              uint32_t *lens) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t bytes = frame_slot_bytes(frames[i].len, stride);
        lens[i] = frames[i].len;
        if (bytes) memcpy(arena + (uint64_t)i * stride + kFramePacketStart, packed + frames[i].off, bytes);
    }
}

// qgcm_frames_unpack_cpu whole: the arguments, the table, then the unpack.
inline int frames_unpack_checked(const uint8_t *packed, uint64_t packed_len, const qgcm_frame *frames, uint32_t n,
                                 uint8_t *arena, uint64_t stride, uint32_t *lens) {
    if (n > QGCM_MAX_BATCH || (stride & 3) || stride < 8) return QGCM_E_ARG;
    if (n && (!packed || !frames || !arena || !lens)) return QGCM_E_ARG;
    if (!frames_table_ok(frames, n, packed_len)) return QGCM_E_ARG;
    frames_unpack_cpu(packed, frames, n, arena, stride, lens);
    return QGCM_OK;
}

}  // namespace qgcm
