// route_core.h -- the probe of the route table (include/qgcm.h "routes resolved on the GPU") for every kernel
// that resolves: route_resolve_kernel (route_kernels.hip) and frames_resolve_kernel (frames_kernels.hip) look a
// key up with this code and with route_hash of gcm_internal.h, which the host builds the table with.
#pragma once
#include "gcm_internal.h"

namespace qgcm {

// The probe sequence from entry h on, e = table[h] already loaded: a caller with other loads to issue reads the
// first entry early and finishes here once they are under way.  At most `capacity` probes: a table without an
// empty entry (never built by qgcm_routes_set) ends too.
__device__ __forceinline__ uint32_t route_lookup_from(const uint2 *table, uint32_t cap_mask, uint32_t ip, uint32_t h, uint2 e) {
    for (uint32_t probes = 0;; ++probes) {
        if (e.y == QGCM_NO_PEER) return QGCM_NO_PEER;
        if (e.x == ip) return e.y;
        if (probes == cap_mask) return QGCM_NO_PEER;
        h = (h + 1) & cap_mask;
        e = table[h];  // {ip, peer} in one 8-byte load
    }
}

__device__ __forceinline__ uint32_t route_lookup(const uint2 *table, uint32_t cap_mask, uint32_t ip) {
    const uint32_t h = route_hash(ip) & cap_mask;
    return route_lookup_from(table, cap_mask, ip, h, table[h]);
}

}  // namespace qgcm
