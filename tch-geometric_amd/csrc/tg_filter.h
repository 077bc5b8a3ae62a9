// The temporal admission predicate (reference: src/algo/neighbor_sampling.rs:55-67), spelled once for every kernel that
// tests an edge's timestamp `t` against the state of the vertex (or subgraph) that looks at it: the filtered hops
// (ns_hop_scan.hip, ns_hop_recent.hip) and the per-subgraph induced edges (ns_induced.hip).
#pragma once
#include "tg_host.h"

namespace tg {

// x = t (static), t - state (relative, forward) or state - t (relative, backward), in wrapping int64 arithmetic like the
// reference's release build; admitted iff lo <= x <= hi
__device__ __forceinline__ bool tg_filter_pass(int32_t filter_mode, int32_t forward, int64_t lo, int64_t hi, int64_t state,
                                               int64_t t) {
    if (filter_mode == TG_FILTER_NONE) return true;
    const uint64_t d = (uint64_t)t - (uint64_t)state;
    const int64_t x = (filter_mode == TG_FILTER_STATIC) ? t : (forward ? (int64_t)d : (int64_t)(0 - d));
    return lo <= x && x <= hi;
}

} // namespace tg
