// The running top-64 of a wavefront, one entry per lane in rank order: the entry type, the compare-exchange step and the
// merge shared by tg_ns_hop_recent (key = a timestamp) and tg_ns_hop_labor (key = a Philox draw of the neighbour's id).
#pragma once
#include "tg_device.h"

namespace tg {

constexpr uint32_t RC_NO_POS = 0xFFFFFFFFu;      // an empty entry: ranks behind every edge (columns have < 2^32 - 1 edges)
constexpr int64_t RC_NO_KEY = INT64_MAX;

struct RcEntry {
    int64_t key;  // the smaller key ranks first
    uint32_t pos; // position inside the column: the smaller edge pointer ranks first among equal keys
};

__device__ __forceinline__ bool rc_before(const RcEntry &a, const RcEntry &b) {
    return a.key < b.key || (a.key == b.key && a.pos < b.pos);
}
__device__ __forceinline__ RcEntry rc_shfl_xor(const RcEntry &a, int j) {
    RcEntry r;
    r.key = __shfl_xor(a.key, j, 64);
    r.pos = __shfl_xor(a.pos, j, 64);
    return r;
}
__device__ __forceinline__ RcEntry rc_shfl(const RcEntry &a, int src) {
    RcEntry r;
    r.key = __shfl(a.key, src, 64);
    r.pos = __shfl(a.pos, src, 64);
    return r;
}
// one compare-exchange step with the lane `j` away: this lane keeps the better entry of the pair iff keep_better
__device__ __forceinline__ RcEntry rc_exchange(const RcEntry &v, int j, bool keep_better) {
    const RcEntry o = rc_shfl_xor(v, j);
    return (rc_before(o, v) == keep_better) ? o : v;
}

// bitonic sort of the 64 candidates (one per lane), best first
__device__ __forceinline__ RcEntry rc_sort64(RcEntry c, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
        const bool up = (lane & size) == 0;
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) c = rc_exchange(c, j, ((lane & j) == 0) == up);
    }
    return c;
}

// `kept` (ascending) against another list given in REVERSE order (lane l holds its entry 63 - l): the lane-wise better
// half of the two is the best 64 of the union, as a bitonic sequence; six steps order it
__device__ __forceinline__ RcEntry rc_merge_reversed(RcEntry kept, const RcEntry &r, int lane) {
    if (rc_before(r, kept)) kept = r;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) kept = rc_exchange(kept, j, (lane & j) == 0);
    return kept;
}

} // namespace tg
