// One hop of TG_SAMPLER_RECENT over a flat frontier: the k most recent admitted edges of every frontier vertex
// (include/tchgeo.h at the define; PyG's temporal_strategy="last").  Deterministic: no draw is made.
//   select   wavefront per frontier vertex: the column's timestamps are read 64 at a time (two blocks of RC_UNROLL chunks in
//            flight: the next block is requested before this one is looked at), the
//            best 64 entries so far live one per lane in rank order (key = the timestamp turned so that smaller is better,
//            position inside the column as the tie break).  A chunk none of whose admitted edges beats the k-th entry costs
//            one ballot; otherwise its 64 candidates are sorted by a bitonic network of lane exchanges, laid against the
//            kept list in reverse -- the lane-wise better half of the two is the best 64 of the union, as a bitonic
//            sequence -- and six more exchanges put it back in order.  The winners' edge pointers are parked in
//            `neighbors` at [vertex * k + rank]: the hop needs no workspace.
//   scan     offsets = exclusive prefix of the counts (one workgroup, tg_scan.h)
//   emit     lane per parked slot: edge pointer, parent and new filter state go to their compact places
//   gather   lane per sample: neighbors = indices[edge_ptr], once, for the winners only (a launch of its own: it
//            overwrites the parked slots)
// A hub column is scanned by ONE wavefront (splitting long columns is not done here).  No LDS beyond the scan's 128 bytes.
#include <algorithm>

#include "tg_device.h"
#include "tg_filter.h"
#include "tg_host.h"
#include "ns_topk.h"
#include "tg_scan.h"

namespace tg {

constexpr int RC_UNROLL = 8;                     // 64-edge chunks of a block; two blocks' timestamps are in flight together

struct RecentParams {
    const int64_t *ptrs, *indices, *timestamps;
    const uint32_t *ptrs32, *indices32;
    const int64_t *vertices, *states;
    int64_t m;
    int32_t k, filter_mode, forward;
    int64_t win_lo, win_hi;
    int64_t *cnt, *offsets, *neighbors, *edge_ptrs, *parents, *states_out;
};

// RcEntry: key = forward ? t : ~t (= -t - 1: order reversed, no overflow), pos = position inside the column (ns_topk.h)

__device__ __forceinline__ bool rc_pass(const RecentParams &p, int64_t state, int64_t t) { // neighbor_sampling.rs:55-67
    return tg_filter_pass(p.filter_mode, p.forward, p.win_lo, p.win_hi, state, t);
}

__global__ void __launch_bounds__(256) recent_select_kernel(const RecentParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int k = p.k;
    for (int64_t v = wave_id; v < p.m; v += n_waves) {
        const int64_t w = p.vertices[v];
        int64_t e0 = 0, deg = 0;
        if (w >= 0) {
            if (p.ptrs32) {
                e0 = (int64_t)p.ptrs32[w];
                deg = (int64_t)p.ptrs32[w + 1] - e0;
            } else {
                e0 = p.ptrs[w];
                deg = p.ptrs[w + 1] - e0;
            }
        }
        const int64_t st = p.states ? p.states[v] : 0;
        RcEntry kept{RC_NO_KEY, RC_NO_POS};
        // the next block's timestamps are requested before this block is looked at: one wavefront is all a hub column gets,
        // and what it streams per second is the bytes it keeps in flight over the memory latency
        int64_t tsv[RC_UNROLL], nxt[RC_UNROLL];
        auto request = [&](int64_t (&dst)[RC_UNROLL], int64_t c0) {
#pragma unroll
            for (int u = 0; u < RC_UNROLL; ++u) {
                // unconditional (a branch around a load makes the compiler wait for every load in flight): lanes past the
                // column's end re-read its last element and are ignored below
                const int64_t q = min(c0 + u * 64 + lane, deg - 1);
                dst[u] = __builtin_nontemporal_load(&p.timestamps[e0 + q]);
            }
        };
        if (deg > 0) request(tsv, 0); // wave-uniform
        for (int64_t c0 = 0; c0 < deg; c0 += (int64_t)64 * RC_UNROLL) {
            request(nxt, c0 + (int64_t)64 * RC_UNROLL);
#pragma unroll
            for (int u = 0; u < RC_UNROLL; ++u) {
                const int64_t q = c0 + u * 64 + lane;
                RcEntry c{p.forward ? tsv[u] : ~tsv[u], (uint32_t)q};
                const RcEntry kth = rc_shfl(kept, k - 1); // empty while fewer than k are kept
                const bool cand = q < deg && rc_pass(p, st, tsv[u]) && rc_before(c, kth);
                if (__ballot(cand) == 0) continue; // wave-uniform
                if (!cand) c = RcEntry{RC_NO_KEY, RC_NO_POS};
                // bitonic sort of the 64 candidates, best first; best 64 of kept (ascending) and candidates (reversed): a
                // bitonic sequence; six steps order it (ns_topk.h)
                c = rc_sort64(c, lane);
                kept = rc_merge_reversed(kept, rc_shfl(c, 63 - lane), lane);
            }
#pragma unroll
            for (int u = 0; u < RC_UNROLL; ++u) tsv[u] = nxt[u];
        }
        const int n_kept = __popcll(__ballot(kept.pos != RC_NO_POS));
        const int cnt = n_kept < k ? n_kept : k;
        if (lane == 0) p.cnt[v] = cnt;
        if (lane < cnt) p.neighbors[v * k + lane] = e0 + (int64_t)kept.pos; // parked until the offsets are known
    }
}

__global__ void __launch_bounds__(SCAN1_THREADS) recent_scan_kernel(const RecentParams p) {
    block_scan_exclusive_plus1(p.m, [&](int64_t i) { return p.cnt[i]; }, p.offsets);
}

__global__ void __launch_bounds__(256) recent_emit_kernel(const RecentParams p) {
    const int64_t n = p.m * p.k;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = j / p.k, r = j - v * p.k;
        if (r >= p.cnt[v]) continue;
        const int64_t ep = p.neighbors[j], o = p.offsets[v] + r;
        p.edge_ptrs[o] = ep;
        p.parents[o] = v;
        if (p.states_out) // the filter's mutate (neighbor_sampling.rs:69-76)
            p.states_out[o] = (p.filter_mode == TG_FILTER_DYNAMIC) ? p.timestamps[ep] : (p.states ? p.states[v] : 0);
    }
}

__global__ void __launch_bounds__(256) recent_gather_kernel(const RecentParams p) {
    const int64_t total = p.offsets[p.m];
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ep = p.edge_ptrs[o];
        p.neighbors[o] = p.indices32 ? (int64_t)__builtin_nontemporal_load(&p.indices32[ep])
                                     : __builtin_nontemporal_load(&p.indices[ep]);
    }
}

} // namespace tg

extern "C" int tg_ns_hop_recent(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *flt, const tg_hop_out *out,
                                int64_t *states_out, void *stream_) {
    using namespace tg;
    TG_REQUIRE(csc && csc->ptrs && in && out, "tg_ns_hop_recent: null argument");
    TG_REQUIRE(in->sampler == TG_SAMPLER_RECENT, "tg_ns_hop_recent: in->sampler must be TG_SAMPLER_RECENT");
    TG_REQUIRE(in->m >= 0, "tg_ns_hop_recent: negative frontier size");
    TG_REQUIRE(in->fanout >= 1 && in->fanout <= 64, "tg_ns_hop_recent: fan-out %d outside 1..64", in->fanout);
    TG_REQUIRE(csc->timestamps || csc->n_edges == 0, "tg_ns_hop_recent: the graph has no edge timestamps");
    TG_REQUIRE(csc->indices || csc->n_edges == 0, "tg_ns_hop_recent: null graph");
    TG_REQUIRE(recent_columns_fit(csc),
               "tg_ns_hop_recent: columns must be shorter than 2^32 - 1 edges (a graph this large has to state max_degree)");
    const int mode = flt ? flt->filter_mode : TG_FILTER_NONE;
    TG_REQUIRE(mode >= TG_FILTER_NONE && mode <= TG_FILTER_DYNAMIC, "tg_ns_hop_recent: bad filter %d", mode);
    TG_REQUIRE(in->m <= INT64_MAX / 64, "tg_ns_hop_recent: frontier too long");
    TG_REQUIRE(out->cnt && out->offsets, "tg_ns_hop_recent: null outputs");
    hipStream_t stream = (hipStream_t)stream_;
    if (in->m == 0) {
        TG_HIP(hipMemsetAsync(out->offsets, 0, sizeof(int64_t), stream));
        return TG_OK;
    }
    TG_REQUIRE(in->vertices && out->neighbors && out->edge_ptrs && out->parents, "tg_ns_hop_recent: null buffers");
    TG_REQUIRE(mode == TG_FILTER_NONE || (flt->states && states_out),
               "tg_ns_hop_recent: a filter needs its states and states_out");
    RecentParams p;
    p.ptrs = csc->ptrs;
    p.indices = csc->indices;
    p.timestamps = csc->timestamps;
    p.ptrs32 = csc->ptrs32;
    p.indices32 = csc->indices32;
    p.vertices = in->vertices;
    p.states = mode == TG_FILTER_NONE ? nullptr : flt->states;
    p.m = in->m;
    p.k = in->fanout;
    p.filter_mode = mode;
    p.forward = (flt && flt->forward) ? 1 : 0;
    p.win_lo = flt ? flt->win_lo : 0;
    p.win_hi = flt ? flt->win_hi : 0;
    p.cnt = out->cnt;
    p.offsets = out->offsets;
    p.neighbors = out->neighbors;
    p.edge_ptrs = out->edge_ptrs;
    p.parents = out->parents;
    p.states_out = mode == TG_FILTER_NONE ? nullptr : states_out;
    auto blocks = [](int64_t items, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min((items + 255) / 256, cap)); };
    // a workgroup is four wavefronts = four vertices; the dispatcher balances the columns' lengths
    hipLaunchKernelGGL(recent_select_kernel, dim3(blocks(p.m * 64, (int64_t)1 << 22)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(recent_scan_kernel, dim3(1), dim3(SCAN1_THREADS), 0, stream, p);
    hipLaunchKernelGGL(recent_emit_kernel, dim3(blocks(p.m * p.k, 256 * 32)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(recent_gather_kernel, dim3(blocks(p.m * p.k, 256 * 32)), dim3(256), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
