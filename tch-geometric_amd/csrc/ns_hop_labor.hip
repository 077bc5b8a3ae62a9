// One hop of TG_SAMPLER_LABOR / TG_SAMPLER_LABOR_SHARED over a flat frontier: layer-neighbor sampling (LABOR-0; semantics in
// include/tchgeo.h at the defines).  Every graph vertex t has one variate per (call id, layer), the draw
// (call key of (seed, call id, TG_TAG_LABOR), id = t, d0 = layer, d1 = 0); a frontier vertex keeps the k admitted edges
// whose neighbours have the smallest variates, ties (parallel edges) to the smaller edge pointer.  tg_ns_hop_recent's shape
// (ns_hop_recent.hip, the top-64 of ns_topk.h) with the draw in the timestamp's place:
//   select   wavefront per frontier vertex: the column's neighbour ids (and, under a filter only, its timestamps) are read
//            64 at a time, the next block requested before this one is looked at; every lane runs one Philox4x32-10 block
//            for its edge; a chunk none of whose admitted edges beats the k-th kept entry costs one ballot, the others a
//            bitonic sort and merge by lane exchanges.  The call key is computed once per vertex.  A column of more than
//            `long_column` edges is not scanned here: its frontier index is appended to a list in the workspace (one atomic);
//   long     a fixed grid of 16-wavefront workgroups strides over that list (the count is read on the device): each
//            wavefront scans a sixteenth of the column into its own top-64, the sixteen lists meet through LDS in four
//            rounds of the same merge step (12 KiB).  Positions are the column's, so ties fall as in the short kernel and
//            the result is the same word for word;
//   scan, emit, gather   as tg_ns_hop_recent's (copied: those kernels take RecentParams and stay as they are).
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "ns_topk.h"
#include "tg_device.h"
#include "tg_filter.h"
#include "tg_host.h"
#include "tg_scan.h"

namespace tg {

// 64-edge chunks of a block; two blocks are in flight together.  Deeper blocks (8 / 16 chunks) were measured and bought
// nothing: a lane's Philox block, not the memory latency, is what a wavefront waits for
constexpr int LB_UNROLL = 4;
constexpr int LB_LONG_WAVES = 16;     // wavefronts of a workgroup of the long-column kernel
constexpr int LB_LONG_BLOCKS = 512;   // its fixed grid
constexpr int64_t LB_WS_HEAD = 32;    // words in front of the list: [0] the number of long vertices

struct LaborParams {
    const int64_t *ptrs, *indices, *timestamps;
    const uint32_t *ptrs32, *indices32;
    const int64_t *vertices, *states, *call_ids;
    int64_t m, long_column;
    int32_t k, filter_mode, forward;
    uint32_t tag, layer;
    int64_t win_lo, win_hi;
    uint64_t seed, call_id;
    int64_t *cnt, *offsets, *neighbors, *edge_ptrs, *parents, *states_out;
    unsigned long long *n_long; // workspace: the counter ...
    int64_t *long_list;         // ... and the frontier indices of the long columns, in any order
};

__device__ __forceinline__ void labor_column(const LaborParams &p, int64_t v, int64_t &e0, int64_t &deg) {
    const int64_t w = p.vertices[v];
    e0 = 0;
    deg = 0;
    if (w >= 0) {
        if (p.ptrs32) {
            e0 = (int64_t)p.ptrs32[w];
            deg = (int64_t)p.ptrs32[w + 1] - e0;
        } else {
            e0 = p.ptrs[w];
            deg = p.ptrs[w + 1] - e0;
        }
    }
}

__device__ __forceinline__ CallKey labor_call_key(const LaborParams &p, int64_t v) {
    return call_key(p.seed, p.call_ids ? (uint64_t)p.call_ids[v] : p.call_id, p.tag);
}

// the best 64 of the column's positions [begin, end) (begin a multiple of 64), ascending one per lane
template <bool IDX32, bool FILTERED>
__device__ __forceinline__ RcEntry labor_scan(const LaborParams &p, int lane, int64_t e0, int64_t begin, int64_t end, int64_t st,
                                              CallKey ck) {
    using IdT = typename std::conditional<IDX32, uint32_t, int64_t>::type;
    const int k = p.k;
    RcEntry kept{RC_NO_KEY, RC_NO_POS};
    if (begin >= end) return kept; // wave-uniform
    IdT idv[LB_UNROLL], idn[LB_UNROLL];
    int64_t tsv[FILTERED ? LB_UNROLL : 1], tsn[FILTERED ? LB_UNROLL : 1];
    auto request = [&](IdT(&ids)[LB_UNROLL], int64_t(&ts)[FILTERED ? LB_UNROLL : 1], int64_t c0) {
#pragma unroll
        for (int u = 0; u < LB_UNROLL; ++u) {
            // unconditional: lanes past the slice's end re-read its last element and are ignored below
            const int64_t q = min(c0 + u * 64 + lane, end - 1);
            if constexpr (IDX32)
                ids[u] = __builtin_nontemporal_load(&p.indices32[e0 + q]);
            else
                ids[u] = __builtin_nontemporal_load(&p.indices[e0 + q]);
            if constexpr (FILTERED) ts[u] = __builtin_nontemporal_load(&p.timestamps[e0 + q]);
        }
    };
    request(idv, tsv, begin);
    for (int64_t c0 = begin; c0 < end; c0 += (int64_t)64 * LB_UNROLL) {
        request(idn, tsn, c0 + (int64_t)64 * LB_UNROLL);
#pragma unroll
        for (int u = 0; u < LB_UNROLL; ++u) {
            if (c0 + u * 64 >= end) break; // wave-uniform: no draws for chunks past the slice's end
            const int64_t q = c0 + u * 64 + lane;
            const uint64_t a = draw(ck, (uint64_t)idv[u], p.layer, 0u).a();
            RcEntry c{(int64_t)(a >> 1), (uint32_t)q};
            const RcEntry kth = rc_shfl(kept, k - 1); // empty while fewer than k are kept
            bool cand = q < end && rc_before(c, kth);
            if constexpr (FILTERED) cand = cand && tg_filter_pass(p.filter_mode, p.forward, p.win_lo, p.win_hi, st, tsv[u]);
            if (__ballot(cand) == 0) continue; // wave-uniform
            if (!cand) c = RcEntry{RC_NO_KEY, RC_NO_POS};
            c = rc_sort64(c, lane);
            kept = rc_merge_reversed(kept, rc_shfl(c, 63 - lane), lane);
        }
#pragma unroll
        for (int u = 0; u < LB_UNROLL; ++u) idv[u] = idn[u];
        if constexpr (FILTERED) {
#pragma unroll
            for (int u = 0; u < LB_UNROLL; ++u) tsv[u] = tsn[u];
        }
    }
    return kept;
}

// the winners' edge pointers are parked in `neighbors` at [vertex * k + rank] until the offsets are known
__device__ __forceinline__ void labor_park(const LaborParams &p, int lane, int64_t v, int64_t e0, const RcEntry &kept) {
    const int n_kept = __popcll(__ballot(kept.pos != RC_NO_POS));
    const int cnt = n_kept < p.k ? n_kept : p.k;
    if (lane == 0) p.cnt[v] = cnt;
    if (lane < cnt) p.neighbors[v * p.k + lane] = e0 + (int64_t)kept.pos;
}

template <bool IDX32, bool FILTERED>
__global__ void __launch_bounds__(256) labor_select_kernel(const LaborParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t v = wave_id; v < p.m; v += n_waves) {
        int64_t e0, deg;
        labor_column(p, v, e0, deg);
        if (deg > p.long_column) { // wave-uniform: left to the long-column kernel
            if (lane == 0) p.long_list[atomicAdd(p.n_long, 1ull)] = v; // at most m entries: one per frontier vertex
            continue;
        }
        const int64_t st = FILTERED ? p.states[v] : 0;
        const RcEntry kept = labor_scan<IDX32, FILTERED>(p, lane, e0, 0, deg, st, labor_call_key(p, v));
        labor_park(p, lane, v, e0, kept);
    }
}

template <bool IDX32, bool FILTERED>
__global__ void __launch_bounds__(64 * LB_LONG_WAVES) labor_long_kernel(const LaborParams p) {
    __shared__ int64_t lkey[LB_LONG_WAVES][64];
    __shared__ uint32_t lpos[LB_LONG_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_long = (int64_t)*p.n_long; // written by the select kernel, which has finished
    for (int64_t i = blockIdx.x; i < n_long; i += gridDim.x) { // block-uniform: every wavefront meets every barrier
        const int64_t v = p.long_list[i];
        int64_t e0, deg;
        labor_column(p, v, e0, deg);
        const int64_t per = ((deg + 63) / 64 + LB_LONG_WAVES - 1) / LB_LONG_WAVES * 64; // a wavefront's slice: whole chunks
        const int64_t begin = min(deg, wave * per), end = min(deg, begin + per);
        const int64_t st = FILTERED ? p.states[v] : 0;
        RcEntry kept = labor_scan<IDX32, FILTERED>(p, lane, e0, begin, end, st, labor_call_key(p, v));
        // four rounds: wavefront w + step hands its list to wavefront w.  A row written in a round was last read in the
        // same round of the vertex before, with a barrier in between: one barrier per round is enough
#pragma unroll
        for (int step = 1; step < LB_LONG_WAVES; step <<= 1) {
            const int role = wave & (2 * step - 1);
            if (role == step) {
                lkey[wave][lane] = kept.key;
                lpos[wave][lane] = kept.pos;
            }
            __syncthreads();
            if (role == 0) {
                const RcEntry r{lkey[wave + step][63 - lane], lpos[wave + step][63 - lane]};
                kept = rc_merge_reversed(kept, r, lane);
            }
        }
        if (wave == 0) labor_park(p, lane, v, e0, kept);
    }
}

__global__ void __launch_bounds__(SCAN1_THREADS) labor_scan_kernel(const LaborParams p) {
    block_scan_exclusive_plus1(p.m, [&](int64_t i) { return p.cnt[i]; }, p.offsets);
}

__global__ void __launch_bounds__(256) labor_emit_kernel(const LaborParams p) {
    const int64_t n = p.m * p.k;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = j / p.k, r = j - v * p.k;
        if (r >= p.cnt[v]) continue;
        const int64_t ep = p.neighbors[j], o = p.offsets[v] + r;
        p.edge_ptrs[o] = ep;
        p.parents[o] = v;
        if (p.states_out) // the filter's mutate (neighbor_sampling.rs:69-76)
            p.states_out[o] = (p.filter_mode == TG_FILTER_DYNAMIC) ? p.timestamps[ep] : p.states[v];
    }
}

__global__ void __launch_bounds__(256) labor_gather_kernel(const LaborParams p) {
    const int64_t total = p.offsets[p.m];
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ep = p.edge_ptrs[o];
        p.neighbors[o] = p.indices32 ? (int64_t)__builtin_nontemporal_load(&p.indices32[ep])
                                     : __builtin_nontemporal_load(&p.indices[ep]);
    }
}

static std::atomic<int64_t> g_long_column{TG_LABOR_LONG_COLUMN};

template <bool IDX32, bool FILTERED>
static void labor_launch(const LaborParams &p, unsigned select_blocks, hipStream_t stream) {
    hipLaunchKernelGGL((labor_select_kernel<IDX32, FILTERED>), dim3(select_blocks), dim3(256), 0, stream, p);
    hipLaunchKernelGGL((labor_long_kernel<IDX32, FILTERED>), dim3(LB_LONG_BLOCKS), dim3(64 * LB_LONG_WAVES), 0, stream, p);
}

} // namespace tg

extern "C" int tg_ns_hop_labor_long_column(int64_t edges, int64_t *previous) {
    TG_REQUIRE(edges >= 0, "tg_ns_hop_labor_long_column: negative threshold");
    const int64_t old = tg::g_long_column.exchange(edges == 0 ? TG_LABOR_LONG_COLUMN : edges);
    if (previous) *previous = old;
    return TG_OK;
}

extern "C" int tg_ns_hop_labor_workspace_bytes(int64_t m, int64_t *bytes) {
    TG_REQUIRE(bytes && m >= 0 && m <= INT64_MAX / 64, "tg_ns_hop_labor_workspace_bytes: bad arguments");
    *bytes = (m + tg::LB_WS_HEAD) * 8;
    return TG_OK;
}

extern "C" int tg_ns_hop_labor(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *flt, const tg_rng *rng,
                               int32_t layer, const tg_hop_out *out, int64_t *states_out, void *workspace,
                               int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    TG_REQUIRE(csc && csc->ptrs && in && out && rng, "tg_ns_hop_labor: null argument");
    TG_REQUIRE(in->sampler == TG_SAMPLER_LABOR || in->sampler == TG_SAMPLER_LABOR_SHARED,
               "tg_ns_hop_labor: in->sampler must be TG_SAMPLER_LABOR or TG_SAMPLER_LABOR_SHARED");
    TG_REQUIRE(in->m >= 0, "tg_ns_hop_labor: negative frontier size");
    TG_REQUIRE(in->fanout >= 1 && in->fanout <= 64, "tg_ns_hop_labor: fan-out %d outside 1..64", in->fanout);
    TG_REQUIRE(layer >= 0, "tg_ns_hop_labor: negative layer");
    TG_REQUIRE(csc->indices || csc->n_edges == 0, "tg_ns_hop_labor: null graph");
    TG_REQUIRE(recent_columns_fit(csc),
               "tg_ns_hop_labor: columns must be shorter than 2^32 - 1 edges (a graph this large has to state max_degree)");
    const int mode = flt ? flt->filter_mode : TG_FILTER_NONE;
    TG_REQUIRE(mode >= TG_FILTER_NONE && mode <= TG_FILTER_DYNAMIC, "tg_ns_hop_labor: bad filter %d", mode);
    TG_REQUIRE(mode == TG_FILTER_NONE || csc->timestamps || csc->n_edges == 0,
               "tg_ns_hop_labor: a filter needs the graph's edge timestamps");
    TG_REQUIRE(in->m <= INT64_MAX / 64, "tg_ns_hop_labor: frontier too long");
    TG_REQUIRE(out->cnt && out->offsets, "tg_ns_hop_labor: null outputs");
    hipStream_t stream = (hipStream_t)stream_;
    if (in->m == 0) {
        TG_HIP(hipMemsetAsync(out->offsets, 0, sizeof(int64_t), stream));
        return TG_OK;
    }
    TG_REQUIRE(in->vertices && out->neighbors && out->edge_ptrs && out->parents, "tg_ns_hop_labor: null buffers");
    TG_REQUIRE(mode == TG_FILTER_NONE || (flt->states && states_out),
               "tg_ns_hop_labor: a filter needs its states and states_out");
    int64_t need = 0;
    tg_ns_hop_labor_workspace_bytes(in->m, &need);
    TG_REQUIRE(workspace && workspace_bytes >= need, "tg_ns_hop_labor: workspace missing or too small (%lld < %lld bytes)",
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(((uintptr_t)workspace & 7) == 0, "tg_ns_hop_labor: the workspace must be 8-byte aligned");
    LaborParams p;
    p.ptrs = csc->ptrs;
    p.indices = csc->indices;
    p.timestamps = csc->timestamps;
    p.ptrs32 = csc->ptrs32;
    p.indices32 = csc->indices32;
    p.vertices = in->vertices;
    p.states = mode == TG_FILTER_NONE ? nullptr : flt->states;
    p.call_ids = in->call_ids;
    p.m = in->m;
    p.long_column = g_long_column.load();
    p.k = in->fanout;
    p.filter_mode = mode;
    p.forward = (flt && flt->forward) ? 1 : 0;
    p.tag = in->rng_tag ? in->rng_tag : TG_TAG_LABOR;
    p.layer = (uint32_t)layer;
    p.win_lo = flt ? flt->win_lo : 0;
    p.win_hi = flt ? flt->win_hi : 0;
    p.seed = rng->seed;
    p.call_id = rng->call_id;
    p.cnt = out->cnt;
    p.offsets = out->offsets;
    p.neighbors = out->neighbors;
    p.edge_ptrs = out->edge_ptrs;
    p.parents = out->parents;
    p.states_out = mode == TG_FILTER_NONE ? nullptr : states_out;
    p.n_long = static_cast<unsigned long long *>(workspace);
    p.long_list = static_cast<int64_t *>(workspace) + LB_WS_HEAD;
    auto blocks = [](int64_t items, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min((items + 255) / 256, cap)); };
    TG_HIP(hipMemsetAsync(p.n_long, 0, sizeof(unsigned long long), stream));
    const unsigned sb = blocks(p.m * 64, (int64_t)1 << 22);
    const bool filtered = mode != TG_FILTER_NONE;
    if (p.indices32)
        filtered ? labor_launch<true, true>(p, sb, stream) : labor_launch<true, false>(p, sb, stream);
    else
        filtered ? labor_launch<false, true>(p, sb, stream) : labor_launch<false, false>(p, sb, stream);
    hipLaunchKernelGGL(labor_scan_kernel, dim3(1), dim3(SCAN1_THREADS), 0, stream, p);
    hipLaunchKernelGGL(labor_emit_kernel, dim3(blocks(p.m * p.k, 256 * 32)), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(labor_gather_kernel, dim3(blocks(p.m * p.k, 256 * 32)), dim3(256), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
