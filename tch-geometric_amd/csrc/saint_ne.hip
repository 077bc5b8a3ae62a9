// GraphSAINT's node and edge samplers (tg_saint_node_nodes, tg_saint_edge_nodes; include/tchgeo.h).
//
// Per mini-batch g of B slots, slot i consumes ONE Philox block, the draw (call key of (seed, call id + g, tag), i, 0, 0):
// lo = w0 | w1 << 32, hi = w2 | w3 << 32, every bounded pick floor(x * n / 2^64).
//   node: e = pick(lo, n_edges), the vertex indices[e] at position i                                    P = B
//   edge: t = pick(lo, n_cols + n_rows); a listed column c (t < n_cols) gives k = pick(hi, deg(c)), source =
//         csc.indices[csc.ptrs[c] + k], target = c; a listed row r gives source = r, target = csr.indices[csr.ptrs[r] + k];
//         the source at position i, the target at position B + i                                        P = 2 B
// nodes[g] = the distinct vertices in order of their first position, by saint_dedup.h (the rule and the tables of
// tg_saint_rw_nodes).  A slot that is refused (an id outside its table, a listed major without entries) visits nothing.
//
// The draw is latency-bound: one random gather per slot (node), a chain of three dependent random reads per slot (edge:
// the list entry, the two offsets, the index word).  So the draw runs in STAGES over all the slots a lane owns: the loads
// of a stage are issued for every slot before any is consumed, and the table is touched only after the last stage.
// LDS form: ONE workgroup draws and dedups ONE mini-batch; a lane owns slots tid, tid + nt, ... -- at most 12 (node) / 6
//   (edge) of them at P = 12 288 -- held in registers across the stages.  The LDS request is sized by P (nsu_plan), so
//   small mini-batches share a CU.
// Flat form: any P.  clear | draw (one lane per slot, blockIdx.y = the mini-batch of the round, u32 visit words in the
//   workspace: the wavefronts of the grid are the loads in flight) | insert | flag | apply.
#include <algorithm>

#include "rw_walk.h"
#include "saint_dedup.h"

namespace tg {

constexpr int32_t SNE_STATUS_EMPTY = 4;   // status bit 2: a listed major without entries
constexpr int SNE_NODE_SLOTS = 12;        // LDS form: slots a lane owns at most, P <= 12 288 over 1 024 lanes
constexpr int SNE_EDGE_SLOTS = 6;
constexpr int64_t SNE_LDS_MAX_P = (int64_t)NSU_THREADS * SNE_NODE_SLOTS; // 12 288: nsu_plan's table fits 160 KiB up to here

struct SneArgs {
    CsrView g, g2;            // node: the graph, -; edge: csc, csr
    int64_t n_major, n_major2, n_edges;
    const int64_t *cols, *rows;
    int64_t n_cols, n_rows;
    int64_t id_bound;
    int64_t *nodes, *counts;
    int64_t pitch, counts_stride, n_batches, B, P;
    uint64_t seed, call_id;   // of mini-batch 0 of the round
    int32_t *status;
    uint32_t cap_mask, hash_shift;
    // flat form: the round's tables
    unsigned char *ws;
    int64_t batch_bytes, vals_off, slot_off, tile_off, visit_off;
};

// ---- the draw, stage by stage ------------------------------------------------------------------------------------------
// A stage is straight-line code: between one slot's load and the next slot's stands no branch but the uniform test that
// some lane has such a slot.  A slot that is off (past B) or refused keeps loading, from `a.nodes` (the head of the round's
// output: 16 readable bytes, nobody's input), and what it loads is dropped; refusals are collected in the lane's `err`
// word and reach `status` with one atomic at the end.  The word width of ptrs / indices is uniform (the host passes the
// u32 shadows of both graphs or of neither).
__device__ __forceinline__ void sne_report(const SneArgs &a, int32_t err) {
    if (err) atomicOr(a.status, err);
}

// node sampler: the slot's vertex (not yet checked)
template <bool I32> __device__ __forceinline__ int64_t sne_node_load(const SneArgs &a, CallKey ck, uint64_t i, bool on) {
    const int64_t e = on ? (int64_t)bounded64(draw(ck, i, 0u, 0u).a(), (uint64_t)a.n_edges) : 0; // n_edges > 0
    return I32 ? (int64_t)a.g.indices32[e] : a.g.indices[e];
}
// its visit word: SAINT_NONE (and status bit 1) outside [0, id_bound)
__device__ __forceinline__ uint32_t sne_node_visit(const SneArgs &a, int64_t v, bool on, int32_t &err) {
    const bool ok = (uint64_t)v < (uint64_t)a.id_bound;
    if (on && !ok) err |= SAINT_STATUS_RANGE;
    return on && ok ? (uint32_t)v : SAINT_NONE;
}

// edge sampler: a slot between its stages.  `live` falls when the slot is off or refused.
struct SneEdgeSlot {
    uint64_t hi;      // the draw's second half: picks the entry inside the major
    int64_t major;    // stage 1: the listed column / row
    uint32_t major32; // from stage 2 on: the same, SAINT_NONE when it is no id (>= id_bound <= 2^31)
    int64_t b, e;     // stage 2: its offsets
    int64_t other;    // stage 3: the entry's minor
    bool side, live;  // side: a row of the CSR
};
// stage 1: the draw and the list entry (a slot that is off reads entry 0: n_cols + n_rows > 0)
__device__ __forceinline__ void sne_edge_list(const SneArgs &a, CallKey ck, uint64_t i, bool on, SneEdgeSlot &s) {
    const Draw d = draw(ck, i, 0u, 0u);
    const int64_t t = on ? (int64_t)bounded64(d.a(), (uint64_t)(a.n_cols + a.n_rows)) : 0;
    s.hi = d.b();
    s.side = t >= a.n_cols;
    s.major = *(s.side ? a.rows + (t - a.n_cols) : a.cols + t);
    s.live = on;
}
// stage 2: the major's two offsets, one load; a major outside its graph never indexes ptrs
template <bool P32> __device__ __forceinline__ void sne_edge_offsets(const SneArgs &a, SneEdgeSlot &s, int32_t &err) {
    const int64_t m = s.major;
    const bool in = (uint64_t)m < (uint64_t)(s.side ? a.n_major2 : a.n_major);
    if (s.live && !in) err |= SAINT_STATUS_RANGE;
    s.live = s.live && in;
    s.major32 = (uint64_t)m < (uint64_t)a.id_bound ? (uint32_t)m : SAINT_NONE;
    if (P32) {
        const uint32_t *p = s.live ? (s.side ? a.g2.ptrs32 : a.g.ptrs32) + m : reinterpret_cast<const uint32_t *>(a.nodes);
        s.b = (int64_t)p[0], s.e = (int64_t)p[1];
    } else {
        const int64_t *p = s.live ? (s.side ? a.g2.ptrs : a.g.ptrs) + m : a.nodes;
        s.b = p[0], s.e = p[1];
    }
}
// stage 3: the entry
template <bool I32> __device__ __forceinline__ void sne_edge_entry(const SneArgs &a, SneEdgeSlot &s, int32_t &err) {
    const bool empty = s.e <= s.b;
    if (s.live && empty) err |= SNE_STATUS_EMPTY;
    s.live = s.live && !empty;
    const int64_t at = s.b + (int64_t)bounded64(s.hi, (uint64_t)(s.e - s.b));
    if (I32)
        s.other = (int64_t)*(s.live ? (s.side ? a.g2.indices32 : a.g.indices32) + at : reinterpret_cast<const uint32_t *>(a.nodes));
    else
        s.other = *(s.live ? (s.side ? a.g2.indices : a.g.indices) + at : a.nodes);
}
// the ends: false (and status bit 1) when either lies outside [0, id_bound)
__device__ __forceinline__ bool sne_edge_ends(const SneArgs &a, const SneEdgeSlot &s, uint32_t &src, uint32_t &dst, int32_t &err) {
    const bool ok = s.major32 != SAINT_NONE && (uint64_t)s.other < (uint64_t)a.id_bound;
    if (s.live && !ok) err |= SAINT_STATUS_RANGE;
    src = s.side ? s.major32 : (uint32_t)s.other;
    dst = s.side ? (uint32_t)s.other : s.major32;
    return s.live && ok;
}

// the stages over a lane's slots i0, i0 + step, ... (K of them at most); `on_slot(k, i, ok, src, dst)` gets every slot < B
template <int K, bool P32, bool I32, typename F>
__device__ __forceinline__ void sne_edge_stages(const SneArgs &a, CallKey ck, int64_t i0, int64_t step, int32_t &err, F on_slot) {
    SneEdgeSlot s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * step >= a.B) break; // uniform: no lane has a slot k
        sne_edge_list(a, ck, (uint64_t)(i0 + k * step), i0 + k * step < a.B, s[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * step >= a.B) break;
        sne_edge_offsets<P32>(a, s[k], err);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * step >= a.B) break;
        sne_edge_entry<I32>(a, s[k], err);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * step >= a.B) break;
        uint32_t src, dst;
        const bool ok = sne_edge_ends(a, s[k], src, dst, err);
        if (i0 + k * step < a.B) on_slot(i0 + k * step, ok, src, dst);
    }
}
template <int K, typename F>
__device__ __forceinline__ void sne_edge_draw(const SneArgs &a, CallKey ck, int64_t i0, int64_t step, int32_t &err, F on_slot) {
    if (a.g.ptrs32) { // uniform
        if (a.g.indices32)
            sne_edge_stages<K, true, true>(a, ck, i0, step, err, on_slot);
        else
            sne_edge_stages<K, true, false>(a, ck, i0, step, err, on_slot);
    } else if (a.g.indices32) {
        sne_edge_stages<K, false, true>(a, ck, i0, step, err, on_slot);
    } else {
        sne_edge_stages<K, false, false>(a, ck, i0, step, err, on_slot);
    }
}

template <int K, bool I32, typename F>
__device__ __forceinline__ void sne_node_stages(const SneArgs &a, CallKey ck, int64_t i0, int64_t step, int32_t &err, F on_slot) {
    int64_t v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { // every gather of the lane is in flight before the first is consumed
        if (k * step >= a.B) break; // uniform
        v[k] = sne_node_load<I32>(a, ck, (uint64_t)(i0 + k * step), i0 + k * step < a.B);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * step >= a.B) break;
        const bool on = i0 + k * step < a.B;
        const uint32_t w = sne_node_visit(a, v[k], on, err);
        if (on) on_slot(i0 + k * step, w);
    }
}
template <int K, typename F>
__device__ __forceinline__ void sne_node_draw(const SneArgs &a, CallKey ck, int64_t i0, int64_t step, int32_t &err, F on_slot) {
    if (a.g.indices32) // uniform
        sne_node_stages<K, true>(a, ck, i0, step, err, on_slot);
    else
        sne_node_stages<K, false>(a, ck, i0, step, err, on_slot);
}

// ---- LDS form --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t sne_lds_visit(nsu_k32 *keys, uint32_t *vals, const SneArgs &a, uint32_t v, int p) {
    const uint32_t s = nsu_insert<nsu_k32>(keys, a.cap_mask, a.hash_shift, v);
    atomicMin(&vals[s], (uint32_t)p);
    return (uint16_t)s;
}

template <bool EDGE> __global__ void __launch_bounds__(NSU_THREADS) sne_lds_kernel(const SneArgs a) {
    extern __shared__ __align__(16) unsigned char sne_lds[];
    __shared__ uint32_t s_wave[NSU_THREADS / 64];
    const uint32_t cap = a.cap_mask + 1;
    nsu_k32 *keys = reinterpret_cast<nsu_k32 *>(sne_lds);
    uint32_t *vals = keys + cap;
    uint16_t *loc = reinterpret_cast<uint16_t *>(vals + cap); // [P]: the position's slot
    const int tid = threadIdx.x, nt = blockDim.x;
    const int B = (int)a.B, n = (int)a.P;
    int32_t err = 0;

    for (int64_t b = blockIdx.x; b < a.n_batches; b += gridDim.x) {
        for (uint32_t s = tid; s < cap; s += nt) {
            keys[s] = nsu_empty<nsu_k32>();
            vals[s] = NSU_UNSEEN;
        }
        __syncthreads(); // also: the previous mini-batch is done with `loc`
        const CallKey ck = call_key(a.seed, a.call_id + (uint64_t)b, EDGE ? TG_TAG_SAINT_EDGE : TG_TAG_SAINT_NODE);
        // a position nobody visits takes slot 0, whose value is not that position
        if (!EDGE)
            sne_node_draw<SNE_NODE_SLOTS>(a, ck, tid, nt, err, [&](int64_t i, uint32_t w) {
                loc[i] = w == SAINT_NONE ? (uint16_t)0 : sne_lds_visit(keys, vals, a, w, (int)i);
            });
        else
            sne_edge_draw<SNE_EDGE_SLOTS>(a, ck, tid, nt, err, [&](int64_t i, bool ok, uint32_t src, uint32_t dst) {
                loc[i] = ok ? sne_lds_visit(keys, vals, a, src, (int)i) : (uint16_t)0;
                loc[B + i] = ok ? sne_lds_visit(keys, vals, a, dst, B + (int)i) : (uint16_t)0;
            });
        __syncthreads(); // the whole mini-batch is in the table
        saint_lds_rank_store(a, b, keys, vals, loc, n, tid, nt, s_wave);
        __syncthreads(); // the next mini-batch clears the table
    }
    sne_report(a, err);
}

// ---- flat form: one lane per slot of a mini-batch; blockIdx.y = the mini-batch ------------------------------------------
template <bool EDGE> __global__ void __launch_bounds__(NSU_TILE_THREADS) sne_draw_kernel(const SneArgs a) {
    const int64_t b = blockIdx.y;
    uint32_t *visit = SaintBatch(a, b).visit;
    const CallKey ck = call_key(a.seed, a.call_id + (uint64_t)b, EDGE ? TG_TAG_SAINT_EDGE : TG_TAG_SAINT_NODE);
    int32_t err = 0;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < a.B; i0 += step) {
        if (!EDGE)
            sne_node_draw<1>(a, ck, i0, step, err, [&](int64_t i, uint32_t w) { visit[i] = w; });
        else
            sne_edge_draw<1>(a, ck, i0, step, err, [&](int64_t i, bool ok, uint32_t src, uint32_t dst) {
                visit[i] = ok ? src : SAINT_NONE;
                visit[a.B + i] = ok ? dst : SAINT_NONE;
            });
    }
    sne_report(a, err);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static inline int sne_plan(int64_t P, const char *who, SaintPlan &pl) {
    TG_REQUIRE(P >= 0 && P <= NSU_MAX_NODES, "%s: positions = %lld outside [0, 2^30]", who, (long long)P);
    if (const int rc = saint_plan(P, who, pl)) return rc;
    if (P > SNE_LDS_MAX_P) pl.nsu.lds_ok = 0; // the LDS form's lanes hold at most 12 slots
    return TG_OK;
}

template <bool EDGE> static int sne_launch_lds(const SneArgs &a, const SaintPlan &pl, hipStream_t stream) {
    const int64_t dyn = pl.nsu.lds_bytes - NSU_STATIC_LDS;
    static std::atomic<int64_t> raised[64]; // zero-initialised; one table per kernel
    if (const int rc = saint_raise_lds(reinterpret_cast<const void *>(sne_lds_kernel<EDGE>), raised, dyn)) return rc;
    const unsigned grid = (unsigned)(a.n_batches < 16384 ? a.n_batches : 16384);
    hipLaunchKernelGGL(sne_lds_kernel<EDGE>, dim3(grid), dim3(pl.nsu.threads), (size_t)dyn, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <bool EDGE> static int sne_launch_flat(const SneArgs &a, const SaintPlan &pl, hipStream_t stream) {
    if (const int rc = saint_launch_clear(a, pl, stream)) return rc;
    hipLaunchKernelGGL(sne_draw_kernel<EDGE>, dim3(grid_1d(a.B, NSU_TILE_THREADS), (unsigned)a.n_batches), dim3(NSU_TILE_THREADS), 0,
                       stream, a);
    TG_LAUNCH_CHECK();
    return saint_launch_dedup(a, pl, stream);
}

static inline CsrView sne_view(const tg_graph *g) {
    return g ? CsrView{g->ptrs, g->indices, g->ptrs32, g->indices32, nullptr, 0} : CsrView{};
}
// a slot's side is a lane's affair, the word width must not be: the shadows of both graphs or of neither (equal words)
static inline void sne_same_width(CsrView &g, CsrView &g2, bool has2) {
    if (has2 && !(g.ptrs32 && g2.ptrs32)) g.ptrs32 = g2.ptrs32 = nullptr;
    if (has2 && !(g.indices32 && g2.indices32)) g.indices32 = g2.indices32 = nullptr;
}

// what the two entry points share behind their own checks: the output's checks, the form, the rounds
template <bool EDGE>
static int sne_run(const char *who, SneArgs a, int64_t n_batches, const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status,
                   void *workspace, int64_t workspace_bytes, int32_t form, void *stream_) {
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    TG_REQUIRE(a.id_bound >= 1, "%s: id_bound = %lld, at least 1 expected", who, (long long)a.id_bound);
    if (a.id_bound > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: id_bound = %lld does not fit the 32-bit hash keys", who, (long long)a.id_bound);
    SaintPlan pl;
    if (const int rc = sne_plan(EDGE ? 2 * a.B : a.B, who, pl)) return rc;
    TG_REQUIRE(out->pitch_nodes >= pl.P, "%s: pitch_nodes = %lld below the %lld positions of a mini-batch", who,
               (long long)out->pitch_nodes, (long long)pl.P);
    TG_REQUIRE(out->counts_stride >= 1, "%s: counts_stride = %lld, at least 1 expected", who, (long long)out->counts_stride);
    TG_REQUIRE(out->nodes && out->counts && status, "%s: null nodes / counts / status", who);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    const bool enough = workspace && workspace_bytes >= pl.batch_bytes;
    TG_REQUIRE(form != 2 || enough, "%s: workspace too small (%lld < %lld, the size of one mini-batch)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    if (n_batches == 0 || a.B == 0) return TG_OK; // nothing to launch: no device is asked either
    const bool lds = form != 2 && nsu_fits(pl.nsu, nsu_device_lds_limit());
    TG_REQUIRE(form != 1 || lds, "%s: form 1: a table of %lld slots (%lld bytes of LDS) does not fit a workgroup", who,
               (long long)pl.nsu.table_cap, (long long)pl.nsu.lds_bytes);
    TG_REQUIRE(lds || enough, "%s: workspace too small (%lld < %lld, the size of one mini-batch)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    hipStream_t stream = (hipStream_t)stream_;

    const int64_t round = lds ? n_batches : std::min(std::min(workspace_bytes / pl.batch_bytes, NSU_ROUND_MAX), n_batches);
    a.pitch = out->pitch_nodes, a.counts_stride = out->counts_stride;
    a.seed = rng->seed;
    a.status = status;
    saint_plan_args(pl, workspace, a);
    for (int64_t b0 = 0; b0 < n_batches; b0 += round) {
        a.nodes = out->nodes + b0 * out->pitch_nodes, a.counts = out->counts + b0 * out->counts_stride;
        a.n_batches = std::min(round, n_batches - b0);
        a.call_id = rng->call_id + (uint64_t)b0;
        if (const int rc = lds ? sne_launch_lds<EDGE>(a, pl, stream) : sne_launch_flat<EDGE>(a, pl, stream)) return rc;
    }
    return TG_OK;
}

static inline int sne_graph_ok(const tg_graph *g, bool need_ptrs, const char *who, const char *name) {
    TG_REQUIRE((!need_ptrs || g->ptrs) && (g->indices || g->n_edges == 0), "%s: null %s graph", who, name);
    TG_REQUIRE(g->n_major >= 0 && g->n_edges >= 0, "%s: negative %s graph size", who, name);
    return TG_OK;
}

} // namespace tg

extern "C" int tg_saint_ne_form(int64_t positions, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_saint_ne_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    SaintPlan pl;
    if (const int rc = sne_plan(positions, who, pl)) return rc;
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : nsu_device_lds_limit();
    *form = nsu_fits(pl.nsu, limit) ? 1 : 2;
    *lds_bytes = pl.nsu.lds_bytes;
    return TG_OK;
}

extern "C" int tg_saint_ne_workspace_bytes(int64_t n_batches, int64_t positions, int32_t form, int64_t *bytes,
                                           int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_saint_ne_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    SaintPlan pl;
    if (const int rc = sne_plan(positions, who, pl)) return rc;
    TG_REQUIRE(n_batches == 0 || pl.batch_bytes <= INT64_MAX / n_batches, "%s: %lld mini-batches of %lld bytes overflow int64", who,
               (long long)n_batches, (long long)pl.batch_bytes);
    *bytes_min = pl.batch_bytes;
    const bool lds = form == 1 || (form == 0 && nsu_fits(pl.nsu, nsu_device_lds_limit())); // forced forms ask no device
    *bytes = lds ? 0 : pl.batch_bytes * n_batches;
    return TG_OK;
}

extern "C" int tg_saint_node_nodes(const tg_graph *graph, int64_t id_bound, int64_t n_batches, int64_t batch_size,
                                   const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status, void *workspace,
                                   int64_t workspace_bytes, int32_t form, void *stream) {
    using namespace tg;
    const char *who = "tg_saint_node_nodes";
    TG_REQUIRE(graph && rng && out, "%s: null argument", who);
    if (const int rc = sne_graph_ok(graph, false, who, "the")) return rc;
    TG_REQUIRE(batch_size >= 0 && batch_size <= NSU_MAX_NODES, "%s: batch_size = %lld outside [0, 2^30]", who, (long long)batch_size);
    TG_REQUIRE(graph->n_edges > 0 || batch_size == 0, "%s: a graph without entries has nothing to draw", who);
    SneArgs a{};
    a.g = sne_view(graph);
    a.n_edges = graph->n_edges;
    a.id_bound = id_bound;
    a.B = batch_size;
    return sne_run<false>(who, a, n_batches, rng, out, status, workspace, workspace_bytes, form, stream);
}

extern "C" int tg_saint_edge_nodes(const tg_saint_edge_in *in, int64_t id_bound, int64_t n_batches, int64_t batch_size,
                                   const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status, void *workspace,
                                   int64_t workspace_bytes, int32_t form, void *stream) {
    using namespace tg;
    const char *who = "tg_saint_edge_nodes";
    TG_REQUIRE(in && rng && out, "%s: null argument", who);
    TG_REQUIRE(in->n_cols >= 0 && in->n_rows >= 0, "%s: negative list size", who);
    TG_REQUIRE(in->n_cols <= INT64_MAX - in->n_rows, "%s: n_cols + n_rows overflows int64", who);
    TG_REQUIRE((in->csc || in->n_cols == 0) && (in->csr || in->n_rows == 0), "%s: a list without its graph", who);
    TG_REQUIRE((in->cols || in->n_cols == 0) && (in->rows || in->n_rows == 0), "%s: null cols / rows", who);
    if (in->csc)
        if (const int rc = sne_graph_ok(in->csc, true, who, "csc")) return rc;
    if (in->csr)
        if (const int rc = sne_graph_ok(in->csr, true, who, "csr")) return rc;
    TG_REQUIRE(batch_size >= 0 && batch_size <= NSU_MAX_NODES / 2, "%s: batch_size = %lld outside [0, 2^29]", who,
               (long long)batch_size);
    TG_REQUIRE(in->n_cols + in->n_rows > 0 || batch_size == 0, "%s: empty lists have nothing to draw", who);
    SneArgs a{};
    a.g = sne_view(in->csc), a.g2 = sne_view(in->csr);
    if (!in->csc) std::swap(a.g, a.g2); // the width is read from g
    sne_same_width(a.g, a.g2, in->csc && in->csr);
    if (!in->csc) std::swap(a.g, a.g2);
    a.n_major = in->csc ? in->csc->n_major : 0, a.n_major2 = in->csr ? in->csr->n_major : 0;
    a.cols = in->cols, a.rows = in->rows;
    a.n_cols = in->n_cols, a.n_rows = in->n_rows;
    a.id_bound = id_bound;
    a.B = batch_size;
    return sne_run<true>(who, a, n_batches, rng, out, status, workspace, workspace_bytes, form, stream);
}
