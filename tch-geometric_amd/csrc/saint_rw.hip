// GraphSAINT's random-walk sampler (tg_saint_rw_nodes, tg_saint_coverage_add, tg_saint_norm; include/tchgeo.h).
//
// tg_saint_rw_nodes, per mini-batch g of B roots: walker i walks T uniform steps (walk_step of rw_walk.h with the draw
// address of tg_random_walk under call id + g, so its vertices are row i of that call), the visit at step l sits at
// position p = l * B + i, and nodes[g] = the distinct visited vertices in order of their first position -- the rule of
// ns_unique.hip on a list that is never stored as int64 rows.  Both forms compute it as that file does: the key is claimed
// with atomicCAS, atomicMin leaves the id's first position in the slot's value, position p is a first occurrence iff
// value[slot(p)] == p, ranks are the exclusive scan of those flags in position order, nodes[rank] = key of the slot.
// A walker that stopped at a dead end repeats its last slot (LDS form) / vertex (flat form) at its remaining positions, a
// root outside the graph takes slot 0 / no vertex: such a position is behind the slot's first one (or the slot holds
// another position, or none), so it is never a first occurrence.
//
// LDS form: ONE workgroup walks and dedups ONE mini-batch; keys, values and a u16 slot word per position live in LDS and
//   only the root loads, the walk's gathers and the node stores touch global memory.  nsu_plan's sizes: 2^k >= 4/3 P
//   slots of 8 bytes + 2 bytes per position, P <= 12 288 in 160 KiB -- at that size a CU holds ONE such workgroup.
// Flat form: any P.  clear | walk (one lane per walker of all mini-batches, u32 visit lists in the workspace) | insert |
//   flag + tile counts | apply, the last three over tiles of positions as in ns_unique.hip.
// Every probe loop is capped at the table size.
//
// tg_saint_coverage_add / tg_saint_norm: the counters GraphSAINT pre-samples and the two normalisation vectors.
#include <algorithm>

#include "rw_walk.h"
#include "saint_dedup.h"

namespace tg {

constexpr uint32_t SRW_NONE = SAINT_NONE;
constexpr int32_t SRW_STATUS_RANGE = SAINT_STATUS_RANGE;
constexpr int SRW_NORM_CHUNK = 1024;       // CSC offsets a wavefront normalises per chunk

struct SrwArgs {
    CsrView g;
    int64_t n_major;
    const int64_t *roots; // mini-batch 0 of the round
    int64_t *nodes, *counts;
    int64_t pitch, counts_stride, n_batches, B, T, P;
    uint64_t seed, call_id; // of mini-batch 0 of the round
    int32_t *status;
    uint32_t cap_mask, hash_shift;
    // flat form: the round's tables
    unsigned char *ws;
    int64_t batch_bytes, vals_off, slot_off, tile_off, visit_off;
};

__device__ __forceinline__ WalkProbs srw_probs() { return WalkProbs{1.0f, 1.0f, 1.0f}; } // p = q = 1

// ---- LDS form --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NSU_THREADS) srw_lds_kernel(const SrwArgs a) {
    extern __shared__ __align__(16) unsigned char srw_lds[];
    __shared__ uint32_t s_wave[NSU_THREADS / 64];
    const uint32_t cap = a.cap_mask + 1;
    nsu_k32 *keys = reinterpret_cast<nsu_k32 *>(srw_lds);
    uint32_t *vals = keys + cap;
    uint16_t *loc = reinterpret_cast<uint16_t *>(vals + cap); // [P]: the position's slot
    const int tid = threadIdx.x, nt = blockDim.x;
    const int B = (int)a.B, T = (int)a.T, n = (int)a.P;
    const WalkProbs pr = srw_probs();

    for (int64_t b = blockIdx.x; b < a.n_batches; b += gridDim.x) {
        for (uint32_t s = tid; s < cap; s += nt) {
            keys[s] = nsu_empty<nsu_k32>();
            vals[s] = NSU_UNSEEN;
        }
        __syncthreads(); // also: the previous mini-batch is done with `loc`
        const CallKey ck = call_key(a.seed, a.call_id + (uint64_t)b, TAG_RW);
        const int64_t *roots = a.roots + b * a.B;
        for (int i = tid; i < B; i += nt) {
            int64_t prev = -1, cur = roots[i];
            if ((uint64_t)cur >= (uint64_t)a.n_major) { // never indexes ptrs; slot 0's value is no position of this walker
                atomicOr(a.status, SRW_STATUS_RANGE);
                for (int l = 0; l <= T; ++l) loc[l * B + i] = 0;
                continue;
            }
            for (int l = 0;; ++l) {
                const int p = l * B + i;
                const uint32_t s = nsu_insert<nsu_k32>(keys, a.cap_mask, a.hash_shift, (nsu_k32)cur);
                atomicMin(&vals[s], (uint32_t)p);
                loc[p] = (uint16_t)s;
                if (l == T) break;
                if (!walk_step(a.g, ck, (uint64_t)i, (uint32_t)l, pr, true, prev, cur)) { // a dead end: the walk is over
                    for (int k = l + 1; k <= T; ++k) loc[k * B + i] = (uint16_t)s;
                    break;
                }
            }
        }
        __syncthreads();
        // first occurrences, ranked in position order: a thread owns a contiguous run of positions (saint_dedup.h's
        // saint_lds_rank_store, kept in line here: this kernel's code is the one its measurements were taken on)
        const int per = (n + nt - 1) / nt; // <= NSU_MAX_PER_THREAD
        const int p0 = min(n, tid * per), p1 = min(n, p0 + per);
        uint32_t first = 0;
        for (int p = p0; p < p1; ++p)
            if (vals[loc[p]] == (uint32_t)p) first |= 1u << (p - p0);
        uint32_t n_unique;
        uint32_t rank = nsu_scan((uint32_t)__popc(first), s_wave, &n_unique);
        int64_t *nodes = a.nodes + b * a.pitch;
        for (uint32_t f = first; f;) {
            const int p = p0 + __ffs(f) - 1;
            f &= f - 1;
            nodes[rank++] = (int64_t)keys[loc[p]];
        }
        if (tid == 0) a.counts[b * a.counts_stride] = (int64_t)n_unique;
        __syncthreads(); // the next mini-batch clears the table
    }
}

// ---- flat form -------------------------------------------------------------------------------------------------------
// one lane per walker of the round: the visit list of its mini-batch in position order
__global__ void __launch_bounds__(NSU_TILE_THREADS) srw_walk_kernel(const SrwArgs a) {
    const WalkProbs pr = srw_probs();
    const int64_t total = a.n_batches * a.B;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = w / a.B, i = w - b * a.B;
        uint32_t *visit = SaintBatch(a, b).visit;
        int64_t prev = -1, cur = a.roots[w];
        if ((uint64_t)cur >= (uint64_t)a.n_major) { // never indexes ptrs
            atomicOr(a.status, SRW_STATUS_RANGE);
            for (int64_t l = 0; l <= a.T; ++l) visit[l * a.B + i] = SRW_NONE;
            continue;
        }
        const CallKey ck = call_key(a.seed, a.call_id + (uint64_t)b, TAG_RW);
        bool dead = false;
        for (int64_t l = 0;; ++l) {
            visit[l * a.B + i] = (uint32_t)cur; // a stopped walker repeats its last vertex
            if (l == a.T) break;
            if (!dead) dead = !walk_step(a.g, ck, (uint64_t)i, (uint32_t)l, pr, true, prev, cur);
        }
    }
}

// ---- coverage counters -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) srw_cover_nodes_kernel(const int64_t *__restrict__ nodes, int64_t pitch,
                                                              const int64_t *__restrict__ counts, int64_t counts_stride,
                                                              int64_t n_batches, int64_t *node_count, int64_t n_nodes,
                                                              int32_t *status) {
    for (int64_t b = blockIdx.y; b < n_batches; b += gridDim.y) {
        const int64_t n = nsu_clamp(counts[b * counts_stride], pitch);
        for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
            const int64_t v = nodes[b * pitch + j];
            if ((uint64_t)v < (uint64_t)n_nodes)
                atomicAdd(reinterpret_cast<unsigned long long *>(&node_count[v]), 1ull);
            else
                atomicOr(status, SRW_STATUS_RANGE);
        }
    }
}

__global__ void __launch_bounds__(256) srw_cover_edges_kernel(const int64_t *__restrict__ edge_ids, int64_t n_edge_ids,
                                                              int64_t *edge_count, int64_t n_edges, int32_t *status) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_edge_ids; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = edge_ids[j];
        if ((uint64_t)e < (uint64_t)n_edges)
            atomicAdd(reinterpret_cast<unsigned long long *>(&edge_count[e]), 1ull);
        else
            atomicOr(status, SRW_STATUS_RANGE);
    }
}

// ---- norms ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) srw_node_norm_kernel(const int64_t *__restrict__ node_count, int64_t n_major,
                                                            float n_samples, float *node_norm) {
    const float n = (float)n_major;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_major; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = node_count[v];
        const float d = c == 0 ? 0.1f : (float)c;
        node_norm[v] = (n_samples / d) / n;
    }
}

// the last column c in [lo, hi] with ptr(c) <= e
__device__ __forceinline__ int64_t srw_col_of(const CsrView &g, int64_t lo, int64_t hi, int64_t e) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (g.ptr(mid) <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// a wavefront takes a chunk of consecutive CSC offsets (a hub column is many chunks); the chunk's columns lie between
// those of its first and last offset, found once per chunk, so an offset's column is a short search in cached offsets
__global__ void __launch_bounds__(256) srw_edge_norm_kernel(const CsrView g, int64_t n_major, int64_t n_edges,
                                                            const int64_t *__restrict__ node_count,
                                                            const int64_t *__restrict__ edge_count, float *edge_norm) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (n_edges + SRW_NORM_CHUNK - 1) / SRW_NORM_CHUNK;
    for (int64_t ch = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; ch < n_chunks;
         ch += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t e0 = ch * SRW_NORM_CHUNK, e1 = min(n_edges, e0 + SRW_NORM_CHUNK);
        const int64_t c0 = srw_col_of(g, 0, n_major - 1, e0), c1 = srw_col_of(g, c0, n_major - 1, e1 - 1);
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t c = srw_col_of(g, c0, c1, e);
            const float r = (float)node_count[c] / (float)edge_count[e];
            edge_norm[e] = r != r ? 0.1f : fminf(fmaxf(r, 0.0f), 1e4f); // 0/0 -> 0.1, x/0 = inf -> 1e4
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
typedef SaintPlan SrwPlan;

static inline int srw_plan(int64_t B, int64_t T, const char *who, SrwPlan &pl) {
    TG_REQUIRE(B >= 0, "%s: batch_size = %lld is negative", who, (long long)B);
    TG_REQUIRE(T >= 1, "%s: walk_length = %lld, at least 1 expected", who, (long long)T);
    TG_REQUIRE(T < NSU_MAX_NODES && B <= NSU_MAX_NODES / (T + 1), "%s: batch_size * (walk_length + 1) = %lld * %lld above 2^30",
               who, (long long)B, (long long)(T + 1));
    return saint_plan(B * (T + 1), who, pl); // ids below 2^31: 32-bit keys
}

static int srw_launch_lds(const SrwArgs &a, const SrwPlan &pl, hipStream_t stream) {
    const int64_t dyn = pl.nsu.lds_bytes - NSU_STATIC_LDS;
    static std::atomic<int64_t> raised[64]; // zero-initialised
    if (const int rc = saint_raise_lds(reinterpret_cast<const void *>(srw_lds_kernel), raised, dyn)) return rc;
    const unsigned grid = (unsigned)(a.n_batches < 16384 ? a.n_batches : 16384);
    hipLaunchKernelGGL(srw_lds_kernel, dim3(grid), dim3(pl.nsu.threads), (size_t)dyn, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

static int srw_launch_flat(const SrwArgs &a, const SrwPlan &pl, hipStream_t stream) {
    if (const int rc = saint_launch_clear(a, pl, stream)) return rc;
    hipLaunchKernelGGL(srw_walk_kernel, dim3(grid_1d(a.n_batches * a.B, NSU_TILE_THREADS)), dim3(NSU_TILE_THREADS), 0, stream, a);
    TG_LAUNCH_CHECK();
    return saint_launch_dedup(a, pl, stream);
}

} // namespace tg

extern "C" int tg_saint_rw_capacity(int64_t batch_size, int64_t walk_length, int64_t *positions) {
    using namespace tg;
    const char *who = "tg_saint_rw_capacity";
    TG_REQUIRE(positions, "%s: null output", who);
    SrwPlan pl;
    if (const int rc = srw_plan(batch_size, walk_length, who, pl)) return rc;
    *positions = pl.P;
    return TG_OK;
}

extern "C" int tg_saint_rw_form(int64_t batch_size, int64_t walk_length, int64_t lds_limit_bytes, int32_t *form,
                                int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_saint_rw_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    SrwPlan pl;
    if (const int rc = srw_plan(batch_size, walk_length, who, pl)) return rc;
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : nsu_device_lds_limit();
    *form = nsu_fits(pl.nsu, limit) ? 1 : 2;
    *lds_bytes = pl.nsu.lds_bytes;
    return TG_OK;
}

extern "C" int tg_saint_rw_workspace_bytes(int64_t n_batches, int64_t batch_size, int64_t walk_length, int32_t form,
                                           int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_saint_rw_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    SrwPlan pl;
    if (const int rc = srw_plan(batch_size, walk_length, who, pl)) return rc;
    TG_REQUIRE(n_batches == 0 || pl.batch_bytes <= INT64_MAX / n_batches, "%s: %lld mini-batches of %lld bytes overflow int64", who,
               (long long)n_batches, (long long)pl.batch_bytes);
    *bytes_min = pl.batch_bytes;
    const bool lds = form == 1 || (form == 0 && nsu_fits(pl.nsu, nsu_device_lds_limit())); // forced forms ask no device
    *bytes = lds ? 0 : pl.batch_bytes * n_batches;
    return TG_OK;
}

extern "C" int tg_saint_rw_nodes(const tg_graph *csr, const int64_t *roots, int64_t n_batches, int64_t batch_size,
                                 int64_t walk_length, const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status,
                                 void *workspace, int64_t workspace_bytes, int32_t form, void *stream_) {
    using namespace tg;
    const char *who = "tg_saint_rw_nodes";
    TG_REQUIRE(csr && rng && out, "%s: null argument", who);
    TG_REQUIRE(csr->ptrs && (csr->indices || csr->n_edges == 0), "%s: null graph", who);
    TG_REQUIRE(csr->n_major >= 0 && csr->n_edges >= 0, "%s: negative graph size", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    SrwPlan pl;
    if (const int rc = srw_plan(batch_size, walk_length, who, pl)) return rc;
    if (csr->n_major > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: %lld vertices do not fit the 32-bit hash keys", who, (long long)csr->n_major);
    TG_REQUIRE(out->pitch_nodes >= pl.P, "%s: pitch_nodes = %lld below batch_size * (walk_length + 1) = %lld", who,
               (long long)out->pitch_nodes, (long long)pl.P);
    TG_REQUIRE(out->counts_stride >= 1, "%s: counts_stride = %lld, at least 1 expected", who, (long long)out->counts_stride);
    TG_REQUIRE(roots && out->nodes && out->counts && status, "%s: null roots / nodes / counts / status", who);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    const bool enough = workspace && workspace_bytes >= pl.batch_bytes;
    TG_REQUIRE(form != 2 || enough, "%s: workspace too small (%lld < %lld, the size of one mini-batch)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    if (n_batches == 0 || batch_size == 0) return TG_OK; // nothing to launch: no device is asked either
    const bool lds = form != 2 && nsu_fits(pl.nsu, nsu_device_lds_limit());
    TG_REQUIRE(form != 1 || lds, "%s: form 1: a table of %lld slots (%lld bytes of LDS) does not fit a workgroup", who,
               (long long)pl.nsu.table_cap, (long long)pl.nsu.lds_bytes);
    TG_REQUIRE(lds || enough, "%s: workspace too small (%lld < %lld, the size of one mini-batch)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    hipStream_t stream = (hipStream_t)stream_;

    const int64_t round = lds ? n_batches : std::min(std::min(workspace_bytes / pl.batch_bytes, NSU_ROUND_MAX), n_batches);
    for (int64_t b0 = 0; b0 < n_batches; b0 += round) {
        SrwArgs a{};
        a.g = CsrView{csr->ptrs, csr->indices, csr->ptrs32, csr->indices32, nullptr, 0};
        a.n_major = csr->n_major;
        a.roots = roots + b0 * batch_size;
        a.nodes = out->nodes + b0 * out->pitch_nodes, a.counts = out->counts + b0 * out->counts_stride;
        a.pitch = out->pitch_nodes, a.counts_stride = out->counts_stride;
        a.n_batches = std::min(round, n_batches - b0);
        a.B = batch_size, a.T = walk_length;
        a.seed = rng->seed, a.call_id = rng->call_id + (uint64_t)b0;
        a.status = status;
        saint_plan_args(pl, workspace, a);
        if (const int rc = lds ? srw_launch_lds(a, pl, stream) : srw_launch_flat(a, pl, stream)) return rc;
    }
    return TG_OK;
}

extern "C" int tg_saint_coverage_add(const int64_t *nodes, int64_t pitch_nodes, const int64_t *counts, int64_t counts_stride,
                                     int64_t n_batches, const int64_t *edge_ids, int64_t n_edge_ids, int64_t *node_count,
                                     int64_t n_nodes, int64_t *edge_count, int64_t n_edges, int32_t *status, void *stream_) {
    using namespace tg;
    const char *who = "tg_saint_coverage_add";
    TG_REQUIRE(n_batches >= 0 && n_edge_ids >= 0 && n_nodes >= 0 && n_edges >= 0 && pitch_nodes >= 0,
               "%s: negative size", who);
    TG_REQUIRE(counts_stride >= 1, "%s: counts_stride = %lld, at least 1 expected", who, (long long)counts_stride);
    TG_REQUIRE(status, "%s: null status", who);
    TG_REQUIRE(n_batches == 0 || (nodes && counts), "%s: null nodes / counts", who);
    TG_REQUIRE(n_edge_ids == 0 || edge_ids, "%s: null edge_ids", who);
    TG_REQUIRE((node_count || n_nodes == 0) && (edge_count || n_edges == 0), "%s: null count table", who);
    hipStream_t stream = (hipStream_t)stream_;
    if (n_batches > 0 && pitch_nodes > 0) {
        const unsigned gy = (unsigned)std::min<int64_t>(n_batches, 32768);
        hipLaunchKernelGGL(srw_cover_nodes_kernel, dim3(std::min(grid_1d(pitch_nodes), 256u), gy), dim3(256), 0, stream, nodes,
                           pitch_nodes, counts, counts_stride, n_batches, node_count, n_nodes, status);
        TG_LAUNCH_CHECK();
    }
    if (n_edge_ids > 0) {
        hipLaunchKernelGGL(srw_cover_edges_kernel, dim3(grid_1d(n_edge_ids)), dim3(256), 0, stream, edge_ids, n_edge_ids,
                           edge_count, n_edges, status);
        TG_LAUNCH_CHECK();
    }
    return TG_OK;
}

extern "C" int tg_saint_norm(const tg_graph *csc, const int64_t *node_count, const int64_t *edge_count, int64_t n_samples,
                             float *node_norm, float *edge_norm, void *stream_) {
    using namespace tg;
    const char *who = "tg_saint_norm";
    TG_REQUIRE(csc && csc->ptrs, "%s: null graph", who);
    TG_REQUIRE(csc->n_major >= 0 && csc->n_edges >= 0, "%s: negative graph size", who);
    TG_REQUIRE(n_samples >= 0, "%s: n_samples = %lld is negative", who, (long long)n_samples);
    TG_REQUIRE(csc->n_major == 0 || (node_count && node_norm), "%s: null node_count / node_norm", who);
    TG_REQUIRE(csc->n_edges == 0 || (node_count && edge_count && edge_norm), "%s: null edge_count / edge_norm", who);
    hipStream_t stream = (hipStream_t)stream_;
    if (csc->n_major > 0) {
        hipLaunchKernelGGL(srw_node_norm_kernel, dim3(grid_1d(csc->n_major)), dim3(256), 0, stream, node_count, csc->n_major,
                           (float)n_samples, node_norm);
        TG_LAUNCH_CHECK();
    }
    if (csc->n_edges > 0 && csc->n_major > 0) {
        const CsrView view{csc->ptrs, csc->indices, csc->ptrs32, csc->indices32, nullptr, 0};
        const int64_t n_chunks = (csc->n_edges + SRW_NORM_CHUNK - 1) / SRW_NORM_CHUNK;
        hipLaunchKernelGGL(srw_edge_norm_kernel, dim3(grid_1d(n_chunks * 64)), dim3(256), 0, stream, view, csc->n_major,
                           csc->n_edges, node_count, edge_count, edge_norm);
        TG_LAUNCH_CHECK();
    }
    return TG_OK;
}
