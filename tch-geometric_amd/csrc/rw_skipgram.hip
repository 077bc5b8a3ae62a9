// Node2Vec skip-gram batches on gfx950: tg_rw_skipgram (contract: include/tchgeo.h; DESIGN.md "Skip-gram batches").
//
// What a Node2Vec trainer composes per mini-batch -- random_walk, PyG's `cat([rw[:, j:j + C] for j in range(nw)])`,
// randint -- as ONE launch for G mini-batches.  The walk is tg_random_walk's (same step, same draws: rw_walk.h), so
// the kernel is latency-bound on dependent look-ups with one LANE per walker; what changes is where the row goes.
//
// LDS form (rws_lds_kernel): a workgroup is one wavefront, its 64 walkers' whole rows sit in LDS ([walker][column] at an
//   odd pitch: the 64 lanes of a column write hit 64 different banks), and after the walk the wave writes, window by window,
//   its walkers' C-wide rows: inside one mini-batch rows j*W + w .. j*W + w + 63 are 64*C*8 contiguous bytes, so every
//   store instruction covers 512 contiguous bytes.  A wave that straddles a mini-batch boundary (W no multiple of 64)
//   needs nothing special: every element takes its walker's own base offset from a 64-entry table in LDS.  The [n, L]
//   walks are never written or read back: bytes written = nw*C*8 per walker instead of L*8 + 2*nw*C*8 moved.
//   The negative walkers are waves of the same grid: their rows are addressed draws instead of look-ups.
// Flat form (any L): walks -> workspace [G*W, L] (rws_walk_kernel, 16 columns staged per flush as rw_node2vec_kernel),
//   then rws_windows_kernel streams the windows out and rws_negatives_kernel makes the negatives element-wise.
#include "rw_skipgram.h"

namespace tg {

struct SkipgramParams {
    CsrView g;
    const int64_t *seeds;  // [G, B]
    int64_t B, W, U;       // per mini-batch: seeds, positive walkers, negative walkers
    int64_t n_pos, n_neg;  // G * W, G * U
    int64_t pos_blocks;    // LDS form: the first pos_blocks wavefronts walk, the others draw negatives
    int32_t L, C, nw, pitch;
    WalkProbs pr;
    uint64_t seed, call_id, n_nodes;
    int64_t *pos, *neg;
    int64_t *walks;        // flat form: [G * W, L]
};

template <typename StageT> __global__ __launch_bounds__(64) void rws_lds_kernel(const SkipgramParams p) {
    extern __shared__ __align__(16) unsigned char smem[];
    int64_t *base = reinterpret_cast<int64_t *>(smem); // [64] element offset of walker's window-0 row in `out`
    StageT *stage = reinterpret_cast<StageT *>(smem + RWS_TABLE_BYTES);
    const int lane = threadIdx.x;
    const bool neg = (int64_t)blockIdx.x >= p.pos_blocks; // uniform
    const int64_t per = neg ? p.U : p.W, total = neg ? p.n_neg : p.n_pos;
    int64_t *__restrict__ out = neg ? p.neg : p.pos;
    const int64_t t0 = ((int64_t)blockIdx.x - (neg ? p.pos_blocks : 0)) * 64, t = t0 + lane;
    const bool live = t < total;
    const int64_t gi = live ? t / per : 0, w = live ? t - gi * per : 0;
    const int L = p.L, C = p.C;
    StageT *row = stage + lane * p.pitch;
    base[lane] = (gi * p.nw * per + w) * C;

    const int64_t first = live ? p.seeds[gi * p.B + w % p.B] : -1;
    row[0] = (StageT)first;
    if (!neg) {
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW);
        const bool always_accept = p.pr.always_accept();
        int64_t prev = -1, cur = first;
        bool dead = !live;
        for (int col = 1; col < L; ++col) { // column col is step col - 1
            int64_t val = -1;
            if (!dead) {
                if (walk_step(p.g, ck, (uint64_t)w, (uint32_t)(col - 1), p.pr, always_accept, prev, cur))
                    val = cur;
                else
                    dead = true;
            }
            row[col] = (StageT)val; // -1 -> all ones
        }
    } else {
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW_NEG);
        for (int m = 1; m < L; ++m) row[m] = live ? (StageT)negative_value(ck, (uint64_t)w, (uint32_t)m, p.n_nodes) : (StageT)-1;
    }
    wave_lds_handoff();
    rws_emit_windows(stage, base, out, lane, 64, t0, total, per, C, p.nw, p.pitch, 0, 1,
                     [](StageT v, int) { return v == (StageT)-1 ? (int64_t)-1 : (int64_t)v; });
}

// flat form, kernel 1: rw_node2vec_kernel with the mini-batch dimension; one wavefront per workgroup
__global__ __launch_bounds__(64) void rws_walk_kernel(const SkipgramParams p) {
    __shared__ int64_t stage[64 * (RWS_STAGE + 1)]; // [walker * 17 + step]: odd pitch spreads LDS banks
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * 64, t = t0 + lane;
    const bool live = t < p.n_pos;
    const int64_t gi = live ? t / p.W : 0, w = live ? t - gi * p.W : 0;
    const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW);
    const bool always_accept = p.pr.always_accept();
    const int64_t L = p.L;
    int64_t prev = -1, cur = live ? p.seeds[gi * p.B + w % p.B] : -1;
    bool dead = !live;
    for (int64_t c0 = 0; c0 < L; c0 += RWS_STAGE) {
        const int ncols = (int)min((int64_t)RWS_STAGE, L - c0);
        for (int j = 0; j < ncols; ++j) {
            const int64_t col = c0 + j;
            int64_t val = -1;
            if (col == 0) {
                val = cur;
            } else if (!dead) {
                if (walk_step(p.g, ck, (uint64_t)w, (uint32_t)(col - 1), p.pr, always_accept, prev, cur))
                    val = cur;
                else
                    dead = true;
            }
            stage[lane * (RWS_STAGE + 1) + j] = val;
        }
        wave_lds_handoff();
        const int n_el = 64 * ncols;
        for (int q = lane; q < n_el; q += 64) {
            const int wl = q / ncols, j = q - wl * ncols;
            if (t0 + wl < p.n_pos) p.walks[(t0 + wl) * L + c0 + j] = stage[wl * (RWS_STAGE + 1) + j];
        }
        wave_lds_handoff();
    }
}

// flat form, kernel 2: rws_windows_kernel (rw_skipgram.h)

// flat form, kernel 3: rws_negatives_kernel (rw_skipgram.h)

} // namespace tg

extern "C" int tg_rw_skipgram_capacity(const tg_rw_skipgram_config *cfg, int64_t batch_size, int64_t *pos_rows,
                                       int64_t *neg_rows) {
    using namespace tg;
    const char *who = "tg_rw_skipgram_capacity";
    TG_REQUIRE(pos_rows && neg_rows, "%s: null output", who);
    RwsPlan pl;
    if (const int rc = rws_plan(cfg, who, pl)) return rc;
    int64_t W, U;
    if (const int rc = rws_sizes(cfg, pl, 1, batch_size, who, W, U)) return rc;
    *pos_rows = pl.nw * W;
    *neg_rows = pl.nw * U;
    return TG_OK;
}

extern "C" int tg_rw_skipgram_form(const tg_rw_skipgram_config *cfg, int64_t id_bound, int64_t lds_limit_bytes, int32_t *form,
                                   int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_rw_skipgram_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    TG_REQUIRE(id_bound >= 0, "%s: id_bound = %lld", who, (long long)id_bound);
    RwsPlan pl;
    if (const int rc = rws_plan(cfg, who, pl)) return rc;
    *form = rws_auto_form(pl, id_bound, lds_limit_bytes > 0 ? lds_limit_bytes : RWS_LDS_LIMIT);
    *lds_bytes = id_bound < (int64_t)0xffffffff ? pl.lds_u32 : pl.lds_i64;
    return TG_OK;
}

extern "C" int tg_rw_skipgram_workspace_bytes(const tg_rw_skipgram_config *cfg, int64_t n_batches, int64_t batch_size,
                                              int64_t id_bound, int32_t form, int64_t *bytes) {
    using namespace tg;
    const char *who = "tg_rw_skipgram_workspace_bytes";
    TG_REQUIRE(bytes, "%s: null output", who);
    TG_REQUIRE(form >= 0 && form <= 3, "%s: form = %d outside [0, 3]", who, (int)form);
    TG_REQUIRE(id_bound >= 0, "%s: id_bound = %lld", who, (long long)id_bound);
    RwsPlan pl;
    if (const int rc = rws_plan(cfg, who, pl)) return rc;
    int64_t W, U;
    if (const int rc = rws_sizes(cfg, pl, n_batches, batch_size, who, W, U)) return rc;
    if (form == 0) form = rws_auto_form(pl, id_bound, RWS_LDS_LIMIT);
    *bytes = form == 3 ? n_batches * W * pl.L * 8 : 0;
    return TG_OK;
}

extern "C" int tg_rw_skipgram(const tg_graph *csr, const void *edge_set, int64_t edge_set_bytes, const int64_t *seeds,
                              int64_t n_batches, int64_t batch_size, const tg_rw_skipgram_config *cfg, const tg_rng *rng,
                              const tg_rw_skipgram_out *out, void *workspace, int64_t workspace_bytes, int32_t form,
                              void *stream_) {
    using namespace tg;
    const char *who = "tg_rw_skipgram";
    RwsPlan pl;
    if (const int rc = rws_plan(cfg, who, pl)) return rc;
    TG_REQUIRE(form >= 0 && form <= 3, "%s: form = %d outside [0, 3]", who, (int)form);
    TG_REQUIRE(rng, "%s: null rng", who);
    int64_t W, U;
    const int64_t G = n_batches, B = batch_size;
    if (const int rc = rws_sizes(cfg, pl, G, B, who, W, U)) return rc;
    if (G == 0 || B == 0) return TG_OK;
    TG_REQUIRE(csr && csr->ptrs && (csr->indices || csr->n_edges == 0), "%s: null graph", who);
    TG_REQUIRE(seeds && out && out->pos_rw && (out->neg_rw || U == 0), "%s: null buffers", who);
    uint64_t edge_mask = 0;
    if (edge_set) {
        const int64_t cap = edge_set_slots(csr->n_edges);
        TG_REQUIRE(edge_set_bytes == 8 * cap && csr->n_major < (int64_t)0xffffffff,
                   "%s: the edge set (%lld bytes) was not built for this graph (%lld bytes)", who, (long long)edge_set_bytes,
                   (long long)(8 * cap));
        edge_mask = (uint64_t)(cap - 1);
    }
    const int64_t id_bound = csr->n_major > cfg->n_nodes ? csr->n_major : cfg->n_nodes;
    if (form == 0) form = rws_auto_form(pl, id_bound, RWS_LDS_LIMIT);
    TG_REQUIRE(form != 1 || (id_bound < (int64_t)0xffffffff && pl.lds_u32 <= RWS_LDS_LIMIT),
               "%s: form 1: ids below %lld and rows of %lld columns (%lld bytes of LDS) do not fit the 32-bit LDS form", who,
               (long long)id_bound, (long long)pl.L, (long long)pl.lds_u32);
    TG_REQUIRE(form != 2 || pl.lds_i64 <= RWS_LDS_LIMIT, "%s: form 2: rows of %lld columns (%lld bytes of LDS) do not fit", who,
               (long long)pl.L, (long long)pl.lds_i64);
    const int64_t n_pos = G * W, n_neg = G * U;
    const int64_t pos_blocks = (n_pos + 63) / 64, neg_blocks = (n_neg + 63) / 64;
    TG_REQUIRE(pos_blocks + neg_blocks <= 0x7fffffff, "%s: %lld walkers are more than one launch takes", who,
               (long long)(n_pos + n_neg));
    if (form == 3) {
        const int64_t need = n_pos * pl.L * 8;
        TG_REQUIRE(workspace && workspace_bytes >= need, "%s: the flat form needs a workspace of %lld bytes, %lld given", who,
                   (long long)need, (long long)(workspace ? workspace_bytes : 0));
    }
    hipStream_t stream = (hipStream_t)stream_;
    SkipgramParams p;
    p.g = CsrView{csr->ptrs, csr->indices, csr->ptrs32, csr->indices32, reinterpret_cast<const uint64_t *>(edge_set), edge_mask};
    p.seeds = seeds;
    p.B = B, p.W = W, p.U = U, p.n_pos = n_pos, p.n_neg = n_neg, p.pos_blocks = pos_blocks;
    p.L = (int32_t)pl.L, p.C = (int32_t)cfg->context_size, p.nw = (int32_t)pl.nw, p.pitch = (int32_t)pl.pitch;
    p.pr = walk_probs(cfg->p, cfg->q);
    p.seed = rng->seed, p.call_id = rng->call_id, p.n_nodes = (uint64_t)cfg->n_nodes;
    p.pos = out->pos_rw, p.neg = out->neg_rw, p.walks = reinterpret_cast<int64_t *>(workspace);
    if (form == 1)
        hipLaunchKernelGGL(rws_lds_kernel<uint32_t>, dim3((unsigned)(pos_blocks + neg_blocks)), dim3(64), (size_t)pl.lds_u32,
                           stream, p);
    else if (form == 2)
        hipLaunchKernelGGL(rws_lds_kernel<int64_t>, dim3((unsigned)(pos_blocks + neg_blocks)), dim3(64), (size_t)pl.lds_i64,
                           stream, p);
    else {
        hipLaunchKernelGGL(rws_walk_kernel, dim3((unsigned)pos_blocks), dim3(64), 0, stream, p);
        const int64_t pos_words = n_pos * pl.nw * p.C, neg_words = n_neg * pl.nw * p.C;
        hipLaunchKernelGGL(rws_windows_kernel, dim3(grid_1d(pos_words)), dim3(256), 0, stream,
                           WindowParams{p.walks, p.pos, W, p.L, p.C, p.nw}, pos_words);
        if (neg_words > 0)
            hipLaunchKernelGGL(rws_negatives_kernel, dim3(grid_1d(neg_words)), dim3(256), 0, stream,
                               NegativeParams{seeds, p.neg, B, U, p.C, p.nw, p.seed, p.call_id, p.n_nodes}, neg_words);
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}
