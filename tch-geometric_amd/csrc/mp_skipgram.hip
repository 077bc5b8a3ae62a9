// MetaPath2Vec skip-gram batches on gfx950: tg_mp_skipgram (contract: include/tchgeo.h; DESIGN.md "Skip-gram batches").
//
// tg_rw_skipgram on a typed graph: step l of a walk reads the CSR of relation metapath[l mod M], so the walk changes
// relation (and node type) every step.  All 64 lanes of a wavefront stand at the same column, so the step's relation is
// wave-uniform: the up to 16 CSR descriptors sit in the kernel arguments and are indexed by a loop counter, which brings
// them in through scalar registers; no lane branches on its relation.  The draws are tg_rw_skipgram's (TAG_RW with
// p = q = 1 for the walk, TAG_RW_NEG for the negatives, whose range is the node count of the column's type).
// Rows are staged as LOCAL ids (so the uint32 form needs only max(type_count) < 2^32 - 1); the column's type_start and
// pad_value are applied when a word is emitted, from a per-column table: in LDS for the LDS forms (L int64 behind the
// per-walker offsets), from the kernel arguments through a wave-uniform counter in the flat walk kernel.  The window emit
// and the flat window kernel are rw_skipgram.h's, shared with tg_rw_skipgram.
#include "rw_skipgram.h"

namespace tg {

struct MpParams {
    CsrView rel[TG_MP_MAX_STEPS];            // rel[m]: the CSR of metapath[m]
    // the column table: entry 0 is column 0 (type step_src[0]), entry k >= 1 the columns c with (c - 1) mod M == k - 1
    // (type step_dst[k - 1]); the step that fills such a column reads rel[k - 1]
    int64_t col_start[TG_MP_MAX_STEPS + 1];  // type_start of the entry's type
    uint64_t col_count[TG_MP_MAX_STEPS + 1]; // type_count of the entry's type
    const int64_t *seeds;                    // [G, B]
    int64_t B, W, U;                         // per mini-batch: seeds, positive walkers, negative walkers
    int64_t n_pos, n_neg;                    // G * W, G * U
    int64_t pos_blocks;                      // LDS form: the first pos_blocks wavefronts walk, the others draw negatives
    int32_t L, C, nw, pitch, M;
    uint64_t seed, call_id;
    int64_t pad;
    int64_t *pos, *neg;
    int64_t *walks;                          // flat form: [G * W, L], finished words
};

__device__ __forceinline__ int next_entry(int k, int M) { return k >= M ? 1 : k + 1; } // 0 -> 1 -> .. -> M -> 1

template <typename StageT> __global__ __launch_bounds__(64) void mps_lds_kernel(const MpParams p) {
    extern __shared__ __align__(16) unsigned char smem[];
    int64_t *base = reinterpret_cast<int64_t *>(smem);                      // [64] as rws_lds_kernel
    int64_t *col_off = reinterpret_cast<int64_t *>(smem + RWS_TABLE_BYTES); // [L] type_start of every column's type
    StageT *stage = reinterpret_cast<StageT *>(smem + RWS_TABLE_BYTES + 8 * (size_t)p.L);
    const int lane = threadIdx.x;
    const bool neg = (int64_t)blockIdx.x >= p.pos_blocks; // uniform
    const int64_t per = neg ? p.U : p.W, total = neg ? p.n_neg : p.n_pos;
    int64_t *__restrict__ out = neg ? p.neg : p.pos;
    const int64_t t0 = ((int64_t)blockIdx.x - (neg ? p.pos_blocks : 0)) * 64, t = t0 + lane;
    const bool live = t < total;
    const int64_t gi = live ? t / per : 0, w = live ? t - gi * per : 0;
    const int L = p.L, C = p.C, M = p.M;
    StageT *row = stage + lane * p.pitch;
    base[lane] = (gi * p.nw * per + w) * C;
    for (int c = lane; c < L; c += 64) col_off[c] = p.col_start[c == 0 ? 0 : (c - 1) % M + 1]; // once per wave and column

    const int64_t first = live ? p.seeds[gi * p.B + w % p.B] : -1;
    row[0] = (StageT)first;
    int k = 1; // the column table's entry of column `col`: wave-uniform
    if (!neg) {
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW);
        const WalkProbs pr{1.0f, 1.0f, 1.0f};
        int64_t prev = -1, cur = first;
        bool dead = !live;
        for (int col = 1; col < L; ++col, k = next_entry(k, M)) { // column col is step col - 1 over rel[k - 1]
            const CsrView g = p.rel[k - 1];
            int64_t val = -1;
            if (!dead) {
                if (walk_step(g, ck, (uint64_t)w, (uint32_t)(col - 1), pr, true, prev, cur))
                    val = cur;
                else
                    dead = true;
            }
            row[col] = (StageT)val; // -1 -> all ones
        }
    } else {
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW_NEG);
        for (int m = 1; m < L; ++m, k = next_entry(k, M)) {
            const uint64_t range = p.col_count[k];
            row[m] = live ? (StageT)negative_value(ck, (uint64_t)w, (uint32_t)m, range) : (StageT)-1;
        }
    }
    wave_lds_handoff();
    const int64_t pad = p.pad;
    rws_emit_windows(stage, base, out, lane, 64, t0, total, per, C, p.nw, p.pitch, 0, 1,
                     [=](StageT v, int col) { return v == (StageT)-1 ? pad : (int64_t)v + col_off[col]; });
}

// flat form, kernel 1: rws_walk_kernel over the metapath; the staged words are finished (start added, pad_value put in)
__global__ __launch_bounds__(64) void mps_walk_kernel(const MpParams p) {
    __shared__ int64_t stage[64 * (RWS_STAGE + 1)]; // [walker * 17 + step]: odd pitch spreads LDS banks
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * 64, t = t0 + lane;
    const bool live = t < p.n_pos;
    const int64_t gi = live ? t / p.W : 0, w = live ? t - gi * p.W : 0;
    const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW);
    const WalkProbs pr{1.0f, 1.0f, 1.0f};
    const int64_t L = p.L;
    const int M = p.M;
    int64_t prev = -1, cur = live ? p.seeds[gi * p.B + w % p.B] : -1;
    bool dead = !live;
    int k = 0; // the column table's entry of column `col`: wave-uniform
    for (int64_t c0 = 0; c0 < L; c0 += RWS_STAGE) {
        const int ncols = (int)min((int64_t)RWS_STAGE, L - c0);
        for (int j = 0; j < ncols; ++j, k = next_entry(k, M)) {
            const int64_t col = c0 + j;
            const CsrView g = p.rel[k == 0 ? 0 : k - 1];
            const int64_t start = p.col_start[k];
            int64_t val = p.pad;
            if (col == 0) {
                val = cur + start;
            } else if (!dead) {
                if (walk_step(g, ck, (uint64_t)w, (uint32_t)(col - 1), pr, true, prev, cur))
                    val = cur + start;
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

// flat form, kernel 3: neg[g][j * U + u][c] = x_u[j + c] + start of column j + c.  One lane per output ROW, so that a row's
// place in the column table is found once (one remainder per row) and stepped along its C words; a wavefront's 64 rows are
// consecutive in the slab and go out through the 16-column staging of the walk kernel: runs of 128 bytes per row, or one
// run of 64 * C * 8 bytes when C <= 16.  Here the table entry differs by lane (rows of several windows share a wave).
__global__ __launch_bounds__(64) void mps_negatives_kernel(const MpParams p, int64_t n_rows) {
    __shared__ int64_t stage[64 * (RWS_STAGE + 1)];
    const int lane = threadIdx.x;
    const int64_t per_batch = (int64_t)p.nw * p.U;
    const int M = p.M, C = p.C;
    for (int64_t i0 = (int64_t)blockIdx.x * 64; i0 < n_rows; i0 += (int64_t)gridDim.x * 64) { // uniform
        const int64_t i = i0 + lane;
        const bool live = i < n_rows;
        const int64_t gi = live ? i / per_batch : 0, r = live ? i - gi * per_batch : 0;
        const int64_t j = r / p.U, u = r - j * p.U;
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW_NEG);
        const int64_t seed0 = live ? p.seeds[gi * p.B + u % p.B] : 0;
        int k = j == 0 ? 0 : (int)((j - 1) % M) + 1;
        for (int c0 = 0; c0 < C; c0 += RWS_STAGE) {
            const int ncols = min(RWS_STAGE, C - c0);
            for (int jj = 0; jj < ncols; ++jj, k = next_entry(k, M)) {
                const int64_t m = j + c0 + jj;
                const int64_t x = m == 0 ? seed0 : negative_value(ck, (uint64_t)u, (uint32_t)m, p.col_count[k]);
                stage[lane * (RWS_STAGE + 1) + jj] = x + p.col_start[k];
            }
            wave_lds_handoff();
            const int n_el = 64 * ncols;
            for (int q = lane; q < n_el; q += 64) {
                const int wl = q / ncols, jj = q - wl * ncols;
                if (i0 + wl < n_rows) p.neg[(i0 + wl) * C + c0 + jj] = stage[wl * (RWS_STAGE + 1) + jj];
            }
            wave_lds_handoff();
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct MpsPlan {
    RwsPlan rws;
    tg_rw_skipgram_config shape; // T, C, R, K for rw_skipgram.h's checks
    int64_t id_bound;            // max(type_count): what a staged word must hold
    int64_t lds_u32, lds_i64;
};

static int mps_plan(const tg_mp_skipgram_config *cfg, const char *who, MpsPlan &pl) {
    TG_REQUIRE(cfg, "%s: null config", who);
    const int M = cfg->n_steps;
    TG_REQUIRE(M >= 1 && M <= TG_MP_MAX_STEPS, "%s: n_steps = %d outside [1, %d]", who, M, TG_MP_MAX_STEPS);
    TG_REQUIRE(cfg->n_types >= 1, "%s: n_types = %d, must be >= 1", who, (int)cfg->n_types);
    TG_REQUIRE(cfg->graphs && cfg->step_src && cfg->step_dst && cfg->type_count, "%s: null graphs, step_src, step_dst or type_count",
               who);
    pl.id_bound = 0;
    for (int t = 0; t < cfg->n_types; ++t) {
        TG_REQUIRE(cfg->type_count[t] >= 1, "%s: type_count[%d] = %lld, must be >= 1", who, t, (long long)cfg->type_count[t]);
        if (cfg->type_count[t] > pl.id_bound) pl.id_bound = cfg->type_count[t];
    }
    for (int m = 0; m < M; ++m) {
        const int s = cfg->step_src[m], d = cfg->step_dst[m];
        TG_REQUIRE(s >= 0 && s < cfg->n_types && d >= 0 && d < cfg->n_types, "%s: step %d: node type (%d -> %d) outside [0, %d)",
                   who, m, s, d, (int)cfg->n_types);
    }
    for (int m = 0; m + 1 < M; ++m)
        TG_REQUIRE(cfg->step_dst[m] == cfg->step_src[m + 1], "%s: step %d: broken chain, it ends at type %d and step %d starts at type %d",
                   who, m, (int)cfg->step_dst[m], m + 1, (int)cfg->step_src[m + 1]);
    pl.shape = tg_rw_skipgram_config{cfg->walk_length, cfg->context_size, cfg->walks_per_node, cfg->num_negative_samples, 1, 1.0f,
                                     1.0f};
    if (const int rc = rws_plan(&pl.shape, who, pl.rws)) return rc;
    TG_REQUIRE(cfg->walk_length <= M || cfg->step_dst[M - 1] == cfg->step_src[0],
               "%s: step %d: open path, it ends at type %d, not at type %d where step 0 starts, and walk_length = %lld > %d steps",
               who, M - 1, (int)cfg->step_dst[M - 1], (int)cfg->step_src[0], (long long)cfg->walk_length, M);
    for (int m = 0; m < M; ++m)
        TG_REQUIRE(cfg->graphs[m].n_major == cfg->type_count[cfg->step_src[m]],
                   "%s: step %d: the CSR has n_major = %lld rows, its source type %d has %lld nodes", who, m,
                   (long long)cfg->graphs[m].n_major, (int)cfg->step_src[m], (long long)cfg->type_count[cfg->step_src[m]]);
    pl.lds_u32 = TG_MP_SKIPGRAM_LDS_BYTES(pl.rws.L, 4);
    pl.lds_i64 = TG_MP_SKIPGRAM_LDS_BYTES(pl.rws.L, 8);
    return TG_OK;
}
static int mps_auto_form(const MpsPlan &pl, int64_t limit) {
    if (pl.id_bound < (int64_t)0xffffffff && pl.lds_u32 <= limit) return 1;
    if (pl.lds_i64 <= limit) return 2;
    return 3;
}

} // namespace tg

extern "C" int tg_mp_skipgram_capacity(const tg_mp_skipgram_config *cfg, int64_t batch_size, int64_t *pos_rows,
                                       int64_t *neg_rows) {
    using namespace tg;
    const char *who = "tg_mp_skipgram_capacity";
    TG_REQUIRE(pos_rows && neg_rows, "%s: null output", who);
    MpsPlan pl;
    if (const int rc = mps_plan(cfg, who, pl)) return rc;
    int64_t W, U;
    if (const int rc = rws_sizes(&pl.shape, pl.rws, 1, batch_size, who, W, U)) return rc;
    *pos_rows = pl.rws.nw * W;
    *neg_rows = pl.rws.nw * U;
    return TG_OK;
}

extern "C" int tg_mp_skipgram_form(const tg_mp_skipgram_config *cfg, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_mp_skipgram_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    MpsPlan pl;
    if (const int rc = mps_plan(cfg, who, pl)) return rc;
    *form = mps_auto_form(pl, lds_limit_bytes > 0 ? lds_limit_bytes : RWS_LDS_LIMIT);
    *lds_bytes = pl.id_bound < (int64_t)0xffffffff ? pl.lds_u32 : pl.lds_i64;
    return TG_OK;
}

extern "C" int tg_mp_skipgram_workspace_bytes(const tg_mp_skipgram_config *cfg, int64_t n_batches, int64_t batch_size,
                                              int32_t form, int64_t *bytes) {
    using namespace tg;
    const char *who = "tg_mp_skipgram_workspace_bytes";
    TG_REQUIRE(bytes, "%s: null output", who);
    TG_REQUIRE(form >= 0 && form <= 3, "%s: form = %d outside [0, 3]", who, (int)form);
    MpsPlan pl;
    if (const int rc = mps_plan(cfg, who, pl)) return rc;
    int64_t W, U;
    if (const int rc = rws_sizes(&pl.shape, pl.rws, n_batches, batch_size, who, W, U)) return rc;
    if (form == 0) form = mps_auto_form(pl, RWS_LDS_LIMIT);
    *bytes = form == 3 ? n_batches * W * pl.rws.L * 8 : 0;
    return TG_OK;
}

extern "C" int tg_mp_skipgram(const tg_mp_skipgram_config *cfg, const int64_t *seeds, int64_t n_batches, int64_t batch_size,
                              const tg_rng *rng, const tg_rw_skipgram_out *out, void *workspace, int64_t workspace_bytes,
                              int32_t form, void *stream_) {
    using namespace tg;
    const char *who = "tg_mp_skipgram";
    MpsPlan pl;
    if (const int rc = mps_plan(cfg, who, pl)) return rc;
    TG_REQUIRE(form >= 0 && form <= 3, "%s: form = %d outside [0, 3]", who, (int)form);
    TG_REQUIRE(rng, "%s: null rng", who);
    int64_t W, U;
    const int64_t G = n_batches, B = batch_size;
    if (const int rc = rws_sizes(&pl.shape, pl.rws, G, B, who, W, U)) return rc;
    if (G == 0 || B == 0) return TG_OK;
    const int M = cfg->n_steps;
    for (int m = 0; m < M; ++m)
        TG_REQUIRE(cfg->graphs[m].ptrs && (cfg->graphs[m].indices || cfg->graphs[m].n_edges == 0), "%s: step %d: null graph", who, m);
    TG_REQUIRE(seeds && out && out->pos_rw && (out->neg_rw || U == 0), "%s: null buffers", who);
    const int64_t L = pl.rws.L;
    if (form == 0) form = mps_auto_form(pl, RWS_LDS_LIMIT);
    TG_REQUIRE(form != 1 || (pl.id_bound < (int64_t)0xffffffff && pl.lds_u32 <= RWS_LDS_LIMIT),
               "%s: form 1: local ids below %lld and rows of %lld columns (%lld bytes of LDS) do not fit the 32-bit LDS form", who,
               (long long)pl.id_bound, (long long)L, (long long)pl.lds_u32);
    TG_REQUIRE(form != 2 || pl.lds_i64 <= RWS_LDS_LIMIT, "%s: form 2: rows of %lld columns (%lld bytes of LDS) do not fit", who,
               (long long)L, (long long)pl.lds_i64);
    const int64_t n_pos = G * W, n_neg = G * U;
    const int64_t pos_blocks = (n_pos + 63) / 64, neg_blocks = (n_neg + 63) / 64;
    TG_REQUIRE(pos_blocks + neg_blocks <= 0x7fffffff, "%s: %lld walkers are more than one launch takes", who,
               (long long)(n_pos + n_neg));
    if (form == 3) {
        const int64_t need = n_pos * L * 8;
        TG_REQUIRE(workspace && workspace_bytes >= need, "%s: the flat form needs a workspace of %lld bytes, %lld given", who,
                   (long long)need, (long long)(workspace ? workspace_bytes : 0));
    }
    hipStream_t stream = (hipStream_t)stream_;
    MpParams p = {};
    for (int m = 0; m < M; ++m) {
        const tg_graph &g = cfg->graphs[m];
        p.rel[m] = CsrView{g.ptrs, g.indices, g.ptrs32, g.indices32, nullptr, 0};
    }
    for (int k = 0; k <= M; ++k) {
        const int t = k == 0 ? cfg->step_src[0] : cfg->step_dst[k - 1];
        p.col_start[k] = cfg->type_start ? cfg->type_start[t] : 0;
        p.col_count[k] = (uint64_t)cfg->type_count[t];
    }
    p.seeds = seeds;
    p.B = B, p.W = W, p.U = U, p.n_pos = n_pos, p.n_neg = n_neg, p.pos_blocks = pos_blocks;
    p.L = (int32_t)L, p.C = (int32_t)cfg->context_size, p.nw = (int32_t)pl.rws.nw, p.pitch = (int32_t)pl.rws.pitch, p.M = M;
    p.seed = rng->seed, p.call_id = rng->call_id, p.pad = cfg->pad_value;
    p.pos = out->pos_rw, p.neg = out->neg_rw, p.walks = reinterpret_cast<int64_t *>(workspace);
    if (form == 1)
        hipLaunchKernelGGL(mps_lds_kernel<uint32_t>, dim3((unsigned)(pos_blocks + neg_blocks)), dim3(64), (size_t)pl.lds_u32,
                           stream, p);
    else if (form == 2)
        hipLaunchKernelGGL(mps_lds_kernel<int64_t>, dim3((unsigned)(pos_blocks + neg_blocks)), dim3(64), (size_t)pl.lds_i64,
                           stream, p);
    else {
        hipLaunchKernelGGL(mps_walk_kernel, dim3((unsigned)pos_blocks), dim3(64), 0, stream, p);
        const int64_t pos_words = n_pos * pl.rws.nw * p.C, neg_rows = n_neg * pl.rws.nw;
        hipLaunchKernelGGL(rws_windows_kernel, dim3(grid_1d(pos_words)), dim3(256), 0, stream,
                           WindowParams{p.walks, p.pos, W, p.L, p.C, p.nw}, pos_words);
        if (neg_rows > 0) hipLaunchKernelGGL(mps_negatives_kernel, dim3(grid_1d(neg_rows, 64)), dim3(64), 0, stream, p, neg_rows);
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}
