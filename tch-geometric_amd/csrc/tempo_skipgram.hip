// Temporal (CTDNE) skip-gram batches on gfx950: tg_tempo_skipgram (contract: include/tchgeo.h).
//
// What a temporal skip-gram trainer composes per mini-batch -- tempo_random_walk, strided slices + cat for the nodes and
// again for the timestamps, randint, slices + cat -- as one launch for G mini-batches.  The walk is tg_tempo_random_walk's
// (same step, same draws: tempo_walk.h), so it keeps a WAVEFRONT per walker: every step inspects a whole row.  What changes
// is where the row goes.  rw_tempo_kernel already holds a walker's [node | ts] row in LDS for its restarts; here a
// workgroup owns a tile of consecutive walkers of the launch (flat t = g * W + w), its wavefronts (one, unless tuned
// otherwise: see TSG_MAX_TILE) take them in turn, the rows stay in LDS at an odd pitch, and after a workgroup barrier the
// wavefronts stream the windows out through rw_skipgram.h's emit, window j of the tile being one run of tile * C * 8
// contiguous bytes per slab inside a mini-batch.
// The [n, L] walks are never written or read back.  The negatives are tg_rw_skipgram's element-wise kernel, a second
// launch on the same stream.
#include "rw_skipgram.h"
#include "tempo_walk.h"

#include <stdlib.h>

namespace tg {

// The workgroup: ONE wavefront that walks TSG_MAX_TILE walkers one after the other, then emits their windows.  Measured
// (profiles/bench_temporal_walk_loader_tiles.json: RMAT-24, 327 680 walkers of 20 columns per launch; the walk alone, as
// tg_tempo_random_walk, 47.6 ms): one wavefront with 1 / 2 / 4 / 8 / 16 / 32 walkers 40.3 / 38.8 / 39.3 / 40.8 / 40.1 / 56.2
// ms -- the walk bounds the launch and the shape of the stores (80-byte pieces to full lines) does not show; several
// wavefronts per workgroup wait at the barrier for the slowest walker (a hub row at every step): 4 wavefronts with 4 / 16
// walkers 82.8 / 55.3 ms, 2 with 2 / 8 / 16 55.4 / 46.7 / 43.8 ms.  Four walkers: within 2 % of the best, runs of 4 * C * 8
// bytes, and a small launch (one mini-batch) still spreads over the CUs.
constexpr int TSG_MAX_TILE = 4;                  // walkers per workgroup
constexpr int TSG_WAVES = 1;                     // wavefronts per workgroup
constexpr int64_t TSG_TILE_LDS = 16 * 1024;      // a tile of several walkers shrinks to this
constexpr int64_t TSG_LDS_LIMIT = 64 * 1024;     // one walker's rows beyond this: refused, as tg_tempo_random_walk does

struct TempoSkipgramParams {
    const int64_t *ptrs, *indices, *node_ts, *edge_ts;
    const int64_t *seeds, *seeds_ts; // [G, B]
    int64_t B, W, n_pos;             // seeds and walkers per mini-batch, G * W
    int64_t win0, win1;
    int32_t L, C, nw, pitch, tile;
    uint64_t seed, call_id;
    int64_t *pos, *pos_ts;           // pos_ts may be null
};

__global__ __launch_bounds__(256) void tsg_kernel(const TempoSkipgramParams p) {
    extern __shared__ __align__(16) unsigned char smem[];
    int64_t *base = reinterpret_cast<int64_t *>(smem); // [tile] element offset of the walker's window-0 row in a slab
    int64_t *rows = base + p.tile;                     // [tile][pitch]: L nodes, L timestamps
    // the wavefront's index as a scalar: what it derives per walker (t, g, w, the start time, the window) then sits in scalar
    // registers -- 61 vector registers instead of 111, 7 wavefronts per SIMD instead of 4
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;
    const int64_t L = p.L;
    const int64_t t0 = (int64_t)blockIdx.x * p.tile;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    for (int wl = wave; wl < p.tile; wl += n_waves) { // uniform per wavefront
        const int64_t t = t0 + wl;
        if (t >= p.n_pos) break;
        const int64_t gi = t / p.W, w = t - gi * p.W;
        int64_t *hist = rows + (int64_t)wl * p.pitch;
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW_TEMPO);
        const int64_t at = gi * p.B + w % p.B;
        int64_t cur = p.seeds[at];
        const int64_t it = p.seeds_ts[at];
        const int64_t wlo = it + p.win0, whi = it + p.win1; // half open, random_walk.rs:111
        if (lane == 0) {
            base[wl] = (gi * p.nw * p.W + w) * p.C;
            hist[0] = cur;
            hist[L] = it;
        }
        for (int64_t l = 0; l < L - 1; ++l) {
            const uint64_t step_id = (uint64_t)w * (uint64_t)L + (uint64_t)l;
            const TempoStep next = tempo_walk_step(p.ptrs, p.indices, p.node_ts, p.edge_ts, ck, step_id, cur, l, it, wlo, whi, hist,
                                                   L, lane, lt_mask);
            cur = next.node;
            if (lane == 0) {
                hist[l + 1] = next.node;
                hist[L + l + 1] = next.ts;
            }
        }
    }
    __syncthreads();
    const auto word = [](int64_t v, int) { return v; };
    rws_emit_windows(rows, base, p.pos, lane, p.tile, t0, p.n_pos, p.W, p.C, p.nw, p.pitch, wave, n_waves, word);
    if (p.pos_ts) rws_emit_windows(rows + L, base, p.pos_ts, lane, p.tile, t0, p.n_pos, p.W, p.C, p.nw, p.pitch, wave, n_waves, word);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct TsgPlan {
    RwsPlan rws;                 // L, nw, pitch (of the [node | ts] row)
    tg_rw_skipgram_config shape; // C, R, K, n_nodes for rw_skipgram.h's size checks
    int tile;                    // walkers per workgroup; 0: one walker's rows do not fit
    int waves;                   // wavefronts per workgroup (at most one per walker)
    int64_t lds;
};

static int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}

static int tsg_plan(const tg_tempo_skipgram_config *cfg, const char *who, TsgPlan &pl) {
    TG_REQUIRE(cfg, "%s: null config", who);
    const int64_t L = cfg->walk_length;
    TG_REQUIRE(L >= 1 && L < 0x3fffffff, "%s: walk_length = %lld outside [1, 2^30 - 1)", who, (long long)L);
    TG_REQUIRE(cfg->context_size >= 1 && cfg->context_size <= L, "%s: context_size = %lld outside [1, walk_length = %lld]", who,
               (long long)cfg->context_size, (long long)L);
    TG_REQUIRE(cfg->walks_per_node >= 1 && cfg->walks_per_node < RWS_MAX, "%s: walks_per_node = %lld, must be >= 1", who,
               (long long)cfg->walks_per_node);
    TG_REQUIRE(cfg->num_negative_samples >= 0 && cfg->num_negative_samples < RWS_MAX,
               "%s: num_negative_samples = %lld, must be >= 0", who, (long long)cfg->num_negative_samples);
    TG_REQUIRE(cfg->num_negative_samples == 0 || cfg->n_nodes >= 1, "%s: n_nodes = %lld, negatives need n_nodes >= 1", who,
               (long long)cfg->n_nodes);
    pl.rws.L = L;
    pl.rws.nw = L - cfg->context_size + 1;
    pl.rws.pitch = (2 * L) | 1;
    pl.rws.lds_u32 = pl.rws.lds_i64 = 0;
    pl.shape = tg_rw_skipgram_config{L - 1, cfg->context_size, cfg->walks_per_node, cfg->num_negative_samples, cfg->n_nodes, 1.0f,
                                     1.0f};
    const int forced = env_int("TG_TEMPO_SKIPGRAM_TILE", 0); // tuning knob: another largest tile (tools/bench_temporal_walk_loader.py)
    pl.tile = forced >= 1 && forced <= 64 ? forced : TSG_MAX_TILE;
    while (pl.tile > 1 && TG_TEMPO_SKIPGRAM_LDS_BYTES(L, pl.tile) > TSG_TILE_LDS) pl.tile >>= 1;
    pl.lds = TG_TEMPO_SKIPGRAM_LDS_BYTES(L, pl.tile);
    const int waves = env_int("TG_TEMPO_SKIPGRAM_WAVES", 0); // tuning knob: wavefronts per workgroup
    pl.waves = waves >= 1 && waves <= 4 ? waves : TSG_WAVES;
    if (pl.lds > TSG_LDS_LIMIT) pl.tile = 0;
    return TG_OK;
}

static int tsg_unsupported(const char *who, const TsgPlan &pl) {
    return fail(TG_ERR_UNSUPPORTED, "%s: walk_length %lld: one walker's rows (%lld bytes) exceed the LDS walk buffer", who,
                (long long)pl.rws.L, (long long)pl.lds);
}

} // namespace tg

extern "C" int tg_tempo_skipgram_capacity(const tg_tempo_skipgram_config *cfg, int64_t batch_size, int64_t *pos_rows,
                                          int64_t *neg_rows) {
    using namespace tg;
    const char *who = "tg_tempo_skipgram_capacity";
    TG_REQUIRE(pos_rows && neg_rows, "%s: null output", who);
    TsgPlan pl;
    if (const int rc = tsg_plan(cfg, who, pl)) return rc;
    int64_t W, U;
    if (const int rc = rws_sizes(&pl.shape, pl.rws, 1, batch_size, who, W, U)) return rc;
    *pos_rows = pl.rws.nw * W;
    *neg_rows = pl.rws.nw * U;
    return TG_OK;
}

extern "C" int tg_tempo_skipgram_lds_bytes(const tg_tempo_skipgram_config *cfg, int32_t *walkers_per_workgroup, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_tempo_skipgram_lds_bytes";
    TG_REQUIRE(walkers_per_workgroup && lds_bytes, "%s: null output", who);
    TsgPlan pl;
    if (const int rc = tsg_plan(cfg, who, pl)) return rc;
    if (pl.tile == 0) return tsg_unsupported(who, pl);
    *walkers_per_workgroup = pl.tile;
    *lds_bytes = pl.lds;
    return TG_OK;
}

extern "C" int tg_tempo_skipgram(const tg_graph *csr, const int64_t *node_ts, const int64_t *edge_ts, const int64_t *seeds,
                                 const int64_t *seeds_ts, int64_t n_batches, int64_t batch_size,
                                 const tg_tempo_skipgram_config *cfg, const tg_rng *rng, const tg_tempo_skipgram_out *out,
                                 void *stream_) {
    using namespace tg;
    const char *who = "tg_tempo_skipgram";
    TsgPlan pl;
    if (const int rc = tsg_plan(cfg, who, pl)) return rc;
    TG_REQUIRE(rng, "%s: null rng", who);
    int64_t W, U;
    const int64_t G = n_batches, B = batch_size;
    if (const int rc = rws_sizes(&pl.shape, pl.rws, G, B, who, W, U)) return rc;
    if (pl.tile == 0) return tsg_unsupported(who, pl);
    if (G == 0 || B == 0) return TG_OK;
    TG_REQUIRE(csr && csr->ptrs && (csr->indices || csr->n_edges == 0), "%s: null graph", who);
    TG_REQUIRE(node_ts && (edge_ts || csr->n_edges == 0) && seeds && seeds_ts && out && out->pos_rw && (out->neg_rw || U == 0),
               "%s: null buffers", who);
    const int64_t n_pos = G * W, blocks = (n_pos + pl.tile - 1) / pl.tile;
    TG_REQUIRE(blocks <= 0x7fffffff, "%s: %lld walkers are more than one launch takes", who, (long long)n_pos);
    hipStream_t stream = (hipStream_t)stream_;
    TempoSkipgramParams p;
    p.ptrs = csr->ptrs, p.indices = csr->indices, p.node_ts = node_ts, p.edge_ts = edge_ts;
    p.seeds = seeds, p.seeds_ts = seeds_ts;
    p.B = B, p.W = W, p.n_pos = n_pos, p.win0 = cfg->win0, p.win1 = cfg->win1;
    p.L = (int32_t)pl.rws.L, p.C = (int32_t)cfg->context_size, p.nw = (int32_t)pl.rws.nw, p.pitch = (int32_t)pl.rws.pitch;
    p.tile = pl.tile;
    p.seed = rng->seed, p.call_id = rng->call_id;
    p.pos = out->pos_rw, p.pos_ts = out->pos_ts;
    const int n_waves = pl.tile < pl.waves ? pl.tile : pl.waves;
    hipLaunchKernelGGL(tsg_kernel, dim3((unsigned)blocks), dim3(64 * n_waves), (size_t)pl.lds, stream, p);
    const int64_t neg_words = G * U * pl.rws.nw * p.C;
    if (neg_words > 0)
        hipLaunchKernelGGL(rws_negatives_kernel, dim3(grid_1d(neg_words)), dim3(256), 0, stream,
                           NegativeParams{seeds, out->neg_rw, B, U, p.C, p.nw, rng->seed, rng->call_id, (uint64_t)cfg->n_nodes},
                           neg_words);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
