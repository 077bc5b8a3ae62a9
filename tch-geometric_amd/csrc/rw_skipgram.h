// What the skip-gram batch kernels share (rw_skipgram.hip: tg_rw_skipgram; mp_skipgram.hip: tg_mp_skipgram;
// tempo_skipgram.hip: tg_tempo_skipgram): the window emit of a wavefront over rows that sit in LDS, the flat form's window
// kernel, the negatives' draw and their element-wise kernel, and the host-side plan (shape checks, LDS bytes of the staged
// rows, walkers per mini-batch).
#pragma once
#include "rw_walk.h"
#include "tg_device.h"
#include "tg_host.h"
#include "tg_map.h"

namespace tg {

constexpr uint32_t TAG_RW_NEG = 12u;
constexpr int RWS_STAGE = 16;                   // flat form: columns staged per walker between flushes
constexpr int64_t RWS_LDS_LIMIT = 40 * 1024;    // LDS form: 4 workgroups (one wavefront each) stay resident per CU
constexpr int64_t RWS_TABLE_BYTES = 64 * 8;     // the wave's per-walker output offsets

__device__ __forceinline__ int64_t negative_value(CallKey ck, uint64_t u, uint32_t m, uint64_t n_nodes) {
    return (int64_t)bounded64(draw(ck, u, m, 0u).a(), n_nodes);
}

// The LDS forms' emit, by one wavefront.  stage: n_rows staged rows [walker][column] at `pitch`; base[wl]: element offset of
// walker wl's window-0 row in `out`; walkers t0 + wl < total are live.  Element q of a window's run is column q % C of
// walker q / C; lanes step by 64 elements without dividing.  The wave writes windows j0, j0 + j_step, ... (0, 1: all of
// them; a workgroup of several wavefronts that share the rows gives each its own j0).  Every element takes its walker's own
// base, so a run that crosses a mini-batch boundary splits there by itself.  word(v, col) turns the staged value of column
// col into the output word.
template <typename StageT, typename Word>
__device__ __forceinline__ void rws_emit_windows(const StageT *stage, const int64_t *base, int64_t *__restrict__ out, int lane,
                                                 int n_rows, int64_t t0, int64_t total, int64_t per, int C, int nw, int pitch,
                                                 int j0, int j_step, Word word) {
    const int n_el = n_rows * C, dw = 64 / C, dc = 64 % C;
    const int w_first = lane / C, c_first = lane - w_first * C;
    const int64_t win_stride = per * C;
    for (int j = j0; j < nw; j += j_step) {
        int wl = w_first, c = c_first;
        for (int q = lane; q < n_el; q += 64) {
            if (t0 + wl < total) out[base[wl] + j * win_stride + c] = word(stage[wl * pitch + j + c], j + c);
            c += dc;
            wl += dw;
            if (c >= C) {
                c -= C;
                ++wl;
            }
        }
    }
}

// flat form: pos[g][j * W + w][c] = walks[g * W + w][j + c], one output word per thread and round
struct WindowParams {
    const int64_t *walks; // [G * W, L]
    int64_t *pos;
    int64_t W;
    int32_t L, C, nw;
};
static __global__ void rws_windows_kernel(const WindowParams p, int64_t n_words) {
    const int64_t per_batch = (int64_t)p.nw * p.W * p.C, per_window = p.W * p.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gi = i / per_batch, r = i - gi * per_batch;
        const int64_t j = r / per_window, r2 = r - j * per_window;
        const int64_t w = r2 / p.C, c = r2 - w * p.C;
        p.pos[i] = p.walks[(gi * p.W + w) * p.L + j + c];
    }
}

// element-wise negatives: neg[g][j * U + u][c] = x_u[j + c], x_u[0] = the walker's seed, x_u[m] = negative_value(.., u, m, ..)
struct NegativeParams {
    const int64_t *seeds; // [G, B]
    int64_t *neg;
    int64_t B, U;
    int32_t C, nw;
    uint64_t seed, call_id, n_nodes;
};
static __global__ void rws_negatives_kernel(const NegativeParams p, int64_t n_words) {
    const int64_t per_batch = (int64_t)p.nw * p.U * p.C, per_window = p.U * p.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gi = i / per_batch, r = i - gi * per_batch;
        const int64_t j = r / per_window, r2 = r - j * per_window;
        const int64_t u = r2 / p.C, c = r2 - u * p.C;
        const int64_t m = j + c;
        p.neg[i] = m == 0 ? p.seeds[gi * p.B + u % p.B]
                          : negative_value(call_key(p.seed, p.call_id + (uint64_t)gi, TAG_RW_NEG), (uint64_t)u, (uint32_t)m, p.n_nodes);
    }
}

// ---- host side: the plan ------------------------------------------------------------------------------------------------
struct RwsPlan {
    int64_t L, nw, pitch;
    int64_t lds_u32, lds_i64;
};
constexpr int64_t RWS_MAX = (int64_t)1 << 40; // every product below stays far inside int64

static int rws_plan(const tg_rw_skipgram_config *cfg, const char *who, RwsPlan &pl) {
    TG_REQUIRE(cfg, "%s: null config", who);
    TG_REQUIRE(cfg->walk_length >= 1 && cfg->walk_length < 0x7fffffff, "%s: walk_length = %lld outside [1, 2^31 - 1)", who,
               (long long)cfg->walk_length);
    pl.L = cfg->walk_length + 1;
    TG_REQUIRE(cfg->context_size >= 1 && cfg->context_size <= pl.L, "%s: context_size = %lld outside [1, walk_length + 1 = %lld]",
               who, (long long)cfg->context_size, (long long)pl.L);
    TG_REQUIRE(cfg->walks_per_node >= 1 && cfg->walks_per_node < RWS_MAX, "%s: walks_per_node = %lld, must be >= 1", who,
               (long long)cfg->walks_per_node);
    TG_REQUIRE(cfg->num_negative_samples >= 0 && cfg->num_negative_samples < RWS_MAX,
               "%s: num_negative_samples = %lld, must be >= 0", who, (long long)cfg->num_negative_samples);
    TG_REQUIRE(cfg->num_negative_samples == 0 || cfg->n_nodes >= 1, "%s: n_nodes = %lld, negatives need n_nodes >= 1", who,
               (long long)cfg->n_nodes);
    TG_REQUIRE(cfg->p > 0.0f && cfg->q > 0.0f, "%s: p and q must be positive (random_walk.rs:29-30)", who);
    pl.nw = pl.L - cfg->context_size + 1;
    pl.pitch = pl.L | 1;
    pl.lds_u32 = 64 * pl.pitch * 4 + RWS_TABLE_BYTES;
    pl.lds_i64 = 64 * pl.pitch * 8 + RWS_TABLE_BYTES;
    return TG_OK;
}
static int rws_auto_form(const RwsPlan &pl, int64_t id_bound, int64_t limit) {
    if (id_bound < (int64_t)0xffffffff && pl.lds_u32 <= limit) return 1;
    if (pl.lds_i64 <= limit) return 2;
    return 3;
}
// per mini-batch walkers and the launch's totals; refuses sizes whose products would leave int64 or the grid
static int rws_sizes(const tg_rw_skipgram_config *cfg, const RwsPlan &pl, int64_t G, int64_t B, const char *who, int64_t &W,
                     int64_t &U) {
    TG_REQUIRE(G >= 0 && B >= 0 && G < RWS_MAX && B < RWS_MAX, "%s: n_batches = %lld, batch_size = %lld: bad sizes", who,
               (long long)G, (long long)B);
    const __int128 w = (__int128)cfg->walks_per_node * B, u = w * cfg->num_negative_samples;
    const __int128 widest = (__int128)pl.nw * cfg->context_size > pl.L ? (__int128)pl.nw * cfg->context_size : (__int128)pl.L;
    const __int128 words = (w + u) * (G > 0 ? G : 1) * widest; // >= every slab's words
    TG_REQUIRE(words < ((__int128)1 << 59), "%s: a launch of %lld x %lld seeds is too large", who, (long long)G, (long long)B);
    W = (int64_t)w;
    U = (int64_t)u;
    return TG_OK;
}

} // namespace tg
