// Common neighbours per link (tg_cn_links; the rule in include/tchgeo_cn.h): the intersection of two
// ascending rows, with no table, no atomics on the common path and no sort -- the output ascends by construction.
//   tile     a = the shorter row, b = the longer.  A tile is 64 consecutive entries of a, one per lane, loaded coalesced.  A
//            lane is LIVE if its entry differs from its predecessor (the lane below; for lane 0 the last entry of the tile
//            before) and passes the exclusion of the link's ends.
//   bracket  the part of b that can match the tile is [lower bound of the tile's first entry, upper bound of its last),
//            searched from the cursor the tile before left (its upper bound).  The search is 64-ary: every lane probes one
//            of 64 evenly spaced places and the popcount of a ballot narrows the range 64-fold per dependent load -- a hub
//            row of 2^20 entries is bracketed in four loads where a binary search takes twenty.  The popcount, not the
//            first set bit, picks the part, so a row that does not ascend still leaves the range inside the row.
//   window   a span of at most TG_CN_WINDOW entries is copied coalesced into the wave's own LDS window (u32 words) and every
//            live lane binary-searches it there: nine LDS probes.  A longer span (few matches inside a hub row) is searched
//            by each live lane in global memory between the span's ends.
//   output   matches are ballotted; the popcount below a lane is its place behind the running count; stores stop at cn_cap,
//            the count goes on.  A matching lane adds its table words to 64-bit accumulators of its own, reduced over the
//            wave once per link.  The adjacency bits are two more bracketed searches.
//   WAVE     one wavefront owns a link; a persistent grid of 256-thread workgroups whose four waves never meet a barrier.
//            Under AUTO a link whose shorter row exceeds wave_max is appended to a list (one atomic per such link).
//   GROUP    one workgroup owns a link, in rounds of TG_CN_GROUP_TILES tiles: wave w takes tiles w, w + 4, ... and leaves
//            each tile's ballot in LDS, a workgroup scan of the popcounts places every tile, and the second half of the
//            round loads the matching entries again (they are L2-hot) and stores them.  Tiles run out of order, so a tile
//            brackets b afresh from the round's cursor and reads its predecessor from memory.
// LDS: the windows are 4 x 512 x 4 B = 8 KiB per workgroup; the group kernel adds 2 KiB of ballots, 1 KiB of tile places and
// 160 B of totals: 11.2 KiB.  Neither bounds the residency of a 160 KiB CU: the registers do, at seven wavefronts per SIMD,
// which is seven workgroups per CU.
#include <algorithm>

#include "rw_walk.h"

#include "../../include/tchgeo_cn.h"

namespace tg {

constexpr int CN_THREADS = 256;
constexpr int CN_WAVES = CN_THREADS / 64;
constexpr int64_t CN_NO_LIMIT = INT64_MAX;

struct CnParams {
    CsrView g;
    int64_t n_major;
    const int64_t *src, *dst;
    const uint32_t *tables;
    int64_t id_bound, m;
    int64_t wave_max; // the wave kernel lists links whose shorter row is longer (CN_NO_LIMIT: none)
    int32_t cn_cap, n_tables, exclude_ends;
    int64_t *count, *cn, *adjacent;
    uint64_t *score;
    int32_t *status;
    uint32_t *counter, *list; // AUTO: the listed slots; null otherwise
};

__host__ __device__ inline int64_t cn_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// The first place p of [lo, hi) whose entry is >= key (UPPER: > key), hi where there is none.  Arguments and result are
// wave-uniform; every lane of the wave calls it.  Every probe lies inside [lo, hi) whatever the entries are.
template <bool UPPER> __device__ __forceinline__ int64_t cn_wave_bound(const CsrView &g, int64_t lo, int64_t hi, int64_t key) {
    const int lane = lane_id();
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) >> 6; // >= 2
        const int64_t q = lo + (int64_t)(lane + 1) * step - 1;
        bool before = false;
        if (q < hi) {
            const int64_t w = g.idx(q);
            before = UPPER ? w <= key : w < key;
        }
        const int64_t k = __popcll(__ballot(before)); // probes 0 .. k - 1 lie before the answer, probe k does not
        const int64_t part = lo + k * step;           // <= hi: only probes inside the range count
        hi = min(hi, part + step - 1);                // probe k's own place: the answer where nothing before it is
        lo = min(part, hi);
    }
    bool before = false;
    if (lo + lane < hi) {
        const int64_t w = g.idx(lo + lane);
        before = UPPER ? w <= key : w < key;
    }
    return lo + (int64_t)__popcll(__ballot(before));
}

// bit 0 of the adjacency word and its like: does `key` occur in the row [r0, r1)
__device__ __forceinline__ bool cn_row_has(const CsrView &g, int64_t r0, int64_t r1, int64_t key) {
    const int64_t p = cn_wave_bound<false>(g, r0, r1, key);
    return p < r1 && g.idx(p) == key;
}

// One tile: the n entries of a from place t against b from the cursor `cur` to b1.  -> the ballot of the lanes whose entry
// is a member of C; `x` is every lane's entry, `cur` moves to the upper bound of the tile's last entry.  A lane whose entry
// equals that last entry's successor in the next tile is no live lane there, so the next tile loses nothing to the cursor.
__device__ __forceinline__ uint64_t cn_tile(const CnParams &P, uint32_t *win, int64_t t, int n, bool has_prev, int64_t prev,
                                            int64_t u, int64_t v, int64_t b1, int64_t &cur, int64_t &x) {
    const int lane = lane_id();
    x = lane < n ? P.g.idx(t + lane) : 0;
    const int64_t below = __shfl_up(x, 1, 64);
    const bool run_start = lane == 0 ? (!has_prev || x != prev) : x != below;
    const bool live = lane < n && run_start && !(P.exclude_ends && (x == u || x == v));
    const int64_t first = __shfl(x, 0, 64), last = __shfl(x, n - 1, 64);
    const int64_t lo = cn_wave_bound<false>(P.g, cur, b1, first);
    const int64_t hi = cn_wave_bound<true>(P.g, lo, b1, last);
    cur = hi;
    const int64_t span = hi - lo;
    bool found = false;
    if (span > 0 && __ballot(live) != 0) { // wave-uniform
        if (span <= TG_CN_WINDOW) {
            wave_lds_handoff(); // the tile before has searched its window
            for (int64_t j = lane; j < span; j += 64) win[j] = (uint32_t)P.g.idx(lo + j);
            wave_lds_handoff();
            if (live) {
                const uint32_t key = (uint32_t)x;
                int l = 0, h = (int)span;
                while (l < h) {
                    const int mid = (l + h) >> 1;
                    if (win[mid] < key) l = mid + 1;
                    else h = mid;
                }
                found = l < (int)span && win[l] == key;
            }
        } else if (live) {
            int64_t l = lo, h = hi;
            while (l < h) {
                const int64_t mid = l + ((h - l) >> 1);
                if (P.g.idx(mid) < x) l = mid + 1;
                else h = mid;
            }
            found = l < hi && P.g.idx(l) == x;
        }
    }
    return __ballot(found);
}

// a matching lane's table words, into accumulators of its own
__device__ __forceinline__ void cn_add_scores(const CnParams &P, bool mine, int64_t x, uint64_t (&acc)[TG_CN_MAX_TABLES]) {
#pragma unroll
    for (int k = 0; k < TG_CN_MAX_TABLES; ++k)
        if (k < P.n_tables && mine) acc[k] += (uint64_t)P.tables[(int64_t)k * P.id_bound + x];
}

// a slot whose end lies outside the graph: never indexes ptrs
__device__ __forceinline__ void cn_refuse(const CnParams &P, int64_t i, int t) {
    if (t == 0) {
        P.count[i] = 0;
        if (P.adjacent) P.adjacent[i] = 0;
        atomicOr(P.status, TG_CN_STATUS_RANGE);
    }
    if (t < P.n_tables) P.score[i * P.n_tables + t] = 0;
}

struct CnRows {
    int64_t u0, u1, v0, v1; // the rows of u and of v
    int64_t a0, a1, b0, b1; // the shorter and the longer of them
};

__device__ __forceinline__ CnRows cn_rows(const CsrView &g, int64_t u, int64_t v) {
    CnRows r;
    r.u0 = g.ptr(u), r.u1 = max(r.u0, g.ptr(u + 1));
    r.v0 = g.ptr(v), r.v1 = max(r.v0, g.ptr(v + 1));
    const bool swap = r.v1 - r.v0 < r.u1 - r.u0;
    r.a0 = swap ? r.v0 : r.u0, r.a1 = swap ? r.v1 : r.u1;
    r.b0 = swap ? r.u0 : r.v0, r.b1 = swap ? r.u1 : r.v1;
    return r;
}

__global__ void cn_clear_kernel(uint32_t *counter) { *counter = 0; }

__global__ void __launch_bounds__(CN_THREADS) cn_wave_kernel(const CnParams P) {
    __shared__ uint32_t s_win[CN_WAVES][TG_CN_WINDOW];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t *win = s_win[wave];
    const int64_t n_waves = (int64_t)gridDim.x * CN_WAVES, cap = P.cn_cap;
    for (int64_t i = (int64_t)blockIdx.x * CN_WAVES + wave; i < P.m; i += n_waves) { // wave-uniform throughout
        const int64_t u = P.src[i], v = P.dst[i];
        if ((uint64_t)u >= (uint64_t)P.n_major || (uint64_t)v >= (uint64_t)P.n_major) {
            cn_refuse(P, i, lane);
            continue;
        }
        const CnRows r = cn_rows(P.g, u, v);
        if (r.a1 - r.a0 > P.wave_max) { // the group kernel's
            if (lane == 0) P.list[atomicAdd(P.counter, 1u)] = (uint32_t)i;
            continue;
        }
        if (P.adjacent) {
            const int64_t word = (cn_row_has(P.g, r.u0, r.u1, v) ? 1 : 0) | (cn_row_has(P.g, r.v0, r.v1, u) ? 2 : 0);
            if (lane == 0) P.adjacent[i] = word;
        }
        uint64_t acc[TG_CN_MAX_TABLES] = {0, 0, 0, 0};
        int64_t total = 0, cur = r.b0, prev = 0, x;
        bool has_prev = false;
        for (int64_t t = r.a0; t < r.a1 && cur < r.b1; t += 64) { // cur == b1: every entry of b lies before the tile
            const int n = (int)min((int64_t)64, r.a1 - t);
            const uint64_t mb = cn_tile(P, win, t, n, has_prev, prev, u, v, r.b1, cur, x);
            prev = __shfl(x, n - 1, 64);
            has_prev = true;
            if (mb == 0) continue;
            const bool mine = (mb >> lane) & 1;
            const int64_t at = total + (int64_t)__popcll(mb & ((1ull << lane) - 1ull));
            if (mine && at < cap) P.cn[i * cap + at] = x;
            cn_add_scores(P, mine, x, acc);
            total += (int64_t)__popcll(mb);
        }
#pragma unroll
        for (int k = 0; k < TG_CN_MAX_TABLES; ++k)
            if (k < P.n_tables) {
                const uint64_t sum = wave_sum<uint64_t>(acc[k]);
                if (lane == 0) P.score[i * P.n_tables + k] = sum;
            }
        if (lane == 0) {
            P.count[i] = total;
            if (total > cap) atomicOr(P.status, TG_CN_STATUS_CAP);
        }
    }
}

__global__ void __launch_bounds__(CN_THREADS) cn_group_kernel(const CnParams P) {
    __shared__ uint32_t s_win[CN_WAVES][TG_CN_WINDOW];
    __shared__ uint64_t s_ballot[TG_CN_GROUP_TILES];
    __shared__ uint32_t s_place[TG_CN_GROUP_TILES];
    __shared__ uint32_t s_wave_n[CN_WAVES];
    __shared__ uint64_t s_acc[CN_WAVES][TG_CN_MAX_TABLES];
    static_assert(TG_CN_GROUP_TILES == CN_THREADS, "the round's scan takes one tile per thread");
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    uint32_t *win = s_win[wave];
    const int64_t cap = P.cn_cap;
    // the wave kernel ran before on the stream: its counter is final
    const int64_t n_slots = P.list ? (int64_t)min((uint64_t)*P.counter, (uint64_t)P.m) : P.m;
    for (int64_t j = blockIdx.x; j < n_slots; j += gridDim.x) { // block-uniform: every thread meets every barrier
        const int64_t i = P.list ? (int64_t)P.list[j] : j;
        const int64_t u = P.src[i], v = P.dst[i];
        if ((uint64_t)u >= (uint64_t)P.n_major || (uint64_t)v >= (uint64_t)P.n_major) {
            cn_refuse(P, i, tid);
            continue;
        }
        const CnRows r = cn_rows(P.g, u, v);
        if (P.adjacent && wave == 0) {
            const int64_t word = (cn_row_has(P.g, r.u0, r.u1, v) ? 1 : 0) | (cn_row_has(P.g, r.v0, r.v1, u) ? 2 : 0);
            if (lane == 0) P.adjacent[i] = word;
        }
        uint64_t acc[TG_CN_MAX_TABLES] = {0, 0, 0, 0};
        int64_t base = 0, cur = r.b0, x;
        for (int64_t r0 = r.a0; r0 < r.a1; r0 += 64 * TG_CN_GROUP_TILES) {
            const int nt = (int)min((int64_t)TG_CN_GROUP_TILES, (r.a1 - r0 + 63) >> 6);
            cur = cn_wave_bound<false>(P.g, cur, r.b1, P.g.idx(r0)); // the round's cursor: every wave finds the same
            if (cur >= r.b1) break;                                  // every entry of b lies before the round
            for (int k = wave; k < nt; k += CN_WAVES) {
                const int64_t t = r0 + (int64_t)k * 64;
                const int n = (int)min((int64_t)64, r.a1 - t);
                const bool has_prev = t > r.a0;
                const int64_t prev = has_prev ? P.g.idx(t - 1) : 0;
                int64_t c = cur;
                const uint64_t mb = cn_tile(P, win, t, n, has_prev, prev, u, v, r.b1, c, x);
                if (lane == 0) s_ballot[k] = mb;
                cn_add_scores(P, (mb >> lane) & 1, x, acc);
            }
            __syncthreads();
            const uint32_t mine = tid < nt ? (uint32_t)__popcll(s_ballot[tid]) : 0u;
            const uint32_t incl = wave_inclusive_scan_u32_dpp(mine);
            if (lane == 63) s_wave_n[wave] = incl;
            __syncthreads();
            uint32_t before = 0, round_total = 0;
#pragma unroll
            for (int w = 0; w < CN_WAVES; ++w) {
                const uint32_t nw = s_wave_n[w];
                if (w < wave) before += nw;
                round_total += nw;
            }
            s_place[tid] = before + incl - mine;
            __syncthreads();
            if (base < cap)
                for (int k = wave; k < nt; k += CN_WAVES) {
                    const uint64_t mb = s_ballot[k];
                    const int64_t at = base + (int64_t)s_place[k] + (int64_t)__popcll(mb & ((1ull << lane) - 1ull));
                    if (((mb >> lane) & 1) && at < cap) P.cn[i * cap + at] = P.g.idx(r0 + (int64_t)k * 64 + lane);
                }
            base += round_total;
            __syncthreads(); // the round's words are read
        }
#pragma unroll
        for (int k = 0; k < TG_CN_MAX_TABLES; ++k)
            if (k < P.n_tables) {
                const uint64_t sum = wave_sum<uint64_t>(acc[k]);
                if (lane == 0) s_acc[wave][k] = sum;
            }
        __syncthreads();
        if (tid < P.n_tables) {
            uint64_t sum = 0;
            for (int w = 0; w < CN_WAVES; ++w) sum += s_acc[w][tid];
            P.score[i * P.n_tables + tid] = sum;
        }
        if (tid == 0) {
            P.count[i] = base;
            if (base > cap) atomicOr(P.status, TG_CN_STATUS_CAP);
        }
        __syncthreads(); // s_acc is read
    }
}

static int cn_plan(int64_t m, int32_t form, int64_t *bytes, const char *who) {
    TG_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "%s: m = %lld outside [0, 2^31)", who, (long long)m);
    TG_REQUIRE(form >= TG_CN_FORM_AUTO && form <= TG_CN_FORM_GROUP, "%s: unknown form %d", who, form);
    *bytes = form == TG_CN_FORM_WAVE ? 0 : cn_r256(256 + 4 * m);
    return TG_OK;
}

} // namespace tg

extern "C" int tg_cn_workspace_bytes(int64_t m, int32_t form, int64_t *bytes, int32_t *form_taken) {
    TG_REQUIRE(bytes, "tg_cn_workspace_bytes: null bytes");
    const int rc = tg::cn_plan(m, form, bytes, "tg_cn_workspace_bytes");
    if (rc != TG_OK) return rc;
    if (form_taken) *form_taken = form;
    return TG_OK;
}

extern "C" int tg_cn_links(const tg_graph *g, const tg_cn_in *in, const tg_cn_out *out, int64_t m, int32_t form,
                           int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_cn_links";
    TG_REQUIRE(g && in && out, "%s: null graph / in / out", who);
    int64_t need = 0;
    const int rc = cn_plan(m, form, &need, who);
    if (rc != TG_OK) return rc;
    TG_REQUIRE(in->cn_cap >= 1 && in->cn_cap <= TG_CN_MAX_CAP, "%s: cn_cap = %d outside [1, 2^20]", who, in->cn_cap);
    TG_REQUIRE(in->n_tables >= 0 && in->n_tables <= TG_CN_MAX_TABLES, "%s: n_tables = %d outside [0, %d]", who, in->n_tables,
               TG_CN_MAX_TABLES);
    TG_REQUIRE(in->n_tables == 0 || (in->tables && in->id_bound >= 1), "%s: %d tables need `tables` and id_bound >= 1", who,
               in->n_tables);
    TG_REQUIRE(in->exclude_ends == 0 || in->exclude_ends == 1, "%s: exclude_ends = %d is neither 0 nor 1", who,
               in->exclude_ends);
    TG_REQUIRE(in->wave_max >= 0, "%s: wave_max = %d is negative", who, in->wave_max);
    TG_REQUIRE(g->n_major >= 0 && g->n_edges >= 0, "%s: negative graph size", who);
    if (g->n_major > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: %lld vertices exceed the 2^31 this kernel takes", who, (long long)g->n_major);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    if (m == 0) return TG_OK; // nothing to launch
    TG_REQUIRE(g->ptrs && (g->indices || g->n_edges == 0), "%s: null graph arrays", who);
    TG_REQUIRE(in->src && in->dst && out->count && out->cn && status, "%s: null src / dst / count / cn / status", who);
    TG_REQUIRE(in->n_tables == 0 || out->score, "%s: null score with %d tables", who, in->n_tables);
    TG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: the workspace has %lld bytes, the call needs %lld", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(need == 0 || ((uintptr_t)workspace & 3u) == 0, "%s: the workspace must be 4-byte aligned", who);

    CnParams p;
    p.g = CsrView{g->ptrs, g->indices, g->ptrs32, g->indices32, nullptr, 0};
    p.n_major = g->n_major;
    p.src = in->src, p.dst = in->dst, p.tables = in->tables, p.id_bound = in->id_bound, p.m = m;
    p.wave_max = CN_NO_LIMIT;
    p.cn_cap = in->cn_cap, p.n_tables = in->n_tables, p.exclude_ends = in->exclude_ends;
    p.count = out->count, p.cn = out->cn, p.adjacent = out->adjacent, p.score = out->score;
    p.status = status;
    p.counter = p.list = nullptr;
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned wave_grid = (unsigned)std::min<int64_t>((m + CN_WAVES - 1) / CN_WAVES, TG_CN_WAVE_GROUPS);
    const unsigned group_grid = (unsigned)std::min<int64_t>(m, TG_CN_GROUP_GROUPS);
    if (form == TG_CN_FORM_AUTO) {
        p.counter = static_cast<uint32_t *>(workspace);
        p.list = p.counter + 64; // behind the counter's 256 bytes
        p.wave_max = in->wave_max > 0 ? in->wave_max : TG_CN_WAVE_MAX;
        hipLaunchKernelGGL(cn_clear_kernel, dim3(1), dim3(1), 0, stream, p.counter);
    }
    if (form != TG_CN_FORM_GROUP) hipLaunchKernelGGL(cn_wave_kernel, dim3(wave_grid), dim3(CN_THREADS), 0, stream, p);
    if (form != TG_CN_FORM_WAVE) hipLaunchKernelGGL(cn_group_kernel, dim3(group_grid), dim3(CN_THREADS), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
