// Random walks on gfx950 -- replace src/algo/random_walk.rs:10-158 (reference).
//
// rw_node2vec_kernel: one LANE per walker (1 M walkers x 80 dependent steps is
//   latency-bound; parallelism comes from walkers).  Per step: ptrs pair,
//   one random neighbour gather, optional has_edge binary search (only when
//   p,q make the three acceptance probabilities differ).  A walker's row is
//   staged 16 steps at a time in LDS and flushed by the whole wave so that each
//   walker's 128 contiguous bytes leave as one full line instead of 16 scattered
//   8-byte stores.  Algorithmic bytes per executed step: 16 + 8 read, 8 written.
//
// rw_tempo_kernel: one WAVEFRONT per walker.  Every step must inspect the whole
//   row (timestamps), so the wave streams indices/edge_ts coalesced, ranks the
//   admissible neighbours with ballot + popcount, and resolves the one-slot
//   reservoir (sampling.rs:17-22 with k = 1: candidate m >= 1 replaces with
//   probability 1/m, candidate 1 always does) from one addressed draw per
//   candidate.  HBM-bound on 16 B per inspected edge.
#include "rw_walk.h"
#include "tempo_walk.h"
#include "tg_device.h"
#include "tg_host.h"
#include "tg_map.h"

namespace tg {

constexpr int RW_STAGE = 16; // steps staged per walker between flushes

// CsrView, the edge-set probe, has_edge and the walk step: rw_walk.h (shared with rw_skipgram.hip)

__global__ void edge_set_clear_kernel(uint64_t *slots, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        slots[i] = EDGE_SET_EMPTY;
}
// the wavefronts walk the edge array in segments of 2 048 edges (coalesced); a segment's rows lie between the rows of its
// first and last edge, found once per segment, so an edge's row is a short search in cached offsets
constexpr int64_t EDGE_SET_SEGMENT = 2048;
__device__ __forceinline__ int64_t row_of_edge(const int64_t *__restrict__ ptrs, int64_t lo, int64_t hi, int64_t e) {
    while (lo < hi) { // last row r in [lo, hi] with ptrs[r] <= e
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (ptrs[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
__global__ void edge_set_insert_kernel(const int64_t *__restrict__ ptrs, const int64_t *__restrict__ indices, int64_t n_major,
                                       int64_t n_edges, uint64_t *slots, uint64_t mask) {
    const int lane = threadIdx.x & 63;
    const int64_t n_seg = (n_edges + EDGE_SET_SEGMENT - 1) / EDGE_SET_SEGMENT;
    for (int64_t sgm = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; sgm < n_seg;
         sgm += ((int64_t)gridDim.x * blockDim.x) >> 6) {
        const int64_t e0 = sgm * EDGE_SET_SEGMENT, e1 = min(n_edges, e0 + EDGE_SET_SEGMENT);
        const int64_t r0 = row_of_edge(ptrs, 0, n_major - 1, e0), r1 = row_of_edge(ptrs, r0, n_major - 1, e1 - 1);
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t r = row_of_edge(ptrs, r0, r1, e);
            const uint64_t key = ((uint64_t)r << 32) | (uint64_t)indices[e];
            for (uint64_t s = edge_key_hash(key) & mask;; s = (s + 1) & mask) {
                const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long *>(&slots[s]),
                                               (unsigned long long)EDGE_SET_EMPTY, (unsigned long long)key);
                if (old == EDGE_SET_EMPTY || old == key) break;
            }
        }
    }
}

// StageT = uint32_t for the has_edge variants when the vertex ids fit (0xffffffff stands for -1): half the LDS per
// workgroup, twice the resident wavefronts -- those variants are bound by the latency of their dependent loads (p != q:
// 11.8 -> 9.1 ms; p = q = 1 is not: 1.16 ms with int64 staging, 1.27 with u32, so it keeps int64)
template <typename StageT>
__global__ void rw_node2vec_kernel(const CsrView g, const int64_t *__restrict__ start, int64_t n, int64_t walk_length, float prob0,
                                   float prob1, float prob2, uint64_t seed, uint64_t call_id, int64_t *walks) {
    __shared__ StageT stage_all[4][64 * (RW_STAGE + 1)]; // [wave][walker * 17 + step]: odd pitch spreads LDS banks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    StageT *stage = stage_all[wave];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t wave_first = t - lane;
    const bool live = t < n;
    const CallKey ck = call_key(seed, call_id, TAG_RW);
    const int64_t L = walk_length + 1;
    const WalkProbs pr{prob0, prob1, prob2};
    const bool always_accept = pr.always_accept();

    int64_t prev = -1, cur = live ? start[t] : -1;
    bool dead = !live;
    // column 0 is the start node; columns 1..walk_length are steps 0..walk_length-1
    for (int64_t c0 = 0; c0 < L; c0 += RW_STAGE) {
        const int ncols = (int)min((int64_t)RW_STAGE, L - c0);
        for (int j = 0; j < ncols; ++j) {
            const int64_t col = c0 + j;
            int64_t val = -1;
            if (col == 0) {
                val = cur;
            } else if (!dead) {
                if (walk_step(g, ck, (uint64_t)t, (uint32_t)(col - 1), pr, always_accept, prev, cur))
                    val = cur;
                else
                    dead = true;
            }
            stage[lane * (RW_STAGE + 1) + j] = (StageT)val; // -1 -> all ones
        }
        wave_lds_handoff();
        // flush: walker w of this wave owns ncols contiguous int64 at walks[(wave_first+w)*L + c0 ..]
        const int total = 64 * ncols;
        for (int q = lane; q < total; q += 64) {
            const int w = q / ncols, j = q - w * ncols;
            const int64_t tw = wave_first + w;
            if (tw < n) {
                const StageT v = stage[w * (RW_STAGE + 1) + j];
                walks[tw * L + c0 + j] = v == (StageT)-1 ? (int64_t)-1 : (int64_t)v;
            }
        }
        wave_lds_handoff();
    }
}

// one wavefront per walker; LDS keeps the walk so far (node, ts) for restarts
__global__ void rw_tempo_kernel(const int64_t *__restrict__ ptrs, const int64_t *__restrict__ indices,
                                const int64_t *__restrict__ node_ts, const int64_t *__restrict__ edge_ts,
                                const int64_t *__restrict__ start, const int64_t *__restrict__ start_ts, int64_t n,
                                int64_t L, int64_t win0, int64_t win1, uint64_t seed, uint64_t call_id,
                                int64_t *walks, int64_t *walks_ts) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    int64_t *hist = reinterpret_cast<int64_t *>(smem) + (size_t)wave * 2 * L; // [L] nodes, [L] timestamps
    const int64_t i = (int64_t)blockIdx.x * n_waves + wave;
    if (i >= n) return;
    const CallKey ck = call_key(seed, call_id, TAG_RW_TEMPO);
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    int64_t cur = start[i];
    const int64_t it = start_ts[i];
    const int64_t wlo = it + win0, whi = it + win1; // half open, random_walk.rs:111
    if (lane == 0 && L > 0) {
        hist[0] = cur;
        hist[L] = it;
    }
    for (int64_t l = 0; l < L - 1; ++l) { // :117
        const uint64_t step_id = (uint64_t)i * (uint64_t)L + (uint64_t)l;
        const TempoStep next = tempo_walk_step(ptrs, indices, node_ts, edge_ts, ck, step_id, cur, l, it, wlo, whi, hist, L, lane,
                                               lt_mask); // tempo_walk.h
        cur = next.node; // :150-153
        if (lane == 0) {
            hist[l + 1] = next.node;
            hist[L + l + 1] = next.ts;
        }
    }
    wave_lds_handoff();
    for (int64_t c = lane; c < L; c += 64) {
        walks[i * L + c] = hist[c];
        walks_ts[i * L + c] = hist[L + c];
    }
}

} // namespace tg

extern "C" int tg_edge_set_bytes(const tg_graph *csr, int64_t *bytes) {
    TG_REQUIRE(csr && bytes && csr->n_edges >= 0 && csr->n_major >= 0, "tg_edge_set_bytes: bad arguments");
    TG_REQUIRE(csr->n_major < (int64_t)0xffffffff, "tg_edge_set_bytes: ids of %lld vertices do not fit the 32-bit halves of a key",
               (long long)csr->n_major);
    *bytes = 8 * edge_set_slots(csr->n_edges);
    return TG_OK;
}
extern "C" int tg_edge_set_build(const tg_graph *csr, void *edge_set, int64_t bytes, void *stream_) {
    TG_REQUIRE(csr && csr->ptrs && (csr->indices || csr->n_edges == 0) && edge_set, "tg_edge_set_build: null argument");
    TG_REQUIRE(csr->n_major < (int64_t)0xffffffff, "tg_edge_set_build: ids of %lld vertices do not fit a key", (long long)csr->n_major);
    const int64_t cap = edge_set_slots(csr->n_edges);
    TG_REQUIRE(bytes >= 8 * cap, "tg_edge_set_build: %lld bytes given, %lld needed", (long long)bytes, (long long)(8 * cap));
    hipStream_t stream = (hipStream_t)stream_;
    uint64_t *slots = reinterpret_cast<uint64_t *>(edge_set);
    hipLaunchKernelGGL(tg::edge_set_clear_kernel, dim3(tg::grid_1d(cap)), dim3(256), 0, stream, slots, cap);
    if (csr->n_edges > 0 && csr->n_major > 0) {
        const int64_t n_seg = (csr->n_edges + tg::EDGE_SET_SEGMENT - 1) / tg::EDGE_SET_SEGMENT;
        hipLaunchKernelGGL(tg::edge_set_insert_kernel, dim3(tg::grid_1d(n_seg * 64)), dim3(256), 0, stream, csr->ptrs, csr->indices,
                           csr->n_major, csr->n_edges, slots, (uint64_t)(cap - 1));
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_random_walk_es(const tg_graph *csr, const void *edge_set, int64_t edge_set_bytes, const int64_t *start, int64_t n,
                                 int64_t walk_length, float p, float q, const tg_rng *rng, int64_t *walks, void *stream) {
    TG_REQUIRE(csr && csr->ptrs && (csr->indices || csr->n_edges == 0), "tg_random_walk: null graph");
    TG_REQUIRE(rng && n >= 0 && walk_length >= 0, "tg_random_walk: bad arguments");
    TG_REQUIRE(p > 0.0f && q > 0.0f, "tg_random_walk: p and q must be positive (random_walk.rs:29-30)");
    uint64_t edge_mask = 0;
    if (edge_set) {
        const int64_t cap = edge_set_slots(csr->n_edges);
        TG_REQUIRE(edge_set_bytes == 8 * cap && csr->n_major < (int64_t)0xffffffff,
                   "tg_random_walk_es: the edge set (%lld bytes) was not built for this graph (%lld bytes)",
                   (long long)edge_set_bytes, (long long)(8 * cap));
        edge_mask = (uint64_t)(cap - 1);
    }
    if (n == 0) return TG_OK;
    TG_REQUIRE(start && walks, "tg_random_walk: null buffers");
    const tg::WalkProbs pr = walk_probs(p, q);
    const float prob0 = pr.prob0, prob1 = pr.prob1, prob2 = pr.prob2;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const tg::CsrView view{csr->ptrs, csr->indices, csr->ptrs32, csr->indices32, reinterpret_cast<const uint64_t *>(edge_set),
                           edge_mask};
    if (!pr.always_accept() && csr->n_major < (int64_t)0xffffffff)
        hipLaunchKernelGGL(tg::rw_node2vec_kernel<uint32_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, view, start, n,
                           walk_length, prob0, prob1, prob2, rng->seed, rng->call_id, walks);
    else
        hipLaunchKernelGGL(tg::rw_node2vec_kernel<int64_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, view, start, n,
                           walk_length, prob0, prob1, prob2, rng->seed, rng->call_id, walks);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
extern "C" int tg_random_walk(const tg_graph *csr, const int64_t *start, int64_t n, int64_t walk_length, float p, float q,
                              const tg_rng *rng, int64_t *walks, void *stream) {
    return tg_random_walk_es(csr, nullptr, 0, start, n, walk_length, p, q, rng, walks, stream);
}

extern "C" int tg_tempo_random_walk(const tg_graph *csr, const int64_t *node_ts, const int64_t *edge_ts,
                                    const int64_t *start, const int64_t *start_ts, int64_t n, int64_t walk_length,
                                    int64_t win0, int64_t win1, const tg_rng *rng, int64_t *walks, int64_t *walks_ts,
                                    void *stream) {
    TG_REQUIRE(csr && csr->ptrs && (csr->indices || csr->n_edges == 0), "tg_tempo_random_walk: null graph");
    TG_REQUIRE(rng && n >= 0 && walk_length >= 0, "tg_tempo_random_walk: bad arguments");
    if (n == 0 || walk_length == 0) return TG_OK;
    TG_REQUIRE(node_ts && (edge_ts || csr->n_edges == 0) && start && start_ts && walks && walks_ts,
               "tg_tempo_random_walk: null buffers");
    int n_waves = 4;
    while (n_waves > 1 && (size_t)n_waves * 2 * walk_length * sizeof(int64_t) > 48 * 1024) n_waves >>= 1;
    const size_t lds = (size_t)n_waves * 2 * walk_length * sizeof(int64_t);
    if (lds > 64 * 1024)
        return tg::fail(TG_ERR_UNSUPPORTED, "tg_tempo_random_walk: walk_length %lld exceeds the LDS walk buffer",
                        (long long)walk_length);
    const unsigned blocks = (unsigned)((n + n_waves - 1) / n_waves);
    hipLaunchKernelGGL(tg::rw_tempo_kernel, dim3(blocks), dim3(64 * n_waves), lds, (hipStream_t)stream, csr->ptrs,
                       csr->indices, node_ts, edge_ts, start, start_ts, n, walk_length, win0, win1, rng->seed,
                       rng->call_id, walks, walks_ts);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
