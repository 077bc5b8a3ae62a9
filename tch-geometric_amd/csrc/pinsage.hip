// PinSAGE's importance sampler over a flat frontier (tg_pinsage_hop; semantics in include/tchgeo.h): the
// neighbours of a frontier vertex are the k vertices that R short random walks with termination from it visit most often,
// the visit counts are the weights.  DGL's RandomWalkNeighborSampler / PinSAGESampler.
//   select   a workgroup owns a TILE of S consecutive frontier slots.  Its threads take the tile's S * R walkers flat,
//            slot-major (a walk is T dependent random look-ups: throughput is the number of walkers in flight, and a
//            wavefront per vertex would idle 54 lanes at R = 10); walker (s, r) writes the vertex after step l as a u32 into
//            word l * R + r of slot s's row of LDS, 0xFFFFFFFF once the walk is over (ids are < 2^31).  The call keys of a
//            slot (tg_random_walk's for the steps, TG_TAG_PINSAGE's for the termination draws) are computed once per slot
//            into LDS.  Then every wavefront takes slots of the tile in turn: it sorts the row (P2 = the power of two >= V
//            = R * T words, at least 64; bitonic: the steps inside a 64-word chunk run in registers by lane exchanges, the
//            steps across chunks in LDS), reads it back 64 words at a time, finds every run's length from a max-scan of
//            the run heads, and offers each run at its LAST word -- where its count is final -- to the running top-64 of
//            ns_topk.h as RcEntry{key = (V - count) << 32 | id, pos = 0}: count descending, then id ascending, all keys
//            distinct.  A chunk none of whose runs beats the k-th kept entry costs one ballot.  The winners are parked in
//            the workspace at [slot * k + rank] as count << 32 | id.  The visits never reach global memory; no atomics but
//            the status word's: the hop is a pure function of its inputs.
//   scan     offsets = exclusive prefix of the counts (one workgroup, tg_scan.h), as tg_ns_hop_recent's
//   emit     lane per parked word: neighbour, parent and visit count go to their compact places
// The tile: S = 16 KiB / (4 * P2) slots, at most 16, at least 1; min(4, S) wavefronts.  With the 256 bytes of call keys a
// workgroup asks for at most 16.25 KiB of LDS -- nine fit a CU's 160 KiB at every size, so the wavefront slots and the
// registers bound the residency, and the launch never needs more than the default dynamic-LDS limit.  (Tiles of at most
// 64 / 32 / 16 slots at R = 10, T = 2 over 16 384 slots: 0.079 / 0.057 / 0.045 ms; the other shapes do not move.)
#include <algorithm>

#include "ns_topk.h"
#include "rw_walk.h"
#include "tg_scan.h"

namespace tg {

constexpr uint32_t PS_NONE = 0xFFFFFFFFu; // a word of a row nobody visited: sorts behind every id
constexpr int PS_MAX_VISITS = 4096;       // V = R * T at most
constexpr int PS_TILE_BYTES = 16384;      // rows of a tile
constexpr int PS_MAX_TILE = 16;           // slots of a tile at most: more, smaller workgroups walk a short frontier faster
constexpr int PS_KEY_WORDS = 4;           // per slot: the walk's call key, the termination draws' call key
constexpr int32_t PS_STATUS_RANGE = 2;    // status bit 1: a frontier vertex outside the graph

struct PinsageParams {
    CsrView g;
    int64_t n_major;
    const int64_t *vertices, *ids, *call_ids;
    int64_t m, id_base;
    int32_t k, R, T, V, P2, S;
    float alpha;
    uint32_t tag;
    uint64_t seed, call_id;
    int64_t *cnt, *offsets, *neighbors, *parents, *visits;
    int32_t *status;
    uint64_t *parked; // workspace [m * k]: count << 32 | id in rank order
};

__device__ __forceinline__ uint32_t ps_exchange(uint32_t x, int j, bool keep_min) {
    const uint32_t o = __shfl_xor(x, j, 64);
    return keep_min ? min(x, o) : max(x, o);
}

// the 64 words at row[c0 ..]: the bitonic steps j = 32 .. 1 of stage `size` in registers
__device__ __forceinline__ void ps_chunk_steps(uint32_t *row, int c0, int lane, bool up) {
    uint32_t x = row[c0 + lane];
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) x = ps_exchange(x, j, ((lane & j) == 0) == up);
    row[c0 + lane] = x;
}

// ascending bitonic sort of row[0 .. P2) by ONE wavefront (P2 a power of two >= 64)
__device__ __forceinline__ void ps_sort_row(uint32_t *row, int P2, int lane) {
    for (int c0 = 0; c0 < P2; c0 += 64) { // stages 2 .. 64: a lane touches its own word only
        uint32_t x = row[c0 + lane];
#pragma unroll
        for (int size = 2; size <= 64; size <<= 1) {
            const bool up = ((c0 + lane) & size) == 0;
#pragma unroll
            for (int j = size >> 1; j > 0; j >>= 1) x = ps_exchange(x, j, ((lane & j) == 0) == up);
        }
        row[c0 + lane] = x;
    }
    for (int size = 128; size <= P2; size <<= 1) {
        wave_lds_handoff();
        for (int j = size >> 1; j >= 64; j >>= 1) { // across chunks: the lanes take disjoint pairs
            for (int t = lane; t < (P2 >> 1); t += 64) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const bool up = (a & size) == 0;
                const uint32_t x = row[a], y = row[b];
                if ((x > y) == up) {
                    row[a] = y;
                    row[b] = x;
                }
            }
            wave_lds_handoff();
        }
        for (int c0 = 0; c0 < P2; c0 += 64) ps_chunk_steps(row, c0, lane, (c0 & size) == 0);
    }
    wave_lds_handoff();
}

// the sorted row -> the best min(k, distinct) runs, one per lane in rank order
__device__ __forceinline__ RcEntry ps_top_runs(const uint32_t *row, int P2, int V, int k, int lane) {
    RcEntry kept{RC_NO_KEY, RC_NO_POS};
    int carry = 0; // where the run that is open at the chunk's first word began
    for (int c0 = 0; c0 < P2; c0 += 64) {
        const int idx = c0 + lane;
        const uint32_t x = row[idx];
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)x) == PS_NONE) break; // sorted: nothing but empty words from here on
        const uint32_t before = idx > 0 ? row[idx - 1] : PS_NONE, after = idx + 1 < P2 ? row[idx + 1] : PS_NONE;
        const bool real = x != PS_NONE;
        const bool head = real && (idx == 0 || before != x), tail = real && after != x;
        int start = head ? idx : -1; // the last head at or before this lane
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(start, off, 64);
            if (lane >= off) start = max(start, u);
        }
        if (start < 0) start = carry;
        carry = __shfl(start, 63, 64);
        const int count = idx - start + 1; // final at the run's last word
        RcEntry c{((int64_t)(V - count) << 32) | (int64_t)x, 0u};
        const RcEntry kth = rc_shfl(kept, k - 1); // empty while fewer than k are kept
        const bool cand = tail && rc_before(c, kth);
        if (__ballot(cand) == 0) continue; // wave-uniform
        if (!cand) c = RcEntry{RC_NO_KEY, RC_NO_POS};
        c = rc_sort64(c, lane);
        kept = rc_merge_reversed(kept, rc_shfl(c, 63 - lane), lane);
    }
    return kept;
}

__global__ void __launch_bounds__(256) pinsage_select_kernel(const PinsageParams p) {
    extern __shared__ __align__(16) unsigned char ps_lds[];
    uint32_t *keys = reinterpret_cast<uint32_t *>(ps_lds); // [PS_MAX_TILE][PS_KEY_WORDS]
    uint32_t *rows = keys + PS_MAX_TILE * PS_KEY_WORDS;    // [S][P2]
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    const int S = p.S, R = p.R, T = p.T, V = p.V, P2 = p.P2, pad = P2 - V;
    const int64_t n_tiles = (p.m + S - 1) / S;
    const WalkProbs pr{1.0f, 1.0f, 1.0f}; // p = q = 1

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { // block-uniform: every thread meets every barrier
        const int64_t i0 = tile * S;
        for (int s = tid; s < S; s += nt) {
            const int64_t i = i0 + s;
            if (i >= p.m) continue;
            const uint64_t cid = p.call_ids ? (uint64_t)p.call_ids[i] : p.call_id;
            const CallKey cw = call_key(p.seed, cid, TAG_RW), ct = call_key(p.seed, cid, p.tag);
            keys[s * PS_KEY_WORDS + 0] = cw.k0;
            keys[s * PS_KEY_WORDS + 1] = cw.k1;
            keys[s * PS_KEY_WORDS + 2] = ct.k0;
            keys[s * PS_KEY_WORDS + 3] = ct.k1;
        }
        for (int q = tid; q < S * pad; q += nt) { // the words of a row past V
            const int s = q / pad;
            rows[s * P2 + V + (q - s * pad)] = PS_NONE;
        }
        __syncthreads();

        for (int j = tid; j < S * R; j += nt) { // the tile's walkers, slot-major
            const int s = j / R, r = j - s * R;
            uint32_t *row = rows + s * P2;
            const int64_t i = i0 + s;
            int64_t prev = -1, cur = i < p.m ? p.vertices[i] : -1;
            bool live = cur >= 0; // < 0: an empty slot
            if (live && cur >= p.n_major) { // never indexes ptrs
                live = false;
                if (r == 0) atomicOr(p.status, PS_STATUS_RANGE);
            }
            uint64_t w = 0;
            CallKey cw{0, 0}, ct{0, 0};
            if (live) {
                const uint64_t u = p.ids ? (uint64_t)p.ids[i] : (uint64_t)(p.id_base + i);
                w = u * (uint64_t)R + (uint64_t)r;
                cw = CallKey{keys[s * PS_KEY_WORDS + 0], keys[s * PS_KEY_WORDS + 1]};
                ct = CallKey{keys[s * PS_KEY_WORDS + 2], keys[s * PS_KEY_WORDS + 3]};
            }
            for (int l = 0; l < T; ++l) {
                if (live && l >= 1 && p.alpha > 0.0f) // alpha = 0 never ends a walk: the draw is not made
                    live = !(u32_to_f32_01(draw(ct, w, (uint32_t)l, 0u).w[0]) < p.alpha);
                if (live) live = walk_step(p.g, cw, w, (uint32_t)l, pr, true, prev, cur); // false: no out-edge
                row[l * R + r] = live ? (uint32_t)cur : PS_NONE;
            }
        }
        __syncthreads();

        for (int s = wave; s < S; s += n_waves) { // wave-uniform
            const int64_t i = i0 + s;
            if (i >= p.m) break;
            const int64_t v = p.vertices[i];
            if (v < 0 || v >= p.n_major) { // nothing was visited
                if (lane == 0) p.cnt[i] = 0;
                continue;
            }
            uint32_t *row = rows + s * P2;
            ps_sort_row(row, P2, lane);
            const RcEntry kept = ps_top_runs(row, P2, V, p.k, lane);
            const int n_kept = __popcll(__ballot(kept.pos != RC_NO_POS));
            const int cnt = n_kept < p.k ? n_kept : p.k;
            if (lane == 0) p.cnt[i] = cnt;
            if (lane < cnt) {
                const uint64_t count = (uint64_t)V - (uint64_t)(kept.key >> 32);
                p.parked[i * p.k + lane] = (count << 32) | (uint64_t)(uint32_t)kept.key; // until the offsets are known
            }
        }
        __syncthreads(); // the next tile writes the rows and the keys
    }
}

__global__ void __launch_bounds__(SCAN1_THREADS) pinsage_scan_kernel(const PinsageParams p) {
    block_scan_exclusive_plus1(p.m, [&](int64_t i) { return p.cnt[i]; }, p.offsets);
}

__global__ void __launch_bounds__(256) pinsage_emit_kernel(const PinsageParams p) {
    const int64_t n = p.m * p.k;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = j / p.k, r = j - v * p.k;
        if (r >= p.cnt[v]) continue;
        const uint64_t word = p.parked[j];
        const int64_t o = p.offsets[v] + r;
        p.neighbors[o] = (int64_t)(uint32_t)word;
        p.parents[o] = v;
        p.visits[o] = (int64_t)(word >> 32);
    }
}

} // namespace tg

extern "C" int tg_pinsage_hop_workspace_bytes(int64_t m, int32_t fanout, int64_t *bytes) {
    const char *who = "tg_pinsage_hop_workspace_bytes";
    TG_REQUIRE(bytes, "%s: null output", who);
    TG_REQUIRE(m >= 0, "%s: negative frontier size %lld", who, (long long)m);
    TG_REQUIRE(fanout >= 1 && fanout <= 64, "%s: fan-out %d outside 1..64", who, fanout);
    TG_REQUIRE(m <= INT64_MAX / (64 * 8), "%s: frontier too long", who);
    *bytes = m * fanout * 8;
    return TG_OK;
}

extern "C" int tg_pinsage_hop(const tg_graph *walk_graph, const tg_hop_in *in, const tg_pinsage_config *cfg, const tg_rng *rng,
                              const tg_hop_out *out, int64_t *visits, int32_t *status, void *workspace,
                              int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_pinsage_hop";
    TG_REQUIRE(walk_graph && in && cfg && rng && out, "%s: null argument", who);
    TG_REQUIRE(in->m >= 0, "%s: negative frontier size %lld", who, (long long)in->m);
    TG_REQUIRE(out->edge_ptrs == nullptr, "%s: out->edge_ptrs must be NULL (a sampled neighbour is not an edge of the graph)", who);
    TG_REQUIRE(cfg->n_walks >= 1, "%s: n_walks = %d, at least 1 expected", who, cfg->n_walks);
    TG_REQUIRE(cfg->walk_length >= 1, "%s: walk_length = %d, at least 1 expected", who, cfg->walk_length);
    TG_REQUIRE(in->fanout >= 1 && in->fanout <= 64, "%s: fan-out %d outside 1..64", who, in->fanout);
    TG_REQUIRE(cfg->termination >= 0.0f && cfg->termination < 1.0f, "%s: termination = %g outside [0, 1)", who,
               (double)cfg->termination); // a NaN fails both comparisons
    if ((int64_t)cfg->n_walks * cfg->walk_length > PS_MAX_VISITS)
        return fail(TG_ERR_UNSUPPORTED, "%s: n_walks * walk_length = %d * %d above %d visits per vertex", who, cfg->n_walks,
                    cfg->walk_length, PS_MAX_VISITS);
    if (walk_graph->n_major > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: %lld vertices do not fit the 32-bit visit words", who,
                    (long long)walk_graph->n_major);
    TG_REQUIRE(walk_graph->n_major >= 0 && walk_graph->n_edges >= 0, "%s: negative graph size", who);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    if (in->m == 0) return TG_OK; // nothing to launch
    TG_REQUIRE(walk_graph->ptrs && (walk_graph->indices || walk_graph->n_edges == 0), "%s: null graph", who);
    TG_REQUIRE(in->vertices && out->cnt && out->offsets && out->neighbors && out->parents && visits && status,
               "%s: null vertices / cnt / offsets / neighbors / parents / visits / status", who);
    int64_t need = 0;
    if (const int rc = tg_pinsage_hop_workspace_bytes(in->m, in->fanout, &need)) return rc;
    TG_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace missing or too small (%lld < %lld bytes)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: the workspace must be 8-byte aligned", who);

    PinsageParams p;
    p.g = CsrView{walk_graph->ptrs, walk_graph->indices, walk_graph->ptrs32, walk_graph->indices32, nullptr, 0};
    p.n_major = walk_graph->n_major;
    p.vertices = in->vertices, p.ids = in->ids, p.call_ids = in->call_ids;
    p.m = in->m, p.id_base = in->id_base;
    p.k = in->fanout, p.R = cfg->n_walks, p.T = cfg->walk_length, p.V = p.R * p.T;
    p.P2 = 64;
    while (p.P2 < p.V) p.P2 <<= 1;
    p.S = std::max(1, std::min(PS_MAX_TILE, PS_TILE_BYTES / (4 * p.P2)));
    p.alpha = cfg->termination;
    p.tag = in->rng_tag ? in->rng_tag : TG_TAG_PINSAGE;
    p.seed = rng->seed, p.call_id = rng->call_id;
    p.cnt = out->cnt, p.offsets = out->offsets, p.neighbors = out->neighbors, p.parents = out->parents, p.visits = visits;
    p.status = status;
    p.parked = static_cast<uint64_t *>(workspace);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n_tiles = (p.m + p.S - 1) / p.S;
    const size_t lds = (size_t)(PS_MAX_TILE * PS_KEY_WORDS + p.S * p.P2) * sizeof(uint32_t); // <= 16.25 KiB
    auto blocks = [](int64_t items, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min((items + 255) / 256, cap)); };
    hipLaunchKernelGGL(pinsage_select_kernel, dim3((unsigned)std::min<int64_t>(n_tiles, (int64_t)1 << 20)),
                       dim3(64 * std::min(4, p.S)), lds, stream, p);
    hipLaunchKernelGGL(pinsage_scan_kernel, dim3(1), dim3(SCAN1_THREADS), 0, stream, p);
    hipLaunchKernelGGL(pinsage_emit_kernel, dim3(blocks(p.m * p.k, 256 * 32)), dim3(256), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
