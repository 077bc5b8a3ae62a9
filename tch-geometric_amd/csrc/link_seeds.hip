// Link-level seed rows on gfx950: tg_link_seeds (contract: include/tchgeo.h; DESIGN.md 4.14 "Link seeds") and its typed
// twin for one relation of a typed graph, tg_link_seeds_typed.
//
// What a link-prediction trainer composes per mini-batch -- randint negatives, cat with the positive edges -- as ONE launch
// for G mini-batches, with the negatives CHECKED against the graph (negative_sampling.rs rejects has_edge(v, w) and
// v == w) and addressed, so a row is a function of (seed, call id) alone.
//
// One flat grid.  Its first blocks own the negatives, a LANE per negative: t = g * N + u (N = K * E per mini-batch), so a
// wavefront that straddles a mini-batch boundary needs nothing special.  A lane runs at most try_count dependent rounds;
// a round is a Philox block (ALU) and a look-up -- two offset loads and a binary search of column d, or one probe of the
// edge set -- so the kernel is latency-bound and wants many resident wavefronts, not wide ones: 256 threads, no LDS.
// The draw of attempt a + 1 does not depend on look-up a: it is computed in the block that issues look-up a's first loads.
// The remaining blocks copy the positives, one 8-byte word per lane, coalesced on both sides.
// `unverified` is zeroed by a memset node ahead of the kernel; a wavefront adds its exhausted lanes with one atomic per
// mini-batch it touches (ballot + popcount).
#include "rw_walk.h"
#include "tg_device.h"
#include "tg_host.h"

namespace tg {

constexpr uint32_t TAG_LINK_NEG = 13u;
constexpr int LINK_THREADS = 256;

struct LinkSeedsParams {
    CsrView g;
    const int64_t *src, *dst; // [G, E]
    int64_t E, K, N, S, P;    // per mini-batch: positives, negatives per positive, negatives, row words, pairs
    int64_t n_neg, n_copy;    // G * N negative lanes, G * 2 E copied words
    int64_t neg_blocks;       // the first neg_blocks workgroups draw, the others copy
    int32_t mode, try_count;
    uint64_t seed, call_id, n_nodes;
    int64_t *seeds;                 // [G, S]
    unsigned long long *unverified; // [G] or null
};

__global__ __launch_bounds__(LINK_THREADS) void link_seeds_kernel(const LinkSeedsParams p) {
    const bool triplet = p.mode == TG_LINK_TRIPLET; // uniform
    if ((int64_t)blockIdx.x >= p.neg_blocks) {      // uniform: the positives, word by word
        const int64_t t = ((int64_t)blockIdx.x - p.neg_blocks) * LINK_THREADS + threadIdx.x;
        if (t >= p.n_copy) return;
        const int64_t gi = t / (2 * p.E), r = t - gi * 2 * p.E;
        const bool second = r >= p.E;
        const int64_t i = second ? r - p.E : r;
        const int64_t v = (second ? p.dst : p.src)[gi * p.E + i];
        // binary: [src_pos | src_neg | dst_pos | dst_neg] -> the halves start at 0 and P; triplet: [src | dst_pos | ...]
        p.seeds[gi * p.S + (second ? (triplet ? p.E : p.P) : 0) + i] = v;
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * LINK_THREADS + threadIdx.x;
    const bool live = t < p.n_neg;
    const int64_t gi = live ? t / p.N : 0, u = live ? t - gi * p.N : 0;
    bool exhausted = false;
    if (live) {
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_LINK_NEG);
        const int64_t anchor = triplet ? p.src[gi * p.E + u / p.K] : 0; // triplet: the positive's source
        const int tries = p.try_count;
        Draw cur = draw(ck, (uint64_t)u, 0u, 0u);
        int64_t s, d;
        for (int a = 0;; ++a) {
            if (triplet) {
                s = anchor;
                d = (int64_t)bounded64(cur.a(), p.n_nodes);
            } else {
                s = (int64_t)bounded64(cur.a(), p.n_nodes);
                d = (int64_t)bounded64(cur.b(), p.n_nodes);
            }
            if (tries == 1) break; // PyG's unchecked negatives: no look-up at all
            const bool last = a + 1 >= tries;
            Draw nxt = cur;
            if (!last) nxt = draw(ck, (uint64_t)u, (uint32_t)(a + 1), 0u); // independent of the look-up below
            if (s != d && !has_edge(p.g, d, s)) break;                     // edge(s -> d): s in column d of the CSC
            if (last) {
                exhausted = true;
                break;
            }
            cur = nxt;
        }
        int64_t *row = p.seeds + gi * p.S;
        if (triplet) {
            row[2 * p.E + u] = d;
        } else {
            row[p.E + u] = s;
            row[p.P + p.E + u] = d;
        }
    }
    if (p.unverified == nullptr || p.try_count == 1) return; // uniform
    const int lane = lane_id();
    uint64_t pending = __ballot(exhausted);
    while (pending) { // uniform: one atomic per mini-batch with exhausted lanes in this wavefront
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int64_t gl = __shfl(gi, leader, 64);
        const uint64_t same = __ballot(exhausted && gi == gl);
        if (lane == leader) atomicAdd(p.unverified + gl, (unsigned long long)__popcll(same));
        pending &= ~same;
    }
}

// ---- the typed twin: one relation (A, rel, B), two id ranges, two output rows per mini-batch --------------------------
// The same grid, the same draws and the same look-ups as above.  What differs: s is bounded by n_src and d by n_dst,
// `s == d` is rejected only when both endpoints are ONE node type (equal ids of two types are unrelated nodes), and a
// mini-batch writes a source row [src_pos | src_neg] (triplet: [src]) and a destination row [dst_pos | dst_neg], each with
// its own base and pitch.  src_out = base, dst_out = base + Ws, both pitches S is tg_link_seeds' row.
struct LinkSeedsTypedParams {
    CsrView g;
    const int64_t *src, *dst; // [G, E]
    int64_t E, K, N;          // per mini-batch: positives, negatives per positive, negatives
    int64_t n_neg, n_copy;    // G * N negative lanes, G * 2 E copied words
    int64_t neg_blocks;       // the first neg_blocks workgroups draw, the others copy
    int32_t mode, try_count, same_type;
    uint64_t seed, call_id, n_src, n_dst;
    int64_t *src_out, *dst_out; // rows of Ws and Wd words at these pitches
    int64_t src_pitch, dst_pitch;
    unsigned long long *unverified; // [G] or null
};

__global__ __launch_bounds__(LINK_THREADS) void link_seeds_typed_kernel(const LinkSeedsTypedParams p) {
    const bool triplet = p.mode == TG_LINK_TRIPLET; // uniform
    if ((int64_t)blockIdx.x >= p.neg_blocks) {      // uniform: the positives lead both rows, word by word
        const int64_t t = ((int64_t)blockIdx.x - p.neg_blocks) * LINK_THREADS + threadIdx.x;
        if (t >= p.n_copy) return;
        const int64_t gi = t / (2 * p.E), r = t - gi * 2 * p.E;
        if (r >= p.E)
            p.dst_out[gi * p.dst_pitch + (r - p.E)] = p.dst[gi * p.E + (r - p.E)];
        else
            p.src_out[gi * p.src_pitch + r] = p.src[gi * p.E + r];
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * LINK_THREADS + threadIdx.x;
    const bool live = t < p.n_neg;
    const int64_t gi = live ? t / p.N : 0, u = live ? t - gi * p.N : 0;
    bool exhausted = false;
    if (live) {
        const CallKey ck = call_key(p.seed, p.call_id + (uint64_t)gi, TAG_LINK_NEG);
        const int64_t anchor = triplet ? p.src[gi * p.E + u / p.K] : 0; // triplet: the positive's source
        const int tries = p.try_count;
        const bool same = p.same_type != 0; // uniform
        Draw cur = draw(ck, (uint64_t)u, 0u, 0u);
        int64_t s, d;
        for (int a = 0;; ++a) {
            if (triplet) {
                s = anchor;
                d = (int64_t)bounded64(cur.a(), p.n_dst);
            } else {
                s = (int64_t)bounded64(cur.a(), p.n_src);
                d = (int64_t)bounded64(cur.b(), p.n_dst);
            }
            if (tries == 1) break; // PyG's unchecked negatives: no look-up at all
            const bool last = a + 1 >= tries;
            Draw nxt = cur;
            if (!last) nxt = draw(ck, (uint64_t)u, (uint32_t)(a + 1), 0u); // independent of the look-up below
            if (!(same && s == d) && !has_edge(p.g, d, s)) break;          // edge(s -> d): s in column d of the CSC
            if (last) {
                exhausted = true;
                break;
            }
            cur = nxt;
        }
        if (!triplet) p.src_out[gi * p.src_pitch + p.E + u] = s;
        p.dst_out[gi * p.dst_pitch + p.E + u] = d;
    }
    if (p.unverified == nullptr || p.try_count == 1) return; // uniform
    const int lane = lane_id();
    uint64_t pending = __ballot(exhausted);
    while (pending) { // uniform: one atomic per mini-batch with exhausted lanes in this wavefront
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int64_t gl = __shfl(gi, leader, 64);
        const uint64_t same_g = __ballot(exhausted && gi == gl);
        if (lane == leader) atomicAdd(p.unverified + gl, (unsigned long long)__popcll(same_g));
        pending &= ~same_g;
    }
}

constexpr int64_t LINK_MAX = (int64_t)1 << 40; // every product below stays far inside int64

static int link_shapes(int64_t E, int64_t K, int32_t mode, const char *who, int64_t &S, int64_t &P) {
    TG_REQUIRE(mode == TG_LINK_BINARY || mode == TG_LINK_TRIPLET, "%s: mode = %d is neither TG_LINK_BINARY nor TG_LINK_TRIPLET",
               who, (int)mode);
    TG_REQUIRE(E >= 0 && E < LINK_MAX, "%s: n_edges = %lld, must be >= 0", who, (long long)E);
    TG_REQUIRE(K >= 0 && K < LINK_MAX, "%s: n_neg = %lld, must be >= 0", who, (long long)K);
    const __int128 pairs = (__int128)E * (1 + K);
    TG_REQUIRE(pairs < ((__int128)1 << 58), "%s: %lld edges with %lld negatives each are too many", who, (long long)E,
               (long long)K);
    P = (int64_t)pairs;
    S = mode == TG_LINK_BINARY ? 2 * P : E + P;
    return TG_OK;
}

} // namespace tg

extern "C" int tg_link_seeds_capacity(int64_t n_edges, int64_t n_neg, int32_t mode, int64_t *seeds_per_batch, int64_t *pairs) {
    using namespace tg;
    const char *who = "tg_link_seeds_capacity";
    TG_REQUIRE(seeds_per_batch && pairs, "%s: null output", who);
    int64_t S, P;
    if (const int rc = link_shapes(n_edges, n_neg, mode, who, S, P)) return rc;
    *seeds_per_batch = S;
    *pairs = P;
    return TG_OK;
}

extern "C" int tg_link_seeds(const tg_graph *csc, const void *edge_set, int64_t edge_set_bytes, const int64_t *src,
                             const int64_t *dst, int64_t n_batches, int64_t n_edges, int64_t n_neg, int32_t mode,
                             int32_t try_count, const tg_rng *rng, int64_t n_nodes, int64_t *seeds, int64_t *unverified,
                             void *stream_) {
    using namespace tg;
    const char *who = "tg_link_seeds";
    const int64_t G = n_batches, E = n_edges, K = n_neg;
    int64_t S, P;
    if (const int rc = link_shapes(E, K, mode, who, S, P)) return rc;
    TG_REQUIRE(G >= 0 && G < LINK_MAX, "%s: n_batches = %lld, must be >= 0", who, (long long)G);
    TG_REQUIRE(try_count >= 1, "%s: try_count = %d, must be >= 1", who, (int)try_count);
    TG_REQUIRE(n_nodes >= 1, "%s: n_nodes = %lld, must be >= 1", who, (long long)n_nodes);
    TG_REQUIRE(rng, "%s: null rng", who);
    TG_REQUIRE(csc && csc->ptrs && (csc->indices || csc->n_edges == 0), "%s: null graph", who);
    TG_REQUIRE(csc->n_edges >= 0 && n_nodes == csc->n_major, "%s: n_nodes = %lld is not the graph's %lld columns", who,
               (long long)n_nodes, (long long)csc->n_major);
    uint64_t edge_mask = 0;
    if (edge_set) {
        TG_REQUIRE(csc->n_major < (int64_t)0xffffffff, "%s: the edge set holds ids below 2^32 - 1, the graph has %lld columns", who,
                   (long long)csc->n_major);
        const int64_t cap = edge_set_slots(csc->n_edges);
        TG_REQUIRE(edge_set_bytes == 8 * cap, "%s: the edge set (%lld bytes) was not built for this graph (%lld bytes)", who,
                   (long long)edge_set_bytes, (long long)(8 * cap));
        edge_mask = (uint64_t)(cap - 1);
    }
    TG_REQUIRE((__int128)G * S < ((__int128)1 << 59), "%s: %lld mini-batches of %lld seeds are too many", who, (long long)G,
               (long long)S);
    if (G == 0 || E == 0) return TG_OK;
    TG_REQUIRE(src && dst && seeds, "%s: null buffers", who);
    LinkSeedsParams p;
    p.g = CsrView{csc->ptrs, csc->indices, csc->ptrs32, csc->indices32, reinterpret_cast<const uint64_t *>(edge_set), edge_mask};
    p.src = src, p.dst = dst;
    p.E = E, p.K = K, p.N = K * E, p.S = S, p.P = P;
    p.n_neg = G * p.N, p.n_copy = G * 2 * E;
    p.neg_blocks = (p.n_neg + LINK_THREADS - 1) / LINK_THREADS;
    const int64_t copy_blocks = (p.n_copy + LINK_THREADS - 1) / LINK_THREADS;
    TG_REQUIRE(p.neg_blocks + copy_blocks <= 0x7fffffff, "%s: %lld seeds are more than one launch takes", who,
               (long long)(G * S));
    p.mode = mode, p.try_count = try_count;
    p.seed = rng->seed, p.call_id = rng->call_id, p.n_nodes = (uint64_t)n_nodes;
    p.seeds = seeds;
    p.unverified = reinterpret_cast<unsigned long long *>(unverified);
    hipStream_t stream = (hipStream_t)stream_;
    if (unverified) TG_HIP(hipMemsetAsync(unverified, 0, (size_t)G * 8, stream));
    hipLaunchKernelGGL(link_seeds_kernel, dim3((unsigned)(p.neg_blocks + copy_blocks)), dim3(LINK_THREADS), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_link_seeds_typed(const tg_link_rel *rel, const int64_t *src, const int64_t *dst, int64_t n_batches,
                                   int64_t n_edges, int64_t n_neg, int32_t mode, int32_t try_count, const tg_rng *rng,
                                   int64_t *src_seeds, int64_t src_pitch, int64_t *dst_seeds, int64_t dst_pitch,
                                   int64_t *unverified, void *stream_) {
    using namespace tg;
    const char *who = "tg_link_seeds_typed";
    const int64_t G = n_batches, E = n_edges, K = n_neg;
    int64_t S, P;
    if (const int rc = link_shapes(E, K, mode, who, S, P)) return rc;
    const int64_t Ws = mode == TG_LINK_BINARY ? P : E, Wd = P;
    TG_REQUIRE(G >= 0 && G < LINK_MAX, "%s: n_batches = %lld, must be >= 0", who, (long long)G);
    TG_REQUIRE(try_count >= 1, "%s: try_count = %d, must be >= 1", who, (int)try_count);
    TG_REQUIRE(rng, "%s: null rng", who);
    TG_REQUIRE(rel, "%s: null rel", who);
    const tg_graph *csc = rel->csc;
    TG_REQUIRE(csc && csc->ptrs && (csc->indices || csc->n_edges == 0), "%s: null graph (rel->csc)", who);
    TG_REQUIRE(rel->n_src >= 1, "%s: n_src = %lld, must be >= 1", who, (long long)rel->n_src);
    TG_REQUIRE(rel->n_dst >= 1, "%s: n_dst = %lld, must be >= 1", who, (long long)rel->n_dst);
    TG_REQUIRE(csc->n_edges >= 0 && rel->n_dst == csc->n_major, "%s: n_dst = %lld is not the graph's %lld columns", who,
               (long long)rel->n_dst, (long long)csc->n_major);
    TG_REQUIRE(!rel->same_type || rel->n_src == rel->n_dst, "%s: same_type needs n_src == n_dst, got n_src = %lld, n_dst = %lld",
               who, (long long)rel->n_src, (long long)rel->n_dst);
    TG_REQUIRE(src_pitch >= Ws, "%s: src_pitch = %lld is below the source row's %lld words", who, (long long)src_pitch,
               (long long)Ws);
    TG_REQUIRE(dst_pitch >= Wd, "%s: dst_pitch = %lld is below the destination row's %lld words", who, (long long)dst_pitch,
               (long long)Wd);
    uint64_t edge_mask = 0;
    if (rel->edge_set) {
        TG_REQUIRE(rel->n_src < (int64_t)0xffffffff && rel->n_dst < (int64_t)0xffffffff,
                   "%s: the edge set holds ids below 2^32 - 1, got n_src = %lld, n_dst = %lld", who, (long long)rel->n_src,
                   (long long)rel->n_dst);
        const int64_t cap = edge_set_slots(csc->n_edges);
        TG_REQUIRE(rel->edge_set_bytes == 8 * cap, "%s: the edge set (%lld bytes) was not built for this graph (%lld bytes)", who,
                   (long long)rel->edge_set_bytes, (long long)(8 * cap));
        edge_mask = (uint64_t)(cap - 1);
    }
    TG_REQUIRE((__int128)G * src_pitch < ((__int128)1 << 59) && (__int128)G * dst_pitch < ((__int128)1 << 59),
               "%s: %lld mini-batches at pitches %lld and %lld are too many", who, (long long)G, (long long)src_pitch,
               (long long)dst_pitch);
    if (G == 0 || E == 0) return TG_OK;
    TG_REQUIRE(src && dst && src_seeds && dst_seeds, "%s: null buffers", who);
    {   // the two regions are disjoint, or their rows interleave inside one pitch (tg_link_seeds' row: dst = src + Ws)
        const int64_t *s0 = src_seeds, *s1 = src_seeds + (G - 1) * src_pitch + Ws;
        const int64_t *d0 = dst_seeds, *d1 = dst_seeds + (G - 1) * dst_pitch + Wd;
        const bool disjoint = s1 <= d0 || d1 <= s0;
        const int64_t off = d0 >= s0 ? d0 - s0 : s0 - d0, lead = d0 >= s0 ? Ws : Wd, trail = d0 >= s0 ? Wd : Ws;
        const bool interleaved = src_pitch == dst_pitch && off >= lead && off + trail <= src_pitch;
        TG_REQUIRE(disjoint || interleaved, "%s: src_seeds and dst_seeds overlap", who);
    }
    LinkSeedsTypedParams p;
    p.g = CsrView{csc->ptrs, csc->indices, csc->ptrs32, csc->indices32, reinterpret_cast<const uint64_t *>(rel->edge_set),
                  edge_mask};
    p.src = src, p.dst = dst;
    p.E = E, p.K = K, p.N = K * E;
    p.n_neg = G * p.N, p.n_copy = G * 2 * E;
    p.neg_blocks = (p.n_neg + LINK_THREADS - 1) / LINK_THREADS;
    const int64_t copy_blocks = (p.n_copy + LINK_THREADS - 1) / LINK_THREADS;
    TG_REQUIRE(p.neg_blocks + copy_blocks <= 0x7fffffff, "%s: %lld seeds are more than one launch takes", who,
               (long long)(G * S));
    p.mode = mode, p.try_count = try_count, p.same_type = rel->same_type != 0;
    p.seed = rng->seed, p.call_id = rng->call_id, p.n_src = (uint64_t)rel->n_src, p.n_dst = (uint64_t)rel->n_dst;
    p.src_out = src_seeds, p.dst_out = dst_seeds, p.src_pitch = src_pitch, p.dst_pitch = dst_pitch;
    p.unverified = reinterpret_cast<unsigned long long *>(unverified);
    hipStream_t stream = (hipStream_t)stream_;
    if (unverified) TG_HIP(hipMemsetAsync(unverified, 0, (size_t)G * 8, stream));
    hipLaunchKernelGGL(link_seeds_typed_kernel, dim3((unsigned)(p.neg_blocks + copy_blocks)), dim3(LINK_THREADS), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
