// Per-batch node dedup and relabel of the tg_ns_homo_batched slabs (include/tchgeo.h): tg_ns_homo_unique, and
// tg_ns_homo_unique_grouped, the same with a group dimension -- PyG's disjoint=True, one subgraph per group of seeds.
// Both are ONE set of kernels, template <bool G, typename K>: G says whether there are groups, K is the key width.  What
// G adds sits behind `if constexpr (G)` and in the tail of the argument struct (NsgArgs); the G = false instantiations see
// NsuArgs alone and compile to what they were before there were groups (tools/kernel_diff.py holds them to it: code
// generation is sensitive to where things are declared, so a change here is checked on the assembly, not on the source).
//
// The rule, per batch: nodes = the distinct values of samples[:n] in order of FIRST occurrence, inverse[p] = index of
// samples[p] in nodes, rows / cols = inverse[rows], inverse[cols].  Both forms compute it the same way (the insert, the scan
// and the flat form's clear, flag and apply tile bodies are ns_unique.h's, shared with ns_unique_typed.hip):
//   1. an open-addressing table (tg_map.h / negative_batched.inl): the key is claimed with atomicCAS, then atomicMin of
//      the position into the slot's value -- the value ends as the id's first position whatever order lanes arrive in;
//   2. position p is a first occurrence iff value[slot(p)] == p; local ids are the exclusive scan of those flags in
//      position order, written back into the slot's value;
//   3. inverse[p] = value[slot(p)], edges go through it.
// layer_nodes[h] is the scan's value at position layer_offsets[h][0].
//
// With groups: root(p) = p for a seed position, else root(cols[p - n_seeds]) (the forest: rows[e] = n_seeds + e, cols[e] <
// n_seeds + e, so a chase ends after at most n_hops parents); group(p) = seed_group[root(p)]; nodes = the distinct PAIRS
// (group(p), samples[p]) in order of first occurrence, group[u] = the group of nodes[u]; inverse, rows, cols, counts,
// layer_nodes as above, over the pair.  The pair is ONE hash key, group * id_bound + id, so steps 1 to 3 are unchanged.
// What is new is the chase and one group word per position.  The chase is capped at n_hops steps, every parent must be
// smaller than its child and every edge index below m: a batch that breaks the forest contract gets group 0 for the
// position, nothing is read or written outside the batch's slabs.
//
// LDS form: ONE workgroup runs ONE batch; keys, values and a u16 word per position (the slot, later the local id) live in
//   LDS, so only the slab reads and the output stores touch global memory.  A table of cap = 2^k >= 4/3 cap_nodes slots
//   (load factor <= 0.75) of (key, u32 value) must fit: cap_nodes <= 12 288 with 32-bit keys in 160 KiB, 6 144 with 64-bit.
//   Groups: a u16 word next to the position's slot word (n_groups <= 65 536, else the shape takes the flat form); the
//   chase runs in the insert phase, barriers before the edge phase -- in place is safe by PHASE order.
// Flat form: the loader's shape (1 024 x [15,10]: 169 984 positions, 16 batches) fits no LDS and has too few batches to
//   fill the device batch by batch, so the grid runs over POSITIONS of all batches: clear | insert | flag + tile counts |
//   apply (a block sums the counts of the tiles before its own, scans its tile, names the first occurrences) | relabel.
//   Tables, the per-position slot words and the tile counts of a batch sit in the workspace.
//   Groups: a u32 word per position in the workspace, written by the insert kernel, read by the apply kernel; the
//   relabel kernel is the only one that writes rows / cols and runs last -- in place is safe by KERNEL order.
// Every probe loop is capped at the table size: an id outside [0, id_bound) ends it instead of spinning.
#include <algorithm>
#include <type_traits>

#include "ns_unique.h"

namespace tg {

struct NsuArgs {
    const int64_t *samples, *rows, *cols, *layer_offsets, *counts; // batch 0 of the round
    int64_t *nodes, *inverse, *rows_u, *cols_u, *counts_u, *layer_nodes;
    int64_t cap_nodes, cap_edges, n_batches;
    int32_t n_hops;
    uint32_t cap_mask, hash_shift;
    // flat form: the round's tables
    unsigned char *ws;
    int64_t batch_bytes, vals_off, slot_off, tile_off;
    int32_t n_node_tiles, inv_tiles;
};
struct NsgArgs : NsuArgs {     // what the groups add
    const int32_t *seed_group; // [n_seeds] or null: the identity
    int64_t *group;
    int64_t n_seeds;
    uint64_t key_mul;          // id_bound: key = group * key_mul + id
    int64_t grp_off;           // flat form: the group words of a batch's part of the workspace
};
template <bool G> using NsuArgsOf = std::conditional_t<G, NsgArgs, NsuArgs>;

// the group of position p < n of a batch with m edges; 0 where the batch breaks the forest contract
__device__ __forceinline__ uint32_t nsu_group_of(const NsgArgs &a, const int64_t *cols, int64_t p, int64_t m) {
    int64_t q = p;
    for (int step = 0; step < a.n_hops && q >= a.n_seeds; ++step) {
        const int64_t e = q - a.n_seeds;
        if (e >= m) return 0;
        const int64_t c = cols[e];
        if ((uint64_t)c >= (uint64_t)q) return 0; // a parent sits before its child: q only falls, and stays a position
        q = c;
    }
    if (q >= a.n_seeds) return 0;
    return a.seed_group ? (uint32_t)a.seed_group[q] : (uint32_t)q;
}

// ---- LDS form ------------------------------------------------------------------------------------------------------------
template <bool G, typename K> __global__ void __launch_bounds__(NSU_THREADS) nsu_lds_kernel(const NsuArgsOf<G> a) {
    extern __shared__ __align__(16) unsigned char nsu_lds[];
    __shared__ uint32_t s_wave[NSU_THREADS / 64];
    const uint32_t cap = a.cap_mask + 1;
    K *keys = reinterpret_cast<K *>(nsu_lds);
    uint32_t *vals = reinterpret_cast<uint32_t *>(keys + cap);
    uint16_t *loc = reinterpret_cast<uint16_t *>(vals + cap);             // [cap_nodes]: the position's slot, later its local id
    uint16_t *grp = G ? loc + ((a.cap_nodes + 7) & ~(int64_t)7) : nullptr; // [cap_nodes]: the position's group
    const int tid = threadIdx.x, nt = blockDim.x;

    for (int64_t b = blockIdx.x; b < a.n_batches; b += gridDim.x) {
        const int n = (int)nsu_clamp(a.counts[b * 2], a.cap_nodes);
        const int64_t m = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
        const int64_t *samples = a.samples + b * a.cap_nodes;
        const int64_t *chase = G ? a.cols + b * a.cap_edges : nullptr; // the input cols, read by the insert phase alone
        for (uint32_t s = tid; s < cap; s += nt) {
            keys[s] = nsu_empty<K>();
            vals[s] = NSU_UNSEEN;
        }
        __syncthreads(); // also: the previous batch is done with `loc` and `grp`
        for (int p = tid; p < n; p += nt) {
            K key = (K)samples[p];
            uint32_t g = 0;
            if constexpr (G) {
                g = nsu_group_of(a, chase, p, m);
                key += (K)g * (K)a.key_mul; // the pair is one key
            }
            const uint32_t s = nsu_insert<K>(keys, a.cap_mask, a.hash_shift, key);
            atomicMin(&vals[s], (uint32_t)p);
            loc[p] = (uint16_t)s;
            if constexpr (G) grp[p] = (uint16_t)g;
        }
        __syncthreads(); // every group is known: nothing below reads the input cols except the edge phase itself
        // first occurrences, ranked in position order: a thread owns a contiguous run of positions
        const int per = (n + nt - 1) / nt; // <= NSU_MAX_PER_THREAD
        const int p0 = min(n, tid * per), p1 = min(n, p0 + per);
        uint32_t first = 0;
        for (int p = p0; p < p1; ++p)
            if (vals[loc[p]] == (uint32_t)p) first |= 1u << (p - p0);
        uint32_t n_unique;
        const uint32_t rank0 = nsu_scan((uint32_t)__popc(first), s_wave, &n_unique); // barriers: every value is read
        int64_t *nodes = a.nodes + b * a.cap_nodes;
        uint32_t rank = rank0;
        for (uint32_t f = first; f;) {
            const int p = p0 + __ffs(f) - 1;
            f &= f - 1;
            vals[loc[p]] = rank;
            if constexpr (G) a.group[b * a.cap_nodes + rank] = (int64_t)grp[p];
            nodes[rank++] = samples[p];
        }
        if (a.layer_nodes) {
            for (int h = 0; h < a.n_hops; ++h) {
                const int64_t L = nsu_clamp(a.layer_offsets[(b * a.n_hops + h) * 3], n);
                if (L >= n) {
                    if (tid == 0) a.layer_nodes[b * a.n_hops + h] = (int64_t)n_unique;
                } else if (L >= p0 && L < p1) {
                    a.layer_nodes[b * a.n_hops + h] = (int64_t)(rank0 + __popc(first & ((1u << (int)(L - p0)) - 1u)));
                }
            }
        }
        if (tid == 0) {
            a.counts_u[b * 2] = (int64_t)n_unique;
            a.counts_u[b * 2 + 1] = m;
        }
        __syncthreads();
        int64_t *inverse = a.inverse ? a.inverse + b * a.cap_nodes : nullptr;
        for (int p = tid; p < n; p += nt) {
            const uint32_t id = vals[loc[p]];
            loc[p] = (uint16_t)id;
            if (inverse) inverse[p] = (int64_t)id;
        }
        __syncthreads();
        const int64_t *rows = a.rows + b * a.cap_edges, *cols = a.cols + b * a.cap_edges;
        int64_t *rows_u = a.rows_u + b * a.cap_edges, *cols_u = a.cols_u + b * a.cap_edges;
        const auto lookup = [&](int64_t r) { return loc[r]; };
        for (int64_t e = tid; e < m; e += nt) { // element e is read before it is written: in place is fine
            const int64_t r = rows[e], c = cols[e];
            rows_u[e] = nsu_end(r, n, lookup);
            cols_u[e] = nsu_end(c, n, lookup);
        }
        __syncthreads(); // the next batch clears the table
    }
}

// ---- flat form -------------------------------------------------------------------------------------------------------------
template <bool G, typename K> struct NsuBatch {
    K *keys;
    uint32_t *vals, *slot, *tile_cnt, *grp;
    __device__ __forceinline__ NsuBatch(const NsuArgsOf<G> &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        keys = reinterpret_cast<K *>(base);
        vals = reinterpret_cast<uint32_t *>(base + a.vals_off);
        slot = reinterpret_cast<uint32_t *>(base + a.slot_off);
        tile_cnt = reinterpret_cast<uint32_t *>(base + a.tile_off);
        if constexpr (G)
            grp = reinterpret_cast<uint32_t *>(base + a.grp_off);
        else
            grp = nullptr;
    }
};

template <bool G, typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_clear_kernel(const NsuArgsOf<G> a) {
    const NsuBatch<G, K> t(a, blockIdx.y);
    nsu_clear_tile<K>(t.keys, t.vals, a.cap_mask + 1, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// the insert of a tile of positions (with groups: the chase and the group word too); reads the input cols, writes none
template <bool G, typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_insert_kernel(const NsuArgsOf<G> a) {
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n) return;
    const int64_t m = G ? nsu_clamp(a.counts[b * 2 + 1], a.cap_edges) : 0;
    const NsuBatch<G, K> t(a, b);
    const int64_t *samples = a.samples + b * a.cap_nodes, *chase = G ? a.cols + b * a.cap_edges : nullptr;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (p < n) {
            K key = (K)samples[p];
            uint32_t g = 0;
            if constexpr (G) {
                g = nsu_group_of(a, chase, p, m);
                key += (K)g * (K)a.key_mul; // the pair is one key
            }
            const uint32_t s = nsu_insert<K>(t.keys, a.cap_mask, a.hash_shift, key);
            atomicMin(&t.vals[s], (uint32_t)p);
            t.slot[p] = s;
            if constexpr (G) t.grp[p] = g;
        }
    }
}

template <bool G, typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_flag_kernel(const NsuArgsOf<G> a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsuBatch<G, K> t(a, b);
    nsu_flag_tile(t, n, tile0, s_wave);
}

template <bool G, typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_apply_kernel(const NsuArgsOf<G> a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsuBatch<G, K> t(a, b);
    const NsuRanks r = nsu_apply_tile(t, n, tile0, a.samples + b * a.cap_nodes, a.nodes + b * a.cap_nodes, s_wave,
                                      [&](uint32_t rank, int64_t p) {
                                          if constexpr (G) a.group[b * a.cap_nodes + rank] = (int64_t)t.grp[p];
                                      });
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    const bool last = tile0 + NSU_TILE >= n; // the batch's last tile (tile 0 of an empty batch)
    if (a.layer_nodes) {
        for (int h = 0; h < a.n_hops; ++h) {
            const int64_t L = nsu_clamp(a.layer_offsets[(b * a.n_hops + h) * 3], n);
            if (L >= n) {
                if (last && threadIdx.x == 0) a.layer_nodes[b * a.n_hops + h] = (int64_t)(r.base + r.total);
            } else if (L >= p0 && L < p0 + NSU_PER) {
                a.layer_nodes[b * a.n_hops + h] = (int64_t)(r.rank0 + __popc(r.first & ((1u << (int)(L - p0)) - 1u)));
            }
        }
    }
    if (last && threadIdx.x == 0) {
        a.counts_u[b * 2] = (int64_t)(r.base + r.total);
        a.counts_u[b * 2 + 1] = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
    }
}

// blocks [0, inv_tiles): inverse of a tile of positions; the others: a tile of edges.  The only kernel that writes rows /
// cols, and the last one: every chase is over
template <bool G, typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_relabel_kernel(const NsuArgsOf<G> a) {
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const NsuBatch<G, K> t(a, b);
    const auto lookup = [&](int64_t p) { return t.vals[t.slot[p] & ~NSU_FLAG]; };
    if ((int)blockIdx.x < a.inv_tiles) {
        const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
        int64_t *inverse = a.inverse + b * a.cap_nodes;
#pragma unroll
        for (int k = 0; k < NSU_PER; ++k) {
            const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
            if (p < n) inverse[p] = (int64_t)lookup(p);
        }
        return;
    }
    const int64_t m = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
    const int64_t tile0 = (int64_t)((int)blockIdx.x - a.inv_tiles) * NSU_EDGE_TILE;
    if (tile0 >= m) return;
    const int64_t *rows = a.rows + b * a.cap_edges, *cols = a.cols + b * a.cap_edges;
    int64_t *rows_u = a.rows_u + b * a.cap_edges, *cols_u = a.cols_u + b * a.cap_edges;
    int64_t r[NSU_EDGE_PER], c[NSU_EDGE_PER];
#pragma unroll
    for (int k = 0; k < NSU_EDGE_PER; ++k) { // element e is read before it is written: in place is fine
        const int64_t e = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        r[k] = e < m ? rows[e] : -1;
        c[k] = e < m ? cols[e] : -1;
    }
#pragma unroll
    for (int k = 0; k < NSU_EDGE_PER; ++k) {
        const int64_t e = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (e < m) {
            rows_u[e] = nsu_end(r[k], n, lookup);
            cols_u[e] = nsu_end(c[k], n, lookup);
        }
    }
}

// ---- host side (the plan, what a shape needs and which form it takes: ns_unique.h) --------------------------------------
// nsu_plan for the pair key, plus the group word per position: u16 in LDS behind the slot words, u32 behind the tile counts
// of a batch's workspace.  nsu_plan itself is untouched: tg_ns_homo_unique and tg_ns_induced_* get from it what they got.
struct NsgPlan {
    NsuPlan u;
    int64_t grp_off;
};

static int nsg_plan(int64_t cap_nodes, int64_t id_bound, int64_t n_groups, const char *who, NsgPlan &pl) {
    TG_REQUIRE(id_bound >= 1, "%s: id_bound = %lld, at least 1 expected", who, (long long)id_bound);
    TG_REQUIRE(n_groups >= 1, "%s: n_groups = %lld, at least 1 expected", who, (long long)n_groups);
    TG_REQUIRE(n_groups <= 0x7fffffff, "%s: n_groups = %lld does not fit the int32 group map", who, (long long)n_groups);
    TG_REQUIRE(id_bound <= INT64_MAX / n_groups, "%s: n_groups * id_bound = %lld * %lld reaches 2^63: no key holds the pair",
               who, (long long)n_groups, (long long)id_bound);
    if (const int rc = nsu_plan(cap_nodes, n_groups * id_bound, who, pl.u)) return rc; // the key bound picks the key width
    pl.u.lds_bytes += (2 * cap_nodes + 15) & ~(int64_t)15;
    pl.u.lds_ok = pl.u.lds_ok && n_groups <= 65536;
    pl.grp_off = pl.u.batch_bytes;
    pl.u.batch_bytes += nsu_r256(cap_nodes * 4);
    return TG_OK;
}

// the two size queries, behind their own argument checks and plan
static int nsu_form_of(const NsuPlan &pl, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes) {
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : nsu_device_lds_limit();
    *form = nsu_fits(pl, limit) ? 1 : 2;
    *lds_bytes = pl.lds_bytes;
    return TG_OK;
}

static int nsu_workspace_of(const NsuPlan &pl, int64_t n_batches, int64_t *bytes, int64_t *bytes_min) {
    *bytes_min = pl.batch_bytes;
    *bytes = nsu_fits(pl, nsu_device_lds_limit()) ? 0 : pl.batch_bytes * n_batches;
    return TG_OK;
}

template <bool G, typename K> static int nsu_launch_lds(const NsuArgsOf<G> &a, const NsuPlan &pl, hipStream_t stream) {
    const int64_t dyn = pl.lds_bytes - NSU_STATIC_LDS;
    static std::atomic<int64_t> raised[64];
    if (const int rc = nsu_raise_lds(reinterpret_cast<const void *>(nsu_lds_kernel<G, K>), raised, dyn)) return rc;
    const unsigned grid = (unsigned)(a.n_batches < 16384 ? a.n_batches : 16384);
    hipLaunchKernelGGL((nsu_lds_kernel<G, K>), dim3(grid), dim3(pl.threads), (size_t)dyn, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <bool G, typename K> static int nsu_launch_flat(const NsuArgsOf<G> &a, const NsuPlan &pl, hipStream_t stream) {
    const unsigned nb = (unsigned)a.n_batches, tiles = (unsigned)pl.n_node_tiles;
    const dim3 block(NSU_TILE_THREADS);
    const int64_t clear_blocks = (pl.table_cap + NSU_TILE_THREADS - 1) / NSU_TILE_THREADS;
    hipLaunchKernelGGL((nsu_clear_kernel<G, K>), dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024), nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL((nsu_insert_kernel<G, K>), dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL((nsu_flag_kernel<G, K>), dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL((nsu_apply_kernel<G, K>), dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    const int64_t edge_tiles = (a.cap_edges + NSU_EDGE_TILE - 1) / NSU_EDGE_TILE;
    if (a.inv_tiles + edge_tiles > 0) {
        hipLaunchKernelGGL((nsu_relabel_kernel<G, K>), dim3((unsigned)(a.inv_tiles + edge_tiles), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
    }
    return TG_OK;
}

// both calls: the argument checks, the plan, the form, the rounds.  seed_group, n_groups and out->group count only with G
template <bool G>
static int nsu_run(const char *who, const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops, int64_t id_bound,
                   const int32_t *seed_group, int64_t n_groups,
                   const std::conditional_t<G, tg_ns_unique_grouped_out, tg_ns_unique_out> *out, void *workspace,
                   int64_t workspace_bytes, int32_t form, void *stream_) {
    TG_REQUIRE(in && out, "%s: null argument", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(n_seeds >= 0, "%s: n_seeds = %lld is negative", who, (long long)n_seeds);
    TG_REQUIRE(n_hops >= 0 && n_hops <= TG_MAX_HOPS, "%s: n_hops = %d outside [0, %d]", who, n_hops, TG_MAX_HOPS);
    TG_REQUIRE(in->cap_edges >= 0, "%s: cap_edges = %lld is negative", who, (long long)in->cap_edges);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    NsgPlan gpl{};
    if (const int rc = G ? nsg_plan(in->cap_nodes, id_bound, n_groups, who, gpl) : nsu_plan(in->cap_nodes, id_bound, who, gpl.u))
        return rc;
    const NsuPlan &pl = gpl.u;
    if constexpr (G)
        TG_REQUIRE(seed_group || n_groups == n_seeds, "%s: n_groups = %lld without a seed_group map: the identity has n_seeds = %lld groups",
                   who, (long long)n_groups, (long long)n_seeds);
    TG_REQUIRE(n_seeds <= in->cap_nodes, "%s: n_seeds = %lld above cap_nodes = %lld", who, (long long)n_seeds,
               (long long)in->cap_nodes);
    const bool fits = form != 2 && nsu_fits(pl, nsu_device_lds_limit());
    if constexpr (G)
        TG_REQUIRE(form != 1 || fits, "%s: form 1: a table of %lld slots (%lld bytes of LDS, %lld groups) does not fit a workgroup", who,
                   (long long)pl.table_cap, (long long)pl.lds_bytes, (long long)n_groups);
    else
        TG_REQUIRE(form != 1 || fits, "%s: form 1: a table of %lld slots (%lld bytes of LDS) does not fit a workgroup", who,
                   (long long)pl.table_cap, (long long)pl.lds_bytes);
    const bool lds = form != 2 && fits;
    if (!lds)
        TG_REQUIRE(workspace && workspace_bytes >= pl.batch_bytes, "%s: workspace too small (%lld < %lld, the size of one batch)",
                   who, (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    if (n_batches == 0) return TG_OK;
    // device pointers
    if constexpr (G)
        TG_REQUIRE(in->samples && in->counts && out->nodes && out->group && out->counts, "%s: null samples / counts / nodes / group", who);
    else
        TG_REQUIRE(in->samples && in->counts && out->nodes && out->counts, "%s: null samples / counts / nodes", who);
    TG_REQUIRE(in->cap_edges == 0 || (in->rows && in->cols && out->rows && out->cols), "%s: null edge slab", who);
    TG_REQUIRE(n_hops == 0 || !out->layer_nodes || in->layer_offsets, "%s: layer_nodes asked for without layer_offsets (null)", who);
    hipStream_t stream = (hipStream_t)stream_;

    const int64_t round = lds ? n_batches : std::min(std::min(workspace_bytes / pl.batch_bytes, NSU_ROUND_MAX), n_batches);
    for (int64_t b0 = 0; b0 < n_batches; b0 += round) {
        NsuArgsOf<G> a{};
        a.samples = in->samples + b0 * in->cap_nodes, a.counts = in->counts + b0 * 2;
        a.rows = in->rows ? in->rows + b0 * in->cap_edges : nullptr, a.cols = in->cols ? in->cols + b0 * in->cap_edges : nullptr;
        a.layer_offsets = in->layer_offsets ? in->layer_offsets + b0 * n_hops * 3 : nullptr;
        a.nodes = out->nodes + b0 * in->cap_nodes, a.counts_u = out->counts + b0 * 2;
        a.inverse = out->inverse ? out->inverse + b0 * in->cap_nodes : nullptr;
        a.rows_u = out->rows ? out->rows + b0 * in->cap_edges : nullptr;
        a.cols_u = out->cols ? out->cols + b0 * in->cap_edges : nullptr;
        a.layer_nodes = out->layer_nodes ? out->layer_nodes + b0 * n_hops : nullptr;
        a.cap_nodes = in->cap_nodes, a.cap_edges = in->cap_edges, a.n_hops = n_hops;
        a.n_batches = std::min(round, n_batches - b0);
        nsu_mask_shift(pl.table_cap, a.cap_mask, a.hash_shift);
        a.ws = static_cast<unsigned char *>(workspace);
        a.batch_bytes = pl.batch_bytes, a.vals_off = pl.vals_off, a.slot_off = pl.slot_off, a.tile_off = pl.tile_off;
        a.n_node_tiles = (int32_t)pl.n_node_tiles, a.inv_tiles = a.inverse ? (int32_t)pl.n_node_tiles : 0;
        if constexpr (G) {
            a.seed_group = seed_group, a.group = out->group + b0 * in->cap_nodes;
            a.n_seeds = n_seeds, a.key_mul = (uint64_t)id_bound, a.grp_off = gpl.grp_off;
        }
        const bool k32 = pl.key_bytes == 4;
        const int rc = lds ? (k32 ? nsu_launch_lds<G, nsu_k32> : nsu_launch_lds<G, nsu_k64>)(a, pl, stream)
                           : (k32 ? nsu_launch_flat<G, nsu_k32> : nsu_launch_flat<G, nsu_k64>)(a, pl, stream);
        if (rc) return rc;
    }
    return TG_OK;
}

} // namespace tg

extern "C" int tg_ns_homo_unique_form(int64_t cap_nodes, int64_t id_bound, int64_t lds_limit_bytes, int32_t *form,
                                      int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    NsuPlan pl;
    if (const int rc = nsu_plan(cap_nodes, id_bound, who, pl)) return rc;
    return nsu_form_of(pl, lds_limit_bytes, form, lds_bytes);
}

extern "C" int tg_ns_homo_unique_grouped_form(int64_t cap_nodes, int64_t id_bound, int64_t n_groups, int64_t lds_limit_bytes,
                                              int32_t *form, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_grouped_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    NsgPlan pl;
    if (const int rc = nsg_plan(cap_nodes, id_bound, n_groups, who, pl)) return rc;
    return nsu_form_of(pl.u, lds_limit_bytes, form, lds_bytes);
}

extern "C" int tg_ns_homo_unique_workspace_bytes(int64_t cap_nodes, int64_t id_bound, int64_t n_batches, int64_t *bytes,
                                                 int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    NsuPlan pl;
    if (const int rc = nsu_plan(cap_nodes, id_bound, who, pl)) return rc;
    return nsu_workspace_of(pl, n_batches, bytes, bytes_min);
}

extern "C" int tg_ns_homo_unique_grouped_workspace_bytes(int64_t cap_nodes, int64_t id_bound, int64_t n_groups,
                                                         int64_t n_batches, int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_grouped_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    NsgPlan pl;
    if (const int rc = nsg_plan(cap_nodes, id_bound, n_groups, who, pl)) return rc;
    return nsu_workspace_of(pl.u, n_batches, bytes, bytes_min);
}

extern "C" int tg_ns_homo_unique(const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops, int64_t id_bound,
                                 const tg_ns_unique_out *out, void *workspace, int64_t workspace_bytes, int32_t form,
                                 void *stream) {
    return tg::nsu_run<false>("tg_ns_homo_unique", in, n_batches, n_seeds, n_hops, id_bound, nullptr, 1, out, workspace,
                              workspace_bytes, form, stream);
}

extern "C" int tg_ns_homo_unique_grouped(const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops,
                                         int64_t id_bound, const int32_t *seed_group, int64_t n_groups,
                                         const tg_ns_unique_grouped_out *out, void *workspace, int64_t workspace_bytes,
                                         int32_t form, void *stream) {
    return tg::nsu_run<true>("tg_ns_homo_unique_grouped", in, n_batches, n_seeds, n_hops, id_bound, seed_group, n_groups, out,
                             workspace, workspace_bytes, form, stream);
}
