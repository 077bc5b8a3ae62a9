// Per-batch, per-GROUP node dedup and relabel of the tg_ns_homo_batched slabs (tg_ns_homo_unique_grouped, include/tchgeo.h):
// tg_ns_homo_unique (ns_unique.hip) with a group dimension -- PyG's disjoint=True, one subgraph per group of seeds.
//
// The rule, per batch: root(p) = p for a seed position, else root(cols[p - n_seeds]) (the forest: rows[e] = n_seeds + e,
// cols[e] < n_seeds + e, so a chase ends after at most n_hops parents); group(p) = seed_group[root(p)]; nodes = the
// distinct pairs (group(p), samples[p]) in order of FIRST occurrence, group[u] = the group of nodes[u]; inverse, rows,
// cols, counts, layer_nodes as tg_ns_homo_unique has them, over the pair.  The pair is ONE hash key, group * id_bound + id,
// so the table, the atomicMin of the first position, the rank scan and the relabel are ns_unique.hip's steps (ns_unique.h
// holds what the two share; the kernels are this file's own, as ns_unique_typed.hip's are, so that nothing tg_ns_homo_unique
// launches changes).  What is new is the chase and one group word per position:
//   LDS form:  a u16 word next to the position's slot word (n_groups <= 65 536, else the shape takes the flat form); the
//              chase runs in the insert phase, barriers before the edge phase -- in place is safe by PHASE order;
//   flat form: a u32 word per position in the workspace, written by the insert kernel, read by the apply kernel; the
//              relabel kernel is the only one that writes rows / cols and runs last -- in place is safe by KERNEL order.
// The chase is capped at n_hops steps, every parent must be smaller than its child and every edge index below m: a batch
// that breaks the forest contract gets group 0 for the position, nothing is read or written outside the batch's slabs.
#include <algorithm>

#include "ns_unique.h"

namespace tg {

struct NsgArgs {
    const int64_t *samples, *rows, *cols, *layer_offsets, *counts; // batch 0 of the round
    const int32_t *seed_group;                                     // [n_seeds] or null: the identity
    int64_t *nodes, *group, *inverse, *rows_u, *cols_u, *counts_u, *layer_nodes;
    int64_t cap_nodes, cap_edges, n_batches, n_seeds;
    uint64_t key_mul;                                              // id_bound: key = group * key_mul + id
    int32_t n_hops;
    uint32_t cap_mask, hash_shift;
    // flat form: the round's tables
    unsigned char *ws;
    int64_t batch_bytes, vals_off, slot_off, tile_off, grp_off;
    int32_t n_node_tiles, inv_tiles;
};

// the group of position p < n of a batch with m edges; 0 where the batch breaks the forest contract
__device__ __forceinline__ uint32_t nsg_group_of(const NsgArgs &a, const int64_t *cols, int64_t p, int64_t m) {
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

template <typename K> __device__ __forceinline__ K nsg_key(const NsgArgs &a, uint32_t g, int64_t id) {
    return (K)g * (K)a.key_mul + (K)id;
}

// ---- LDS form ------------------------------------------------------------------------------------------------------------
template <typename K> __global__ void __launch_bounds__(NSU_THREADS) nsg_lds_kernel(const NsgArgs a) {
    extern __shared__ __align__(16) unsigned char nsg_lds[];
    __shared__ uint32_t s_wave[NSU_THREADS / 64];
    const uint32_t cap = a.cap_mask + 1;
    K *keys = reinterpret_cast<K *>(nsg_lds);
    uint32_t *vals = reinterpret_cast<uint32_t *>(keys + cap);
    uint16_t *loc = reinterpret_cast<uint16_t *>(vals + cap);  // [cap_nodes]: the position's slot, later its local id
    uint16_t *grp = loc + ((a.cap_nodes + 7) & ~(int64_t)7);   // [cap_nodes]: the position's group
    const int tid = threadIdx.x, nt = blockDim.x;

    for (int64_t b = blockIdx.x; b < a.n_batches; b += gridDim.x) {
        const int n = (int)nsu_clamp(a.counts[b * 2], a.cap_nodes);
        const int64_t m = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
        const int64_t *samples = a.samples + b * a.cap_nodes;
        const int64_t *rows = a.rows + b * a.cap_edges, *cols = a.cols + b * a.cap_edges;
        for (uint32_t s = tid; s < cap; s += nt) {
            keys[s] = nsu_empty<K>();
            vals[s] = NSU_UNSEEN;
        }
        __syncthreads(); // also: the previous batch is done with `loc` and `grp`
        for (int p = tid; p < n; p += nt) {
            const uint32_t g = nsg_group_of(a, cols, p, m);
            const uint32_t s = nsu_insert<K>(keys, a.cap_mask, a.hash_shift, nsg_key<K>(a, g, samples[p]));
            atomicMin(&vals[s], (uint32_t)p);
            loc[p] = (uint16_t)s;
            grp[p] = (uint16_t)g;
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
        int64_t *nodes = a.nodes + b * a.cap_nodes, *group = a.group + b * a.cap_nodes;
        uint32_t rank = rank0;
        for (uint32_t f = first; f;) {
            const int p = p0 + __ffs(f) - 1;
            f &= f - 1;
            vals[loc[p]] = rank;
            group[rank] = (int64_t)grp[p];
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
template <typename K> struct NsgBatch {
    K *keys;
    uint32_t *vals, *slot, *tile_cnt, *grp;
    __device__ __forceinline__ NsgBatch(const NsgArgs &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        keys = reinterpret_cast<K *>(base);
        vals = reinterpret_cast<uint32_t *>(base + a.vals_off);
        slot = reinterpret_cast<uint32_t *>(base + a.slot_off);
        tile_cnt = reinterpret_cast<uint32_t *>(base + a.tile_off);
        grp = reinterpret_cast<uint32_t *>(base + a.grp_off);
    }
};

template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsg_clear_kernel(const NsgArgs a) {
    const NsgBatch<K> t(a, blockIdx.y);
    const uint32_t cap = a.cap_mask + 1;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += gridDim.x * blockDim.x) {
        t.keys[s] = nsu_empty<K>();
        t.vals[s] = NSU_UNSEEN;
    }
}

// the chase, the group word and the insert of a tile of positions; reads the input cols, writes none
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsg_insert_kernel(const NsgArgs a) {
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n) return;
    const int64_t m = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
    const NsgBatch<K> t(a, b);
    const int64_t *samples = a.samples + b * a.cap_nodes, *cols = a.cols + b * a.cap_edges;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (p < n) {
            const uint32_t g = nsg_group_of(a, cols, p, m);
            const uint32_t s = nsu_insert<K>(t.keys, a.cap_mask, a.hash_shift, nsg_key<K>(a, g, samples[p]));
            atomicMin(&t.vals[s], (uint32_t)p);
            t.slot[p] = s;
            t.grp[p] = g;
        }
    }
}

// flags the first occurrences of a tile in their slot words and counts them
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsg_flag_kernel(const NsgArgs a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsgBatch<K> t(a, b);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = p0 + k;
        if (p < n) {
            const uint32_t s = t.slot[p];
            if (t.vals[s] == (uint32_t)p) {
                t.slot[p] = s | NSU_FLAG;
                ++cnt;
            }
        }
    }
    uint32_t total;
    nsu_scan(cnt, s_wave, &total);
    if (threadIdx.x == 0) t.tile_cnt[blockIdx.x] = total;
}

// names the first occurrences of a tile: local id = first occurrences in the tiles before it + the scan inside it
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsg_apply_kernel(const NsgArgs a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsgBatch<K> t(a, b);
    uint32_t before = 0, base;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += NSU_TILE_THREADS) before += t.tile_cnt[i];
    nsu_scan(before, s_wave, &base);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    uint32_t first = 0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k)
        if (p0 + k < n && (t.slot[p0 + k] & NSU_FLAG)) first |= 1u << k;
    uint32_t total;
    const uint32_t rank0 = base + nsu_scan((uint32_t)__popc(first), s_wave, &total);
    const int64_t *samples = a.samples + b * a.cap_nodes;
    int64_t *nodes = a.nodes + b * a.cap_nodes, *group = a.group + b * a.cap_nodes;
    uint32_t rank = rank0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        if (first & (1u << k)) {
            t.vals[t.slot[p0 + k] & ~NSU_FLAG] = rank;
            group[rank] = (int64_t)t.grp[p0 + k];
            nodes[rank++] = samples[p0 + k];
        }
    }
    const bool last = tile0 + NSU_TILE >= n; // the batch's last tile (tile 0 of an empty batch)
    if (a.layer_nodes) {
        for (int h = 0; h < a.n_hops; ++h) {
            const int64_t L = nsu_clamp(a.layer_offsets[(b * a.n_hops + h) * 3], n);
            if (L >= n) {
                if (last && threadIdx.x == 0) a.layer_nodes[b * a.n_hops + h] = (int64_t)(base + total);
            } else if (L >= p0 && L < p0 + NSU_PER) {
                a.layer_nodes[b * a.n_hops + h] = (int64_t)(rank0 + __popc(first & ((1u << (int)(L - p0)) - 1u)));
            }
        }
    }
    if (last && threadIdx.x == 0) {
        a.counts_u[b * 2] = (int64_t)(base + total);
        a.counts_u[b * 2 + 1] = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
    }
}

// blocks [0, inv_tiles): inverse of a tile of positions; the others: a tile of edges.  The only kernel that writes rows /
// cols, and the last one: every chase is over
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsg_relabel_kernel(const NsgArgs a) {
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const NsgBatch<K> t(a, b);
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

// ---- host side ---------------------------------------------------------------------------------------------------------------
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

template <typename K> static int nsg_launch_lds(const NsgArgs &a, const NsgPlan &pl, hipStream_t stream) {
    const int64_t dyn = pl.u.lds_bytes - NSU_STATIC_LDS;
    if (dyn > 64 * 1024) { // above the default limit of a launch: raise it once per device (the plan keeps it below the device's)
        static std::atomic<int64_t> raised[64]; // zero-initialised; a race only sets the attribute twice
        int dev = 0;
        TG_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || raised[dev] < dyn) {
            TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nsg_lds_kernel<K>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
            if (dev >= 0 && dev < 64) raised[dev] = dyn;
        }
    }
    const unsigned grid = (unsigned)(a.n_batches < 16384 ? a.n_batches : 16384);
    hipLaunchKernelGGL(nsg_lds_kernel<K>, dim3(grid), dim3(pl.u.threads), (size_t)dyn, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <typename K> static int nsg_launch_flat(const NsgArgs &a, const NsgPlan &pl, hipStream_t stream) {
    const unsigned nb = (unsigned)a.n_batches, tiles = (unsigned)pl.u.n_node_tiles;
    const dim3 block(NSU_TILE_THREADS);
    const int64_t clear_blocks = (pl.u.table_cap + NSU_TILE_THREADS - 1) / NSU_TILE_THREADS;
    hipLaunchKernelGGL(nsg_clear_kernel<K>, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024), nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsg_insert_kernel<K>, dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsg_flag_kernel<K>, dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsg_apply_kernel<K>, dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    const int64_t edge_tiles = (a.cap_edges + NSU_EDGE_TILE - 1) / NSU_EDGE_TILE;
    if (a.inv_tiles + edge_tiles > 0) {
        hipLaunchKernelGGL(nsg_relabel_kernel<K>, dim3((unsigned)(a.inv_tiles + edge_tiles), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
    }
    return TG_OK;
}

} // namespace tg

extern "C" int tg_ns_homo_unique_grouped_form(int64_t cap_nodes, int64_t id_bound, int64_t n_groups, int64_t lds_limit_bytes,
                                              int32_t *form, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_grouped_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    NsgPlan pl;
    if (const int rc = nsg_plan(cap_nodes, id_bound, n_groups, who, pl)) return rc;
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : nsu_device_lds_limit();
    *form = nsu_fits(pl.u, limit) ? 1 : 2;
    *lds_bytes = pl.u.lds_bytes;
    return TG_OK;
}

extern "C" int tg_ns_homo_unique_grouped_workspace_bytes(int64_t cap_nodes, int64_t id_bound, int64_t n_groups,
                                                         int64_t n_batches, int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_grouped_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    NsgPlan pl;
    if (const int rc = nsg_plan(cap_nodes, id_bound, n_groups, who, pl)) return rc;
    *bytes_min = pl.u.batch_bytes;
    *bytes = nsu_fits(pl.u, nsu_device_lds_limit()) ? 0 : pl.u.batch_bytes * n_batches;
    return TG_OK;
}

extern "C" int tg_ns_homo_unique_grouped(const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops,
                                         int64_t id_bound, const int32_t *seed_group, int64_t n_groups,
                                         const tg_ns_unique_grouped_out *out, void *workspace, int64_t workspace_bytes,
                                         int32_t form, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_grouped";
    TG_REQUIRE(in && out, "%s: null argument", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(n_seeds >= 0, "%s: n_seeds = %lld is negative", who, (long long)n_seeds);
    TG_REQUIRE(n_hops >= 0 && n_hops <= TG_MAX_HOPS, "%s: n_hops = %d outside [0, %d]", who, n_hops, TG_MAX_HOPS);
    TG_REQUIRE(in->cap_edges >= 0, "%s: cap_edges = %lld is negative", who, (long long)in->cap_edges);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    NsgPlan pl;
    if (const int rc = nsg_plan(in->cap_nodes, id_bound, n_groups, who, pl)) return rc;
    TG_REQUIRE(seed_group || n_groups == n_seeds, "%s: n_groups = %lld without a seed_group map: the identity has n_seeds = %lld groups",
               who, (long long)n_groups, (long long)n_seeds);
    TG_REQUIRE(n_seeds <= in->cap_nodes, "%s: n_seeds = %lld above cap_nodes = %lld", who, (long long)n_seeds,
               (long long)in->cap_nodes);
    const bool fits = form != 2 && nsu_fits(pl.u, nsu_device_lds_limit());
    TG_REQUIRE(form != 1 || fits, "%s: form 1: a table of %lld slots (%lld bytes of LDS, %lld groups) does not fit a workgroup", who,
               (long long)pl.u.table_cap, (long long)pl.u.lds_bytes, (long long)n_groups);
    const bool lds = form != 2 && fits;
    if (!lds)
        TG_REQUIRE(workspace && workspace_bytes >= pl.u.batch_bytes, "%s: workspace too small (%lld < %lld, the size of one batch)",
                   who, (long long)(workspace ? workspace_bytes : 0), (long long)pl.u.batch_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    if (n_batches == 0) return TG_OK;
    // device pointers
    TG_REQUIRE(in->samples && in->counts && out->nodes && out->group && out->counts, "%s: null samples / counts / nodes / group", who);
    TG_REQUIRE(in->cap_edges == 0 || (in->rows && in->cols && out->rows && out->cols), "%s: null edge slab", who);
    TG_REQUIRE(n_hops == 0 || !out->layer_nodes || in->layer_offsets, "%s: layer_nodes asked for without layer_offsets (null)", who);
    hipStream_t stream = (hipStream_t)stream_;

    const int64_t round = lds ? n_batches : std::min(std::min(workspace_bytes / pl.u.batch_bytes, NSU_ROUND_MAX), n_batches);
    for (int64_t b0 = 0; b0 < n_batches; b0 += round) {
        NsgArgs a{};
        a.samples = in->samples + b0 * in->cap_nodes, a.counts = in->counts + b0 * 2;
        a.rows = in->rows ? in->rows + b0 * in->cap_edges : nullptr, a.cols = in->cols ? in->cols + b0 * in->cap_edges : nullptr;
        a.layer_offsets = in->layer_offsets ? in->layer_offsets + b0 * n_hops * 3 : nullptr;
        a.seed_group = seed_group;
        a.nodes = out->nodes + b0 * in->cap_nodes, a.group = out->group + b0 * in->cap_nodes, a.counts_u = out->counts + b0 * 2;
        a.inverse = out->inverse ? out->inverse + b0 * in->cap_nodes : nullptr;
        a.rows_u = out->rows ? out->rows + b0 * in->cap_edges : nullptr;
        a.cols_u = out->cols ? out->cols + b0 * in->cap_edges : nullptr;
        a.layer_nodes = out->layer_nodes ? out->layer_nodes + b0 * n_hops : nullptr;
        a.cap_nodes = in->cap_nodes, a.cap_edges = in->cap_edges, a.n_hops = n_hops, a.n_seeds = n_seeds;
        a.key_mul = (uint64_t)id_bound;
        a.n_batches = std::min(round, n_batches - b0);
        a.cap_mask = (uint32_t)(pl.u.table_cap - 1);
        a.hash_shift = 32u - (uint32_t)__builtin_ctzll((unsigned long long)pl.u.table_cap);
        a.ws = static_cast<unsigned char *>(workspace);
        a.batch_bytes = pl.u.batch_bytes, a.vals_off = pl.u.vals_off, a.slot_off = pl.u.slot_off, a.tile_off = pl.u.tile_off;
        a.grp_off = pl.grp_off;
        a.n_node_tiles = (int32_t)pl.u.n_node_tiles, a.inv_tiles = a.inverse ? (int32_t)pl.u.n_node_tiles : 0;
        int rc;
        if (lds)
            rc = pl.u.key_bytes == 4 ? nsg_launch_lds<nsu_k32>(a, pl, stream) : nsg_launch_lds<nsu_k64>(a, pl, stream);
        else
            rc = pl.u.key_bytes == 4 ? nsg_launch_flat<nsu_k32>(a, pl, stream) : nsg_launch_flat<nsu_k64>(a, pl, stream);
        if (rc) return rc;
    }
    return TG_OK;
}
