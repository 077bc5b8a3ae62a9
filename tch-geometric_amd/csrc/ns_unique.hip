// Per-batch node dedup and relabel of the tg_ns_homo_batched slabs (tg_ns_homo_unique, include/tchgeo.h).
//
// The rule, per batch: nodes = the distinct values of samples[:n] in order of FIRST occurrence, inverse[p] = index of
// samples[p] in nodes, rows / cols = inverse[rows], inverse[cols].  Both forms compute it the same way:
//   1. an open-addressing table (tg_map.h / negative_batched.inl): the key is claimed with atomicCAS, then atomicMin of
//      the position into the slot's value -- the value ends as the id's first position whatever order lanes arrive in;
//   2. position p is a first occurrence iff value[slot(p)] == p; local ids are the exclusive scan of those flags in
//      position order, written back into the slot's value;
//   3. inverse[p] = value[slot(p)], edges go through it.
// layer_nodes[h] is the scan's value at position layer_offsets[h][0].
//
// LDS form: ONE workgroup runs ONE batch; keys, values and a u16 word per position (the slot, later the local id) live in
//   LDS, so only the slab reads and the output stores touch global memory.  A table of cap = 2^k >= 4/3 cap_nodes slots
//   (load factor <= 0.75) of (key, u32 value) must fit: cap_nodes <= 12 288 with 32-bit keys in 160 KiB, 6 144 with 64-bit.
// Flat form: the loader's shape (1 024 x [15,10]: 169 984 positions, 16 batches) fits no LDS and has too few batches to
//   fill the device batch by batch, so the grid runs over POSITIONS of all batches: clear | insert | flag + tile counts |
//   apply (a block sums the counts of the tiles before its own, scans its tile, names the first occurrences) | relabel.
//   Tables, the per-position slot words and the tile counts of a batch sit in the workspace.
// Every probe loop is capped at the table size: an id outside [0, id_bound) ends it instead of spinning.
#include <algorithm>

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

// ---- LDS form ------------------------------------------------------------------------------------------------------------
template <typename K> __global__ void __launch_bounds__(NSU_THREADS) nsu_lds_kernel(const NsuArgs a) {
    extern __shared__ __align__(16) unsigned char nsu_lds[];
    __shared__ uint32_t s_wave[NSU_THREADS / 64];
    const uint32_t cap = a.cap_mask + 1;
    K *keys = reinterpret_cast<K *>(nsu_lds);
    uint32_t *vals = reinterpret_cast<uint32_t *>(keys + cap);
    uint16_t *loc = reinterpret_cast<uint16_t *>(vals + cap); // [cap_nodes]: the position's slot, later its local id
    const int tid = threadIdx.x, nt = blockDim.x;

    for (int64_t b = blockIdx.x; b < a.n_batches; b += gridDim.x) {
        const int n = (int)nsu_clamp(a.counts[b * 2], a.cap_nodes);
        const int64_t m = nsu_clamp(a.counts[b * 2 + 1], a.cap_edges);
        const int64_t *samples = a.samples + b * a.cap_nodes;
        for (uint32_t s = tid; s < cap; s += nt) {
            keys[s] = nsu_empty<K>();
            vals[s] = NSU_UNSEEN;
        }
        __syncthreads(); // also: the previous batch is done with `loc`
        for (int p = tid; p < n; p += nt) {
            const uint32_t s = nsu_insert<K>(keys, a.cap_mask, a.hash_shift, (K)samples[p]);
            atomicMin(&vals[s], (uint32_t)p);
            loc[p] = (uint16_t)s;
        }
        __syncthreads();
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
template <typename K> struct NsuBatch {
    K *keys;
    uint32_t *vals, *slot, *tile_cnt;
    __device__ __forceinline__ NsuBatch(const NsuArgs &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        keys = reinterpret_cast<K *>(base);
        vals = reinterpret_cast<uint32_t *>(base + a.vals_off);
        slot = reinterpret_cast<uint32_t *>(base + a.slot_off);
        tile_cnt = reinterpret_cast<uint32_t *>(base + a.tile_off);
    }
};

template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_clear_kernel(const NsuArgs a) {
    const NsuBatch<K> t(a, blockIdx.y);
    const uint32_t cap = a.cap_mask + 1;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += gridDim.x * blockDim.x) {
        t.keys[s] = nsu_empty<K>();
        t.vals[s] = NSU_UNSEEN;
    }
}

template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_insert_kernel(const NsuArgs a) {
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n) return;
    const NsuBatch<K> t(a, b);
    const int64_t *samples = a.samples + b * a.cap_nodes;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (p < n) {
            const uint32_t s = nsu_insert<K>(t.keys, a.cap_mask, a.hash_shift, (K)samples[p]);
            atomicMin(&t.vals[s], (uint32_t)p);
            t.slot[p] = s;
        }
    }
}

// flags the first occurrences of a tile in their slot words and counts them
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_flag_kernel(const NsuArgs a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsuBatch<K> t(a, b);
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
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_apply_kernel(const NsuArgs a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsuBatch<K> t(a, b);
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
    int64_t *nodes = a.nodes + b * a.cap_nodes;
    uint32_t rank = rank0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        if (first & (1u << k)) {
            t.vals[t.slot[p0 + k] & ~NSU_FLAG] = rank;
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

// blocks [0, inv_tiles): inverse of a tile of positions; the others: a tile of edges
template <typename K> __global__ void __launch_bounds__(NSU_TILE_THREADS) nsu_relabel_kernel(const NsuArgs a) {
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * 2], a.cap_nodes);
    const NsuBatch<K> t(a, b);
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
template <typename K> static int nsu_launch_lds(const NsuArgs &a, const NsuPlan &pl, hipStream_t stream) {
    const int64_t dyn = pl.lds_bytes - NSU_STATIC_LDS;
    if (dyn > 64 * 1024) { // above the default limit of a launch: raise it once per device (the plan keeps it below the device's)
        static std::atomic<int64_t> raised[64]; // zero-initialised; a race only sets the attribute twice
        int dev = 0;
        TG_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || raised[dev] < dyn) {
            TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nsu_lds_kernel<K>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
            if (dev >= 0 && dev < 64) raised[dev] = dyn;
        }
    }
    const unsigned grid = (unsigned)(a.n_batches < 16384 ? a.n_batches : 16384);
    hipLaunchKernelGGL(nsu_lds_kernel<K>, dim3(grid), dim3(pl.threads), (size_t)dyn, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <typename K> static int nsu_launch_flat(const NsuArgs &a, const NsuPlan &pl, hipStream_t stream) {
    const unsigned nb = (unsigned)a.n_batches, tiles = (unsigned)pl.n_node_tiles;
    const dim3 block(NSU_TILE_THREADS);
    const int64_t clear_blocks = (pl.table_cap + NSU_TILE_THREADS - 1) / NSU_TILE_THREADS;
    hipLaunchKernelGGL(nsu_clear_kernel<K>, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024), nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsu_insert_kernel<K>, dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsu_flag_kernel<K>, dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsu_apply_kernel<K>, dim3(tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    const int64_t edge_tiles = (a.cap_edges + NSU_EDGE_TILE - 1) / NSU_EDGE_TILE;
    if (a.inv_tiles + edge_tiles > 0) {
        hipLaunchKernelGGL(nsu_relabel_kernel<K>, dim3((unsigned)(a.inv_tiles + edge_tiles), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
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
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : nsu_device_lds_limit();
    *form = nsu_fits(pl, limit) ? 1 : 2;
    *lds_bytes = pl.lds_bytes;
    return TG_OK;
}

extern "C" int tg_ns_homo_unique_workspace_bytes(int64_t cap_nodes, int64_t id_bound, int64_t n_batches, int64_t *bytes,
                                                 int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    NsuPlan pl;
    if (const int rc = nsu_plan(cap_nodes, id_bound, who, pl)) return rc;
    *bytes_min = pl.batch_bytes;
    *bytes = nsu_fits(pl, nsu_device_lds_limit()) ? 0 : pl.batch_bytes * n_batches;
    return TG_OK;
}

extern "C" int tg_ns_homo_unique(const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops, int64_t id_bound,
                                 const tg_ns_unique_out *out, void *workspace, int64_t workspace_bytes, int32_t form,
                                 void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_homo_unique";
    TG_REQUIRE(in && out, "%s: null argument", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(n_seeds >= 0, "%s: n_seeds = %lld is negative", who, (long long)n_seeds);
    TG_REQUIRE(n_hops >= 0 && n_hops <= TG_MAX_HOPS, "%s: n_hops = %d outside [0, %d]", who, n_hops, TG_MAX_HOPS);
    TG_REQUIRE(in->cap_edges >= 0, "%s: cap_edges = %lld is negative", who, (long long)in->cap_edges);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    NsuPlan pl;
    if (const int rc = nsu_plan(in->cap_nodes, id_bound, who, pl)) return rc;
    TG_REQUIRE(n_seeds <= in->cap_nodes, "%s: n_seeds = %lld above cap_nodes = %lld", who, (long long)n_seeds,
               (long long)in->cap_nodes);
    const bool fits = form != 2 && nsu_fits(pl, nsu_device_lds_limit());
    TG_REQUIRE(form != 1 || fits, "%s: form 1: a table of %lld slots (%lld bytes of LDS) does not fit a workgroup", who,
               (long long)pl.table_cap, (long long)pl.lds_bytes);
    const bool lds = form != 2 && fits;
    if (!lds)
        TG_REQUIRE(workspace && workspace_bytes >= pl.batch_bytes, "%s: workspace too small (%lld < %lld, the size of one batch)",
                   who, (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    if (n_batches == 0) return TG_OK;
    // device pointers
    TG_REQUIRE(in->samples && in->counts && out->nodes && out->counts, "%s: null samples / counts / nodes", who);
    TG_REQUIRE(in->cap_edges == 0 || (in->rows && in->cols && out->rows && out->cols), "%s: null edge slab", who);
    TG_REQUIRE(n_hops == 0 || !out->layer_nodes || in->layer_offsets, "%s: layer_nodes asked for without layer_offsets (null)", who);
    hipStream_t stream = (hipStream_t)stream_;

    const int64_t round = lds ? n_batches : std::min(std::min(workspace_bytes / pl.batch_bytes, NSU_ROUND_MAX), n_batches);
    for (int64_t b0 = 0; b0 < n_batches; b0 += round) {
        NsuArgs a{};
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
        a.cap_mask = (uint32_t)(pl.table_cap - 1);
        a.hash_shift = 32u - (uint32_t)__builtin_ctzll((unsigned long long)pl.table_cap);
        a.ws = static_cast<unsigned char *>(workspace);
        a.batch_bytes = pl.batch_bytes, a.vals_off = pl.vals_off, a.slot_off = pl.slot_off, a.tile_off = pl.tile_off;
        a.n_node_tiles = (int32_t)pl.n_node_tiles, a.inv_tiles = a.inverse ? (int32_t)pl.n_node_tiles : 0;
        int rc;
        if (lds)
            rc = pl.key_bytes == 4 ? nsu_launch_lds<nsu_k32>(a, pl, stream) : nsu_launch_lds<nsu_k64>(a, pl, stream);
        else
            rc = pl.key_bytes == 4 ? nsu_launch_flat<nsu_k32>(a, pl, stream) : nsu_launch_flat<nsu_k64>(a, pl, stream);
        if (rc) return rc;
    }
    return TG_OK;
}
