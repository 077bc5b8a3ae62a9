// Per-batch, per-type node dedup and relabel of the typed slabs of tg_ns_hetero_batched (tg_ns_typed_unique,
// include/tchgeo.h): ns_unique.hip with a type dimension.  The insert, the scan, the LDS-limit raise and the flat form's clear,
// flag and apply tile bodies are ns_unique.h's; the kernel shells, their grids over (tile, batch, type) and NstArgs are this file's.
//
// The rule, per batch b and node type t: nodes[t] = the distinct values of samples[t][:n] in order of FIRST occurrence,
// inverse[t][p] = index of samples[t][p] in nodes[t]; per relation r: rows = inverse[rel_src[r]][rows], cols =
// inverse[rel_dst[r]][cols].  A type is deduplicated exactly as ns_unique.hip does it (atomicCAS claims the key, atomicMin
// leaves the first position, first occurrences are ranked by a scan in position order); what is new is that a relation's two
// ends go through the maps of two types (the same one twice for a self-relation).
//
// LDS form: ONE workgroup runs ONE batch.  It goes through the types one after the other with one table area sized for the
//   type that needs most (table_cap[t] * (key bytes[t] + 4); a type's table is 2^k >= 4/3 pitch[t] slots, its keys 32- or
//   64-bit by its own id_bound), and keeps a u16 word per position of EVERY type behind it (first the slot, then the local
//   id).  When the last type is done the relabel of every relation reads only those words and the edge slabs.
// Flat form: grids over (tile of positions, batch, type); a batch has one table, one slot word per position and one count
//   per tile for every type in the workspace: clear | insert | flag + tile counts | apply (names the first occurrences) |
//   inverse (where asked for) | edges, gridded over (tile of edges, batch, relation).
// Every probe loop is capped at the table size: an id outside [0, id_bound) ends it instead of spinning.
#include <algorithm>

#include "ns_unique.h"

namespace tg {

struct NstType {
    const int64_t *samples; // batch 0 of the round
    int64_t *nodes, *inverse;
    int64_t pitch, n_inputs;
    int64_t keys_off, vals_off, slot_off, tile_off; // flat form: inside a batch's part of the workspace
    uint32_t cap_mask, hash_shift;
    int32_t n_tiles, key64;
    uint32_t loc_off, pad_; // LDS form: the type's first word in the u16 area
};
struct NstRel {
    const int64_t *rows, *cols; // batch 0 of the round
    int64_t *rows_u, *cols_u;
    int64_t pitch;
    int32_t src, dst;
};
struct NstArgs {
    NstType t[TG_HET_MAX_TYPES];
    NstRel r[TG_HET_MAX_RELS];
    const int64_t *counts; // batch 0 of the round
    int64_t *counts_u, *seed_counts;
    int64_t counts_stride, n_batches, batch_bytes;
    unsigned char *ws;
    int32_t n_types, n_rels;
    uint32_t loc_base, pad_; // LDS form: bytes of the table area, the u16 area starts behind it
};

__device__ __forceinline__ int64_t nst_seed_bound(const NstType &ty, int64_t n) { return nsu_clamp(ty.n_inputs, n); }

// ---- LDS form ------------------------------------------------------------------------------------------------------------
// one type of one batch: on return loc[p] is the local id of position p < n (not yet visible: the caller's barrier)
template <typename K>
__device__ __forceinline__ void nst_lds_type(const NstArgs &a, const NstType &ty, int t, int64_t b, unsigned char *table,
                                             uint16_t *loc, uint32_t *s_wave) {
    const uint32_t cap = ty.cap_mask + 1;
    K *keys = reinterpret_cast<K *>(table);
    uint32_t *vals = reinterpret_cast<uint32_t *>(keys + cap);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = (int)nsu_clamp(a.counts[b * a.counts_stride + t], ty.pitch);
    const int64_t *samples = ty.samples + b * ty.pitch;
    for (uint32_t s = tid; s < cap; s += nt) {
        keys[s] = nsu_empty<K>();
        vals[s] = NSU_UNSEEN;
    }
    __syncthreads();
    for (int p = tid; p < n; p += nt) {
        const uint32_t s = nsu_insert<K>(keys, ty.cap_mask, ty.hash_shift, (K)samples[p]);
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
    int64_t *nodes = ty.nodes + b * ty.pitch;
    uint32_t rank = rank0;
    for (uint32_t f = first; f;) {
        const int p = p0 + __ffs(f) - 1;
        f &= f - 1;
        vals[loc[p]] = rank;
        nodes[rank++] = samples[p];
    }
    if (a.seed_counts) {
        const int L = (int)nst_seed_bound(ty, n);
        if (L >= n) {
            if (tid == 0) a.seed_counts[b * a.n_types + t] = (int64_t)n_unique;
        } else if (L >= p0 && L < p1) {
            a.seed_counts[b * a.n_types + t] = (int64_t)(rank0 + __popc(first & ((1u << (L - p0)) - 1u)));
        }
    }
    if (tid == 0) a.counts_u[b * a.counts_stride + t] = (int64_t)n_unique;
    __syncthreads();
    int64_t *inverse = ty.inverse ? ty.inverse + b * ty.pitch : nullptr;
    for (int p = tid; p < n; p += nt) {
        const uint32_t id = vals[loc[p]];
        loc[p] = (uint16_t)id;
        if (inverse) inverse[p] = (int64_t)id;
    }
    __syncthreads(); // the next type clears the table; the edges read loc
}

__global__ void __launch_bounds__(NSU_THREADS) nst_lds_kernel(const NstArgs a) {
    extern __shared__ __align__(16) unsigned char nst_lds[];
    __shared__ uint32_t s_wave[NSU_THREADS / 64];
    uint16_t *loc_all = reinterpret_cast<uint16_t *>(nst_lds + a.loc_base);
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int64_t b = blockIdx.x; b < a.n_batches; b += gridDim.x) {
        for (int t = 0; t < a.n_types; ++t) {
            const NstType &ty = a.t[t];
            if (ty.key64)
                nst_lds_type<nsu_k64>(a, ty, t, b, nst_lds, loc_all + ty.loc_off, s_wave);
            else
                nst_lds_type<nsu_k32>(a, ty, t, b, nst_lds, loc_all + ty.loc_off, s_wave);
        }
        for (int r = 0; r < a.n_rels; ++r) {
            const NstRel &re = a.r[r];
            const NstType &ts = a.t[re.src], &td = a.t[re.dst];
            const int64_t m = nsu_clamp(a.counts[b * a.counts_stride + a.n_types + r], re.pitch);
            const int64_t n_src = nsu_clamp(a.counts[b * a.counts_stride + re.src], ts.pitch);
            const int64_t n_dst = nsu_clamp(a.counts[b * a.counts_stride + re.dst], td.pitch);
            const uint16_t *loc_s = loc_all + ts.loc_off, *loc_d = loc_all + td.loc_off;
            const int64_t *rows = re.rows + b * re.pitch, *cols = re.cols + b * re.pitch;
            int64_t *rows_u = re.rows_u + b * re.pitch, *cols_u = re.cols_u + b * re.pitch;
            if (tid == 0) a.counts_u[b * a.counts_stride + a.n_types + r] = m;
            for (int64_t e = tid; e < m; e += nt) { // element e is read before it is written: in place is fine
                const int64_t rr = rows[e], cc = cols[e];
                rows_u[e] = nsu_end(rr, n_src, [&](int64_t p) { return loc_s[p]; });
                cols_u[e] = nsu_end(cc, n_dst, [&](int64_t p) { return loc_d[p]; });
            }
        }
        __syncthreads(); // the next batch overwrites loc
    }
}

// ---- flat form -------------------------------------------------------------------------------------------------------------
template <typename K> struct NstTable {
    K *keys;
    uint32_t *vals, *slot, *tile_cnt;
    __device__ __forceinline__ NstTable(const NstArgs &a, const NstType &ty, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        keys = reinterpret_cast<K *>(base + ty.keys_off);
        vals = reinterpret_cast<uint32_t *>(base + ty.vals_off);
        slot = reinterpret_cast<uint32_t *>(base + ty.slot_off);
        tile_cnt = reinterpret_cast<uint32_t *>(base + ty.tile_off);
    }
};
// vals / slot / tile_cnt do not depend on the key width: the kernels behind the insert read them through this
typedef NstTable<nsu_k32> NstWords;

template <typename K> __device__ __forceinline__ void nst_clear(const NstArgs &a, const NstType &ty, int64_t b) {
    const NstTable<K> tb(a, ty, b);
    nsu_clear_tile<K>(tb.keys, tb.vals, ty.cap_mask + 1, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
__global__ void __launch_bounds__(NSU_TILE_THREADS) nst_clear_kernel(const NstArgs a) {
    const NstType &ty = a.t[blockIdx.z];
    if (ty.key64)
        nst_clear<nsu_k64>(a, ty, blockIdx.y);
    else
        nst_clear<nsu_k32>(a, ty, blockIdx.y);
}

template <typename K>
__device__ __forceinline__ void nst_insert(const NstArgs &a, const NstType &ty, int64_t b, int64_t n, int64_t tile0) {
    const NstTable<K> tb(a, ty, b);
    const int64_t *samples = ty.samples + b * ty.pitch;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (p < n) {
            const uint32_t s = nsu_insert<K>(tb.keys, ty.cap_mask, ty.hash_shift, (K)samples[p]);
            atomicMin(&tb.vals[s], (uint32_t)p);
            tb.slot[p] = s;
        }
    }
}
__global__ void __launch_bounds__(NSU_TILE_THREADS) nst_insert_kernel(const NstArgs a) {
    const int t = blockIdx.z;
    const NstType &ty = a.t[t];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride + t], ty.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n) return;
    if (ty.key64)
        nst_insert<nsu_k64>(a, ty, b, n, tile0);
    else
        nst_insert<nsu_k32>(a, ty, b, n, tile0);
}

// flags the first occurrences of a tile in their slot words and counts them
__global__ void __launch_bounds__(NSU_TILE_THREADS) nst_flag_kernel(const NstArgs a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int t = blockIdx.z;
    const NstType &ty = a.t[t];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride + t], ty.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if ((int)blockIdx.x >= ty.n_tiles || (tile0 >= n && blockIdx.x != 0)) return; // uniform
    nsu_flag_tile(NstWords(a, ty, b), n, tile0, s_wave);
}

// names the first occurrences of a tile: local id = first occurrences in the tiles before it + the scan inside it
__global__ void __launch_bounds__(NSU_TILE_THREADS) nst_apply_kernel(const NstArgs a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int t = blockIdx.z;
    const NstType &ty = a.t[t];
    const int64_t b = blockIdx.y;
    if (t == 0 && blockIdx.x == 0 && (int)threadIdx.x < a.n_rels) // the edge counts of the batch: clamped copies
        a.counts_u[b * a.counts_stride + a.n_types + threadIdx.x] =
            nsu_clamp(a.counts[b * a.counts_stride + a.n_types + threadIdx.x], a.r[threadIdx.x].pitch);
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride + t], ty.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if ((int)blockIdx.x >= ty.n_tiles || (tile0 >= n && blockIdx.x != 0)) return; // uniform
    const NsuRanks r = nsu_apply_tile(NstWords(a, ty, b), n, tile0, ty.samples + b * ty.pitch, ty.nodes + b * ty.pitch, s_wave,
                                      [](uint32_t, int64_t) {});
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    const bool last = tile0 + NSU_TILE >= n; // the type's last tile in this batch (tile 0 of an empty list)
    if (a.seed_counts) {
        const int64_t L = nst_seed_bound(ty, n);
        if (L >= n) {
            if (last && threadIdx.x == 0) a.seed_counts[b * a.n_types + t] = (int64_t)(r.base + r.total);
        } else if (L >= p0 && L < p0 + NSU_PER) {
            a.seed_counts[b * a.n_types + t] = (int64_t)(r.rank0 + __popc(r.first & ((1u << (int)(L - p0)) - 1u)));
        }
    }
    if (last && threadIdx.x == 0) a.counts_u[b * a.counts_stride + t] = (int64_t)(r.base + r.total);
}

__global__ void __launch_bounds__(NSU_TILE_THREADS) nst_inverse_kernel(const NstArgs a) {
    const int t = blockIdx.z;
    const NstType &ty = a.t[t];
    if (!ty.inverse) return;
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride + t], ty.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    if (tile0 >= n) return;
    const NstWords tb(a, ty, b);
    int64_t *inverse = ty.inverse + b * ty.pitch;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (p < n) inverse[p] = (int64_t)tb.vals[tb.slot[p] & ~NSU_FLAG];
    }
}

__global__ void __launch_bounds__(NSU_TILE_THREADS) nst_edges_kernel(const NstArgs a) {
    const int r = blockIdx.z;
    const NstRel &re = a.r[r];
    const int64_t b = blockIdx.y;
    const int64_t m = nsu_clamp(a.counts[b * a.counts_stride + a.n_types + r], re.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_EDGE_TILE;
    if (tile0 >= m) return;
    const NstType &ts = a.t[re.src], &td = a.t[re.dst];
    const int64_t n_src = nsu_clamp(a.counts[b * a.counts_stride + re.src], ts.pitch);
    const int64_t n_dst = nsu_clamp(a.counts[b * a.counts_stride + re.dst], td.pitch);
    const NstWords tbs(a, ts, b), tbd(a, td, b);
    const auto look_s = [&](int64_t p) { return tbs.vals[tbs.slot[p] & ~NSU_FLAG]; };
    const auto look_d = [&](int64_t p) { return tbd.vals[tbd.slot[p] & ~NSU_FLAG]; };
    const int64_t *rows = re.rows + b * re.pitch, *cols = re.cols + b * re.pitch;
    int64_t *rows_u = re.rows_u + b * re.pitch, *cols_u = re.cols_u + b * re.pitch;
    int64_t rr[NSU_EDGE_PER], cc[NSU_EDGE_PER];
#pragma unroll
    for (int k = 0; k < NSU_EDGE_PER; ++k) { // element e is read before it is written: in place is fine
        const int64_t e = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        rr[k] = e < m ? rows[e] : -1;
        cc[k] = e < m ? cols[e] : -1;
    }
#pragma unroll
    for (int k = 0; k < NSU_EDGE_PER; ++k) {
        const int64_t e = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (e < m) {
            rows_u[e] = nsu_end(rr[k], n_src, look_s);
            cols_u[e] = nsu_end(cc[k], n_dst, look_d);
        }
    }
}

// ---- host side: what a shape needs, which form it takes -----------------------------------------------------------------
struct NstPlan {
    int n_types;
    int key_bytes[TG_HET_MAX_TYPES];
    int64_t table_cap[TG_HET_MAX_TYPES];
    int64_t loc_off[TG_HET_MAX_TYPES];  // LDS form: u16 words before the type's
    int64_t table_bytes, lds_bytes;     // LDS form: the table area (the largest type's), everything
    int lds_ok, threads;                // the LDS form's words fit their widths (the LDS limit is checked apart)
    int64_t n_tiles[TG_HET_MAX_TYPES], max_tiles, max_cap;
    int64_t keys_off[TG_HET_MAX_TYPES], vals_off[TG_HET_MAX_TYPES], slot_off[TG_HET_MAX_TYPES], tile_off[TG_HET_MAX_TYPES];
    int64_t batch_bytes;                // flat form: a batch's part of the workspace
};

static int nst_plan(int32_t n_types, const int64_t *pitch_nodes, const int64_t *id_bound, const char *who, NstPlan &pl) {
    TG_REQUIRE(n_types >= 1 && n_types <= TG_HET_MAX_TYPES, "%s: n_types = %d outside [1, %d]", who, n_types, TG_HET_MAX_TYPES);
    TG_REQUIRE(pitch_nodes && id_bound, "%s: null pitch_nodes / id_bound", who);
    pl.n_types = n_types;
    pl.table_bytes = 0, pl.lds_ok = 1, pl.max_tiles = 1, pl.max_cap = 0;
    int64_t loc_words = 0, off = 0, max_pitch = 0;
    for (int t = 0; t < n_types; ++t) {
        const int64_t pitch = pitch_nodes[t];
        TG_REQUIRE(pitch >= 0 && pitch <= NSU_MAX_NODES, "%s: pitch_nodes[%d] = %lld outside [0, 2^30]", who, t, (long long)pitch);
        TG_REQUIRE(id_bound[t] >= 1, "%s: id_bound[%d] = %lld, at least 1 expected", who, t, (long long)id_bound[t]);
        pl.key_bytes[t] = id_bound[t] <= ((int64_t)1 << 31) ? 4 : 8;
        pl.table_cap[t] = pow2_at_least((4 * pitch + 2) / 3); // > pitch: a probe always meets an empty slot
        pl.table_bytes = std::max(pl.table_bytes, pl.table_cap[t] * (pl.key_bytes[t] + 4));
        pl.loc_off[t] = loc_words;
        loc_words += (pitch + 7) & ~(int64_t)7; // every type's words start 16-byte aligned
        if (pitch > NSU_LDS_MAX_NODES) pl.lds_ok = 0;
        max_pitch = std::max(max_pitch, pitch);
        pl.n_tiles[t] = pitch > 0 ? (pitch + NSU_TILE - 1) / NSU_TILE : 1;
        pl.max_tiles = std::max(pl.max_tiles, pl.n_tiles[t]);
        pl.max_cap = std::max(pl.max_cap, pl.table_cap[t]);
        pl.keys_off[t] = off;
        pl.vals_off[t] = pl.keys_off[t] + nsu_r256(pl.table_cap[t] * pl.key_bytes[t]);
        pl.slot_off[t] = pl.vals_off[t] + nsu_r256(pl.table_cap[t] * 4);
        pl.tile_off[t] = pl.slot_off[t] + nsu_r256(pitch * 4);
        off = pl.tile_off[t] + nsu_r256(pl.n_tiles[t] * 4);
    }
    pl.batch_bytes = off;
    pl.lds_bytes = pl.table_bytes + 2 * loc_words + NSU_STATIC_LDS;
    pl.threads = max_pitch >= NSU_THREADS ? NSU_THREADS : (int)(max_pitch < 64 ? 64 : (max_pitch + 63) & ~(int64_t)63);
    return TG_OK;
}

static inline bool nst_fits(const NstPlan &pl, int64_t lds_limit) { return pl.lds_ok && pl.lds_bytes <= lds_limit; }

static int nst_launch_lds(const NstArgs &a, const NstPlan &pl, hipStream_t stream) {
    const int64_t dyn = pl.lds_bytes - NSU_STATIC_LDS;
    static std::atomic<int64_t> raised[64];
    if (const int rc = nsu_raise_lds(reinterpret_cast<const void *>(nst_lds_kernel), raised, dyn)) return rc;
    const unsigned grid = (unsigned)(a.n_batches < 16384 ? a.n_batches : 16384);
    hipLaunchKernelGGL(nst_lds_kernel, dim3(grid), dim3(pl.threads), (size_t)dyn, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

static int nst_launch_flat(const NstArgs &a, const NstPlan &pl, int64_t max_edge_pitch, bool any_inverse, hipStream_t stream) {
    const unsigned nb = (unsigned)a.n_batches, tiles = (unsigned)pl.max_tiles, T = (unsigned)a.n_types;
    const dim3 block(NSU_TILE_THREADS);
    const int64_t clear_blocks = (pl.max_cap + NSU_TILE_THREADS - 1) / NSU_TILE_THREADS;
    hipLaunchKernelGGL(nst_clear_kernel, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024), nb, T), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nst_insert_kernel, dim3(tiles, nb, T), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nst_flag_kernel, dim3(tiles, nb, T), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nst_apply_kernel, dim3(tiles, nb, T), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    if (any_inverse) {
        hipLaunchKernelGGL(nst_inverse_kernel, dim3(tiles, nb, T), block, 0, stream, a);
        TG_LAUNCH_CHECK();
    }
    const int64_t edge_tiles = (max_edge_pitch + NSU_EDGE_TILE - 1) / NSU_EDGE_TILE;
    if (a.n_rels > 0 && edge_tiles > 0) {
        hipLaunchKernelGGL(nst_edges_kernel, dim3((unsigned)edge_tiles, nb, (unsigned)a.n_rels), block, 0, stream, a);
        TG_LAUNCH_CHECK();
    }
    return TG_OK;
}

} // namespace tg

extern "C" int tg_ns_typed_unique_form(int32_t n_types, const int64_t *pitch_nodes, const int64_t *id_bound,
                                       int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_ns_typed_unique_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    NstPlan pl;
    if (const int rc = nst_plan(n_types, pitch_nodes, id_bound, who, pl)) return rc;
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : nsu_device_lds_limit();
    *form = nst_fits(pl, limit) ? 1 : 2;
    *lds_bytes = pl.lds_bytes;
    return TG_OK;
}

extern "C" int tg_ns_typed_unique_workspace_bytes(int32_t n_types, const int64_t *pitch_nodes, const int64_t *id_bound,
                                                  int64_t n_batches, int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_typed_unique_workspace_bytes";
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    NstPlan pl;
    if (const int rc = nst_plan(n_types, pitch_nodes, id_bound, who, pl)) return rc;
    *bytes_min = pl.batch_bytes;
    *bytes = nst_fits(pl, nsu_device_lds_limit()) ? 0 : pl.batch_bytes * n_batches;
    return TG_OK;
}

extern "C" int tg_ns_typed_unique(const tg_ns_typed_in *in, int64_t n_batches, const tg_ns_typed_unique_out *out,
                                  void *workspace, int64_t workspace_bytes, int32_t form, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_typed_unique";
    TG_REQUIRE(in && out, "%s: null argument", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    const int32_t T = in->n_types, R = in->n_rels;
    NstPlan pl;
    if (const int rc = nst_plan(T, in->pitch_nodes, in->id_bound, who, pl)) return rc;
    TG_REQUIRE(R >= 0 && R <= TG_HET_MAX_RELS, "%s: n_rels = %d outside [0, %d]", who, R, TG_HET_MAX_RELS);
    TG_REQUIRE(R == 0 || (in->rel_src && in->rel_dst && in->pitch_edges), "%s: null rel_src / rel_dst / pitch_edges", who);
    int64_t max_edge_pitch = 0;
    for (int r = 0; r < R; ++r) {
        TG_REQUIRE(in->rel_src[r] >= 0 && in->rel_src[r] < T, "%s: rel_src[%d] = %d outside [0, %d)", who, r, in->rel_src[r], T);
        TG_REQUIRE(in->rel_dst[r] >= 0 && in->rel_dst[r] < T, "%s: rel_dst[%d] = %d outside [0, %d)", who, r, in->rel_dst[r], T);
        TG_REQUIRE(in->pitch_edges[r] >= 0 && in->pitch_edges[r] <= NSU_MAX_NODES, "%s: pitch_edges[%d] = %lld outside [0, 2^30]",
                   who, r, (long long)in->pitch_edges[r]);
        max_edge_pitch = std::max(max_edge_pitch, in->pitch_edges[r]);
    }
    TG_REQUIRE(in->counts_stride >= T + R, "%s: counts_stride = %lld below n_types + n_rels = %d", who,
               (long long)in->counts_stride, T + R);
    TG_REQUIRE(!out->seed_counts || in->n_inputs, "%s: seed_counts asked for without n_inputs (null)", who);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(form >= 0 && form <= 2, "%s: unknown form %d (0 auto, 1 LDS, 2 flat)", who, form);
    const bool fits = form != 2 && nst_fits(pl, nsu_device_lds_limit());
    TG_REQUIRE(form != 1 || fits, "%s: form 1: %lld bytes of LDS (a table area of %lld bytes and a word per position of every type) "
               "does not fit a workgroup", who, (long long)pl.lds_bytes, (long long)pl.table_bytes);
    const bool lds = form != 2 && fits;
    if (!lds)
        TG_REQUIRE(workspace && workspace_bytes >= pl.batch_bytes, "%s: workspace too small (%lld < %lld, the size of one batch)",
                   who, (long long)(workspace ? workspace_bytes : 0), (long long)pl.batch_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    if (n_batches == 0) return TG_OK;
    // device pointers
    TG_REQUIRE(in->samples && in->counts && out->nodes && out->counts, "%s: null samples / counts / nodes", who);
    TG_REQUIRE(R == 0 || (in->rows && in->cols && out->rows && out->cols), "%s: null edge slab arrays", who);
    for (int t = 0; t < T; ++t)
        TG_REQUIRE(in->pitch_nodes[t] == 0 || (in->samples[t] && out->nodes[t]), "%s: null samples / nodes slab of type %d", who, t);
    for (int r = 0; r < R; ++r)
        TG_REQUIRE(in->pitch_edges[r] == 0 || (in->rows[r] && in->cols[r] && out->rows[r] && out->cols[r]),
                   "%s: null edge slab of relation %d", who, r);
    hipStream_t stream = (hipStream_t)stream_;

    bool any_inverse = false;
    const int64_t round = lds ? n_batches : std::min(std::min(workspace_bytes / pl.batch_bytes, NSU_ROUND_MAX), n_batches);
    for (int64_t b0 = 0; b0 < n_batches; b0 += round) {
        NstArgs a{};
        for (int t = 0; t < T; ++t) {
            NstType &ty = a.t[t];
            const int64_t pitch = in->pitch_nodes[t];
            ty.samples = in->samples[t] ? in->samples[t] + b0 * pitch : nullptr;
            ty.nodes = out->nodes[t] ? out->nodes[t] + b0 * pitch : nullptr;
            ty.inverse = out->inverse && out->inverse[t] ? out->inverse[t] + b0 * pitch : nullptr;
            any_inverse |= ty.inverse != nullptr;
            ty.pitch = pitch, ty.n_inputs = in->n_inputs ? in->n_inputs[t] : 0;
            ty.keys_off = pl.keys_off[t], ty.vals_off = pl.vals_off[t], ty.slot_off = pl.slot_off[t], ty.tile_off = pl.tile_off[t];
            nsu_mask_shift(pl.table_cap[t], ty.cap_mask, ty.hash_shift);
            ty.n_tiles = (int32_t)pl.n_tiles[t], ty.key64 = pl.key_bytes[t] == 8;
            ty.loc_off = (uint32_t)pl.loc_off[t];
        }
        for (int r = 0; r < R; ++r) {
            NstRel &re = a.r[r];
            const int64_t pitch = in->pitch_edges[r];
            re.rows = in->rows[r] ? in->rows[r] + b0 * pitch : nullptr, re.cols = in->cols[r] ? in->cols[r] + b0 * pitch : nullptr;
            re.rows_u = out->rows[r] ? out->rows[r] + b0 * pitch : nullptr;
            re.cols_u = out->cols[r] ? out->cols[r] + b0 * pitch : nullptr;
            re.pitch = pitch, re.src = in->rel_src[r], re.dst = in->rel_dst[r];
        }
        a.counts = in->counts + b0 * in->counts_stride, a.counts_u = out->counts + b0 * in->counts_stride;
        a.seed_counts = out->seed_counts ? out->seed_counts + b0 * T : nullptr;
        a.counts_stride = in->counts_stride, a.n_batches = std::min(round, n_batches - b0), a.batch_bytes = pl.batch_bytes;
        a.ws = static_cast<unsigned char *>(workspace);
        a.n_types = T, a.n_rels = R, a.loc_base = (uint32_t)pl.table_bytes;
        const int rc = lds ? nst_launch_lds(a, pl, stream) : nst_launch_flat(a, pl, max_edge_pitch, any_inverse, stream);
        if (rc) return rc;
    }
    return TG_OK;
}
