// Per-batch induced subgraph of a list of distinct nodes (tg_ns_induced_count / tg_ns_induced_emit, include/tchgeo.h):
// PyG's directed=False edge set behind tg_ns_homo_unique.
//
// The rule, per batch: local(v) = the FIRST position of v in nodes[:n]; for every position i in list order and every CSC
// offset e of column nodes[i] in ascending order, (local(indices[e]), i, e) is emitted where local exists.  Output order
// is (i, e) ascending; parallel edges and self loops are emitted, each offset once per position that scans it.
//
// One form, the flat one (the argument is ns_unique.hip's: the loader's shape fits no LDS and has too few batches to
// fill the device batch by batch).  Per batch the workspace holds the open-addressing table of ns_unique.h (key = id,
// value = first position by atomicMin), the node-chunk prefix, and one word per chunk.
//
// Columns are cut into chunks of CS_CHUNK consecutive CSC offsets; the chunk size, the count / prefix / emit scheme and
// the unit walk are chunk_scan.h's.
//
// Pass 1: clear (table, tile sums, header) | insert + chunks per node, scanned inside a tile of positions | node apply
//   (adds the tiles before; the batch's chunk total is compared with the bound HERE, before anything indexes the
//   per-chunk array: overflow raises status bit 0 and the batch gets 0 chunks) | scan: hits per chunk | chunk apply (the
//   exclusive prefix over chunks in place; its total is m_b, edge_marks read it at the marks' first chunks).
// Pass 2: scan again, a chunk's hits go to edge_off[b] + its prefix, so a chunk's stores are consecutive addresses.
// A unit's look-up lanes each search one chunk's node in the node-chunk prefix (17 dependent reads for the loader's
// pitch); the unit shrinks by cs_short_quarter.
// The table of a loader-shaped batch (2^18 slots, 2 MB) does not stay in one XCD's 4 MiB L2 beside 15 others: probes are
// Infinity Cache hits at best, and only wavefronts in flight hide them -- 8 waves per SIMD, no LDS, few registers.
// An id outside [0, n_major) is a column of length 0, is not inserted and raises status bit 1.  Probe loops are capped at
// the table size.
//
// The GROUPED pair (tg_ns_induced_grouped_count / _emit: induced edges per subgraph of a disjoint list, ShaDow's k-hop
// sampler) is the same kernels with G = true: the table key is group * id_bound + id (tg_ns_homo_unique_grouped's), the
// scan reads the position's group -- and, under times, the group's time -- once per chunk in the unit's look-up lanes, and
// a table hit is kept only where tg_filter_pass admits the edge's timestamp (loaded behind the hit, the same expression in
// both passes).  Columns of such a list are not disjoint, so the chunk capacity is the caller's (chunk_cap), the exact
// chunk count goes to chunks[b], and the comparison still happens in the node apply kernel.  A group word outside
// [0, n_groups) is a column of length 0, is not inserted and raises status bit 2.  The G = false instances are what the
// ungrouped exports launch: no group word is read, no key is widened, no timestamp is looked at.
#include "chunk_scan.h"
#include "tg_filter.h"

namespace tg {

struct NsiArgs {
    const int64_t *ptrs, *indices;
    const uint32_t *ptrs32, *indices32;
    int64_t n_major;
    const int64_t *nodes, *counts, *node_marks; // batch 0 of the launch
    int64_t pitch, counts_stride;
    int32_t n_marks;
    int64_t *n_edges, *edge_marks;
    int32_t *status;
    const int64_t *edge_off;
    int64_t *rows, *cols, *edge_index;
    unsigned char *ws;
    int64_t batch_bytes, vals_off, npref_off, ntile_off, cpref_off, ctile_off, chunk_bound;
    int64_t table_cap, chunk_tiles;
    uint32_t cap_mask, hash_shift;
    // the grouped pair
    const int64_t *group, *group_time, *timestamps; // group: batch 0 of the launch; group_time: [n_groups] per batch or null
    int64_t n_groups, win_lo, win_hi;
    uint64_t key_mul;                               // id_bound: key = group * key_mul + id
    int64_t *chunks;                                // [batches] the exact chunk counts, or null
};

template <typename K> struct NsiBatch {
    unsigned long long *hdr, *npref, *ntile, *cpref, *ctile;
    K *keys;
    uint32_t *vals;
    __device__ __forceinline__ NsiBatch(const NsiArgs &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        hdr = reinterpret_cast<unsigned long long *>(base);
        keys = reinterpret_cast<K *>(base + CS_HEADER);
        vals = reinterpret_cast<uint32_t *>(base + a.vals_off);
        npref = reinterpret_cast<unsigned long long *>(base + a.npref_off); // [pitch + 1] chunks before a position
        ntile = reinterpret_cast<unsigned long long *>(base + a.ntile_off); // [node tiles]
        cpref = reinterpret_cast<unsigned long long *>(base + a.cpref_off); // [chunk_bound + 1] hits of / before a chunk
        ctile = reinterpret_cast<unsigned long long *>(base + a.ctile_off); // [chunk tiles]
    }
};

template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsi_clear_kernel(const NsiArgs a) {
    const NsiBatch<K> t(a, blockIdx.y);
    cs_clear<1>(t.keys, t.vals, a.table_cap, t.ctile, a.chunk_tiles, t.hdr, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                (int64_t)gridDim.x * blockDim.x);
}

// a tile of positions: insert, chunks per position, their exclusive prefix inside the tile and the tile's sum
template <typename K, bool G> __global__ void __launch_bounds__(CS_THREADS) nsi_insert_kernel(const NsiArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride], a.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsiBatch<K> t(a, b);
    const int64_t *nodes = a.nodes + b * a.pitch;
    const int64_t *group = G ? a.group + b * a.pitch : nullptr;
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    unsigned long long c[NSU_PER], mine = 0;
    bool outside = false, no_group = false;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        c[k] = 0;
        const int64_t p = p0 + k;
        if (p < n) {
            const int64_t v = nodes[p];
            K key = (K)v;
            bool grouped = true;
            if (G) {
                const int64_t g = group[p];
                grouped = (uint64_t)g < (uint64_t)a.n_groups;
                no_group |= !grouped;
                key += (K)g * (K)a.key_mul;
            }
            if ((uint64_t)v >= (uint64_t)a.n_major) {
                outside = true;
            } else if (grouped) {
                const uint32_t s = nsu_insert<K>(t.keys, a.cap_mask, a.hash_shift, key);
                atomicMin(&t.vals[s], (uint32_t)p);
                const int64_t deg = csc_ptr(a.ptrs, a.ptrs32, v + 1) - csc_ptr(a.ptrs, a.ptrs32, v);
                if (deg > 0) c[k] = (unsigned long long)((deg + CS_CHUNK - 1) / CS_CHUNK);
            }
        }
        mine += c[k];
    }
    if (outside) atomicOr(a.status, 2);
    if (G && no_group) atomicOr(a.status, 4);
    unsigned long long total;
    unsigned long long run = nsu_scan64(mine, s_wave, &total);
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        if (p0 + k < n) t.npref[p0 + k] = run;
        run += c[k];
    }
    if (threadIdx.x == 0) t.ntile[blockIdx.x] = total;
}

// adds the chunks of the tiles before; the last tile closes the prefix and decides whether the batch fits the bound
template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsi_node_apply_kernel(const NsiArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride], a.pitch);
    const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsiBatch<K> t(a, b);
    const unsigned long long base = cs_tiles_before(t.ntile, s_wave);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k)
        if (p0 + k < n) t.npref[p0 + k] += base;
    if (tile0 + CS_TILE >= n && threadIdx.x == 0) { // the batch's last tile (tile 0 of an empty batch)
        const unsigned long long total = base + t.ntile[blockIdx.x];
        t.npref[n] = total;
        if (a.chunks) a.chunks[b] = (int64_t)total;
        if (total > (unsigned long long)a.chunk_bound) {
            atomicOr(a.status, 1);
            t.hdr[0] = 0;
        } else {
            t.hdr[0] = total;
        }
    }
}

// EMIT = false: hits per chunk (and their sum per tile of chunks); true: the hits themselves
template <typename K, bool I32, bool EMIT, bool G>
__global__ void __launch_bounds__(CS_THREADS) nsi_scan_kernel(const NsiArgs a) {
    const int64_t b = blockIdx.y;
    const NsiBatch<K> t(a, b);
    const unsigned long long n_chunks = t.hdr[0];
    if (n_chunks == 0) return;
    const int64_t n = nsu_clamp(a.counts[b * a.counts_stride], a.pitch);
    const int64_t *nodes = a.nodes + b * a.pitch;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = CS_THREADS / 64;
    int unit = CS_UNIT;
    while (unit > 1 && cs_short_quarter(n_chunks, unit, gridDim.x, waves)) unit >>= 1;
    const unsigned long long n_units = (n_chunks + unit - 1) / unit;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    const int64_t out0 = EMIT ? a.edge_off[b] : 0;
    for (unsigned long long u = (unsigned long long)blockIdx.x * waves + wave; u < n_units; u += (unsigned long long)gridDim.x * waves) {
        const unsigned long long c = u * unit + lane;
        long long my_i = 0, my_e0 = 0, my_time = 0;
        int my_len = 0;
        uint32_t my_group = 0;
        if (lane < unit && c < n_chunks) {
            const int64_t lo = cs_last_le(t.npref, n, c); // npref[0] = 0 <= c < n_chunks = npref[n]
            const int64_t v = nodes[lo];                  // in range: it has chunks
            const int64_t col0 = csc_ptr(a.ptrs, a.ptrs32, v), col1 = csc_ptr(a.ptrs, a.ptrs32, v + 1);
            my_i = lo;
            my_e0 = col0 + (int64_t)(c - t.npref[lo]) * CS_CHUNK;
            my_len = (int)std::min<int64_t>(CS_CHUNK, col1 - my_e0);
            if (G) { // the position has chunks, so its group word is in range
                my_group = (uint32_t)a.group[b * a.pitch + lo];
                if (a.group_time) my_time = a.group_time[b * a.n_groups + my_group];
            }
        }
        unsigned long long unit_hits = 0;
        for (int q = 0; q < unit; ++q) {
            const unsigned long long cq = u * unit + q;
            if (cq >= n_chunks) break; // uniform
            const long long i = __shfl(my_i, q), e0 = __shfl(my_e0, q);
            const int len = __shfl(my_len, q);
            const K key0 = G ? (K)__shfl(my_group, q) * (K)a.key_mul : (K)0;
            const long long time = G ? __shfl(my_time, q) : 0;
            const int64_t out = EMIT ? out0 + (int64_t)t.cpref[cq] : 0;
            uint32_t cnt = 0;
            for (int s = 0; s < len; s += 64) {
                const int64_t e = e0 + s + lane;
                uint32_t pos = NSU_UNSEEN;
                if (s + lane < len) {
                    const K key = key0 + (I32 ? (K)a.indices32[e] : (K)a.indices[e]);
                    pos = cs_find<true, false>(t.keys, t.vals, a.cap_mask, a.hash_shift, key); // the first position
                    if (G && pos != NSU_UNSEEN && a.group_time &&
                        !tg_filter_pass(TG_FILTER_RELATIVE, 0, a.win_lo, a.win_hi, time, a.timestamps[e]))
                        pos = NSU_UNSEEN;
                }
                const unsigned long long hits = __ballot(pos != NSU_UNSEEN);
                if (EMIT && pos != NSU_UNSEEN) {
                    const int64_t o = out + cnt + __popcll(hits & below);
                    a.rows[o] = (int64_t)pos;
                    a.cols[o] = i;
                    a.edge_index[o] = e;
                }
                cnt += (uint32_t)__popcll(hits);
            }
            if (!EMIT) {
                if (lane == 0) t.cpref[cq] = cnt;
                unit_hits += cnt;
            }
        }
        if (!EMIT) cs_unit_counted(t.ctile, u, unit, unit_hits, lane);
    }
}

// the exclusive prefix over a tile of chunks, in place; the last tile writes m_b; edge_marks read the prefix at the marks'
// first chunks
template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsi_chunk_apply_kernel(const NsiArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    const NsiBatch<K> t(a, b);
    const unsigned long long n_chunks = t.hdr[0];
    if (cs_tile_idle(n_chunks)) return;
    unsigned long long pre[NSU_PER];
    const CsTile<unsigned long long> r = cs_chunk_apply_tile(t.cpref, t.ctile, n_chunks, s_wave, pre);
    const int64_t m_b = (int64_t)(r.base + r.total);
    if (r.last && threadIdx.x == 0) {
        t.cpref[n_chunks] = r.base + r.total;
        a.n_edges[b] = m_b;
    }
    if (a.edge_marks) {
        const int64_t n = nsu_clamp(a.counts[b * a.counts_stride], a.pitch);
        for (int m = 0; m < a.n_marks; ++m) {
            const int64_t L = nsu_clamp(a.node_marks[b * a.n_marks + m], n);
            const unsigned long long cs = n_chunks ? t.npref[L] : 0; // the first chunk of position L (n_chunks: none left)
            if (cs >= n_chunks) {
                if (r.last && threadIdx.x == 0) a.edge_marks[b * a.n_marks + m] = m_b;
            } else if (cs >= r.c0 && cs < r.c0 + NSU_PER) {
                a.edge_marks[b * a.n_marks + m] = (int64_t)pre[cs - r.c0];
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct NsiPlan {
    NsuPlan table;
    int64_t chunk_bound, node_tiles, chunk_tiles;
    int64_t vals_off, npref_off, ntile_off, cpref_off, ctile_off, batch_bytes;
};

// n_groups = 0: the ungrouped pair (key = id, the chunk bound is the graph's); else key = group * id_bound + id and
// chunk_cap > 0 is the caller's capacity
static int nsi_plan(const tg_graph *csc, int64_t pitch, int64_t id_bound, int64_t n_groups, int64_t chunk_cap, const char *who,
                    NsiPlan &pl) {
    TG_REQUIRE(pitch >= 0 && pitch <= NSU_MAX_NODES, "%s: pitch_nodes = %lld outside [0, 2^30]", who, (long long)pitch);
    // distinct nodes have disjoint columns, which is cs_plan_chunks' default bound.  A disjoint list has no such property;
    // there it is only the default a caller may raise
    if (const int rc = cs_plan_chunks(csc, pitch, chunk_cap, who, pl.chunk_bound, pl.chunk_tiles)) return rc;
    TG_REQUIRE(id_bound >= 1, "%s: id_bound = %lld, at least 1 expected", who, (long long)id_bound);
    int64_t key_bound = id_bound;
    if (n_groups) {
        TG_REQUIRE(n_groups <= 0x7fffffff, "%s: n_groups = %lld does not fit a 31-bit group word", who, (long long)n_groups);
        TG_REQUIRE(id_bound <= INT64_MAX / n_groups, "%s: n_groups * id_bound = %lld * %lld reaches 2^63: no key holds the pair",
                   who, (long long)n_groups, (long long)id_bound);
        key_bound = n_groups * id_bound;
    }
    if (const int rc = nsu_plan(pitch, key_bound, who, pl.table)) return rc; // the key width, the table
    TG_REQUIRE(id_bound >= csc->n_major, "%s: id_bound = %lld below n_major = %lld", who, (long long)id_bound,
               (long long)csc->n_major);
    pl.node_tiles = pitch > 0 ? (pitch + CS_TILE - 1) / CS_TILE : 1;
    pl.vals_off = CS_HEADER + nsu_r256(pl.table.table_cap * pl.table.key_bytes);
    pl.npref_off = pl.vals_off + nsu_r256(pl.table.table_cap * 4);
    pl.ntile_off = pl.npref_off + nsu_r256((pitch + 1) * 8);
    pl.cpref_off = pl.ntile_off + nsu_r256(pl.node_tiles * 8);
    pl.ctile_off = pl.cpref_off + nsu_r256((pl.chunk_bound + 1) * 8);
    pl.batch_bytes = pl.ctile_off + nsu_r256(pl.chunk_tiles * 8);
    return TG_OK;
}

// what both passes check alike, and the kernel arguments of batch 0
static int nsi_common(const tg_graph *csc, const tg_ns_induced_in *in, const tg_ns_induced_grouped_in *gin, int64_t n_batches,
                      int64_t id_bound, void *workspace, int64_t workspace_bytes, const char *who, NsiPlan &pl, NsiArgs &a) {
    TG_REQUIRE(csc && in, "%s: null argument", who);
    if (gin) TG_REQUIRE(gin->n_groups >= 1, "%s: n_groups = %lld, at least 1 expected", who, (long long)gin->n_groups);
    if (const int rc = nsi_plan(csc, in->pitch_nodes, id_bound, gin ? gin->n_groups : 0, gin ? gin->chunk_cap : 0, who, pl))
        return rc;
    if (gin) {
        TG_REQUIRE(gin->group, "%s: null group", who);
        TG_REQUIRE(!gin->group_time || csc->timestamps, "%s: group_time given, but the graph has no timestamps", who);
    }
    TG_REQUIRE(in->counts_stride >= 1, "%s: counts_stride = %lld, at least 1 expected", who, (long long)in->counts_stride);
    TG_REQUIRE(in->n_marks >= 0 && in->n_marks <= TG_MAX_HOPS, "%s: n_marks = %d outside [0, %d]", who, in->n_marks, TG_MAX_HOPS);
    if (const int rc = cs_check_launch(csc, n_batches, pl.batch_bytes, workspace, workspace_bytes, who)) return rc;
    TG_REQUIRE(in->nodes && in->counts, "%s: null nodes / counts", who);
    a = NsiArgs{};
    a.ptrs = csc->ptrs, a.indices = csc->indices, a.ptrs32 = csc->ptrs32, a.indices32 = csc->indices32;
    a.n_major = csc->n_major;
    a.nodes = in->nodes, a.counts = in->counts, a.node_marks = in->node_marks;
    a.pitch = in->pitch_nodes, a.counts_stride = in->counts_stride, a.n_marks = in->n_marks;
    a.ws = static_cast<unsigned char *>(workspace);
    a.batch_bytes = pl.batch_bytes, a.vals_off = pl.vals_off, a.npref_off = pl.npref_off, a.ntile_off = pl.ntile_off;
    a.cpref_off = pl.cpref_off, a.ctile_off = pl.ctile_off, a.chunk_bound = pl.chunk_bound;
    a.table_cap = pl.table.table_cap, a.chunk_tiles = pl.chunk_tiles;
    nsu_mask_shift(pl.table.table_cap, a.cap_mask, a.hash_shift);
    if (gin) {
        a.group = gin->group, a.group_time = gin->group_time, a.timestamps = csc->timestamps;
        a.n_groups = gin->n_groups, a.win_lo = gin->window_lo, a.win_hi = gin->window_hi;
        a.key_mul = (uint64_t)id_bound;
    }
    return TG_OK;
}

// the ungrouped fields of a grouped input
static tg_ns_induced_in nsi_plain(const tg_ns_induced_grouped_in *g) {
    tg_ns_induced_in in{};
    if (g) {
        in.nodes = g->nodes, in.pitch_nodes = g->pitch_nodes, in.counts = g->counts, in.counts_stride = g->counts_stride;
        in.node_marks = g->node_marks, in.n_marks = g->n_marks;
    }
    return in;
}

// the arguments of the launch that starts at batch b0
static NsiArgs nsi_at(const NsiArgs &a0, int64_t b0) {
    NsiArgs a = a0;
    a.nodes += b0 * a.pitch, a.counts += b0 * a.counts_stride, a.ws += b0 * a.batch_bytes;
    if (a.group) a.group += b0 * a.pitch;
    if (a.group_time) a.group_time += b0 * a.n_groups;
    if (a.chunks) a.chunks += b0;
    if (a.node_marks) a.node_marks += b0 * a.n_marks;
    if (a.edge_marks) a.edge_marks += b0 * a.n_marks;
    if (a.n_edges) a.n_edges += b0;
    if (a.edge_off) a.edge_off += b0;
    return a;
}

template <typename K, bool G> static int nsi_launch_count(const NsiArgs &a, const NsiPlan &pl, int64_t nb_, hipStream_t stream) {
    const unsigned nb = (unsigned)nb_;
    const dim3 block(CS_THREADS);
    const int64_t clear_blocks = (pl.table.table_cap + CS_THREADS - 1) / CS_THREADS;
    hipLaunchKernelGGL(nsi_clear_kernel<K>, dim3((unsigned)std::min<int64_t>(clear_blocks, 1024), nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL((nsi_insert_kernel<K, G>), dim3((unsigned)pl.node_tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsi_node_apply_kernel<K>, dim3((unsigned)pl.node_tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    if (a.indices32)
        hipLaunchKernelGGL((nsi_scan_kernel<K, true, false, G>), dim3(cs_scan_grid(nb_), nb), block, 0, stream, a);
    else
        hipLaunchKernelGGL((nsi_scan_kernel<K, false, false, G>), dim3(cs_scan_grid(nb_), nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsi_chunk_apply_kernel<K>, dim3((unsigned)pl.chunk_tiles, nb), block, 0, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <typename K, bool G> static int nsi_launch_emit(const NsiArgs &a, int64_t nb_, hipStream_t stream) {
    const dim3 grid(cs_scan_grid(nb_), (unsigned)nb_), block(CS_THREADS);
    if (a.indices32)
        hipLaunchKernelGGL((nsi_scan_kernel<K, true, true, G>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((nsi_scan_kernel<K, false, true, G>), grid, block, 0, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

// the passes of either pair over launches of at most CS_ROUND_MAX batches
template <bool G> static int nsi_count(const NsiArgs &a0, const NsiPlan &pl, int64_t n_batches, hipStream_t stream) {
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb) {
        const NsiArgs a = nsi_at(a0, b0);
        return pl.table.key_bytes == 4 ? nsi_launch_count<nsu_k32, G>(a, pl, nb, stream)
                                       : nsi_launch_count<nsu_k64, G>(a, pl, nb, stream);
    });
}

template <bool G> static int nsi_emit(const NsiArgs &a0, const NsiPlan &pl, int64_t n_batches, hipStream_t stream) {
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb) {
        const NsiArgs a = nsi_at(a0, b0);
        return pl.table.key_bytes == 4 ? nsi_launch_emit<nsu_k32, G>(a, nb, stream) : nsi_launch_emit<nsu_k64, G>(a, nb, stream);
    });
}

} // namespace tg

extern "C" int tg_ns_induced_workspace_bytes(const tg_graph *csc, int64_t pitch_nodes, int64_t id_bound, int64_t n_batches,
                                             int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_induced_workspace_bytes";
    NsiPlan pl;
    if (const int rc = nsi_plan(csc, pitch_nodes, id_bound, 0, 0, who, pl)) return rc;
    return cs_answer_bytes(pl.batch_bytes, n_batches, who, bytes, bytes_min);
}

extern "C" int tg_ns_induced_count(const tg_graph *csc, const tg_ns_induced_in *in, int64_t n_batches, int64_t id_bound,
                                   int64_t *n_edges, int64_t *edge_marks, int32_t *status, void *workspace,
                                   int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_induced_count";
    NsiPlan pl;
    NsiArgs a0;
    if (const int rc = nsi_common(csc, in, nullptr, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(n_edges && status, "%s: null n_edges / status", who);
    a0.n_edges = n_edges, a0.status = status;
    a0.edge_marks = in->n_marks > 0 && in->node_marks ? edge_marks : nullptr;
    return nsi_count<false>(a0, pl, n_batches, (hipStream_t)stream_);
}

extern "C" int tg_ns_induced_emit(const tg_graph *csc, const tg_ns_induced_in *in, int64_t n_batches, int64_t id_bound,
                                  const int64_t *edge_off, int64_t *rows, int64_t *cols, int64_t *edge_index, void *workspace,
                                  int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_induced_emit";
    NsiPlan pl;
    NsiArgs a0;
    if (const int rc = nsi_common(csc, in, nullptr, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(edge_off && rows && cols && edge_index, "%s: null edge_off / rows / cols / edge_index", who);
    a0.edge_off = edge_off, a0.rows = rows, a0.cols = cols, a0.edge_index = edge_index;
    return nsi_emit<false>(a0, pl, n_batches, (hipStream_t)stream_);
}

extern "C" int tg_ns_induced_grouped_workspace_bytes(const tg_graph *csc, int64_t pitch_nodes, int64_t id_bound,
                                                     int64_t n_groups, int64_t chunk_cap, int64_t n_batches, int64_t *bytes,
                                                     int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_induced_grouped_workspace_bytes";
    TG_REQUIRE(n_groups >= 1, "%s: n_groups = %lld, at least 1 expected", who, (long long)n_groups);
    NsiPlan pl;
    if (const int rc = nsi_plan(csc, pitch_nodes, id_bound, n_groups, chunk_cap, who, pl)) return rc;
    return cs_answer_bytes(pl.batch_bytes, n_batches, who, bytes, bytes_min);
}

extern "C" int tg_ns_induced_grouped_count(const tg_graph *csc, const tg_ns_induced_grouped_in *in, int64_t n_batches,
                                           int64_t id_bound, int64_t *n_edges, int64_t *edge_marks, int64_t *chunks,
                                           int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_induced_grouped_count";
    NsiPlan pl;
    NsiArgs a0;
    const tg_ns_induced_in plain = nsi_plain(in);
    if (const int rc = nsi_common(csc, in ? &plain : nullptr, in, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0))
        return rc;
    TG_REQUIRE(n_edges && status, "%s: null n_edges / status", who);
    a0.n_edges = n_edges, a0.status = status, a0.chunks = chunks;
    a0.edge_marks = in->n_marks > 0 && in->node_marks ? edge_marks : nullptr;
    return nsi_count<true>(a0, pl, n_batches, (hipStream_t)stream_);
}

extern "C" int tg_ns_induced_grouped_emit(const tg_graph *csc, const tg_ns_induced_grouped_in *in, int64_t n_batches,
                                          int64_t id_bound, const int64_t *edge_off, int64_t *rows, int64_t *cols,
                                          int64_t *edge_index, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_induced_grouped_emit";
    NsiPlan pl;
    NsiArgs a0;
    const tg_ns_induced_in plain = nsi_plain(in);
    if (const int rc = nsi_common(csc, in ? &plain : nullptr, in, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0))
        return rc;
    TG_REQUIRE(edge_off && rows && cols && edge_index, "%s: null edge_off / rows / cols / edge_index", who);
    a0.edge_off = edge_off, a0.rows = rows, a0.cols = cols, a0.edge_index = edge_index;
    return nsi_emit<true>(a0, pl, n_batches, (hipStream_t)stream_);
}
