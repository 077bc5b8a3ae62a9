// Full-neighbour hop (tg_ns_full_count / tg_ns_full_emit, include/tchgeo.h): EVERY in-edge of every node of a frontier, the
// sources deduplicated in first-occurrence order behind the frontier.  The layer of layer-wise inference (PyG's
// NeighborLoader(num_neighbors=[-1]), DGL's MultiLayerFullNeighborSampler).
//
// The rule, per batch with frontier v_0 .. v_{n-1}: triple k in (i, e) ascending order is (src = indices[e], col = i, e) for
// every CSC offset e of column v_i; out_nodes = the frontier followed by every src that equals no earlier entry, in order
// of first occurrence; row_k = the FIRST position of src_k in out_nodes.  The output is ragged and exact: pass 1 counts,
// the caller allocates and passes two exclusive prefixes, pass 2 writes.
//
// Everything is chunk_scan.h's and ns_unique.h's machinery put together: columns are cut into chunks (a hub column is many
// chunks all over the device), a wave takes a unit of chunks whose look-ups run in its first lanes (the unit shrinks by
// cs_short_fill), the batch's open-addressing table holds key = id, value = first position by atomicMin.  What is new is
// that the scan INSERTS: entry k of the batch's triple order inserts its source with value n + k, so after the insert pass
// a slot's value is < n for a frontier node and n + (the first triple that names it) for a new one.
//
// Pass 1: clear (table, tile sums, header) | plan: column begin, length and chunks per position, scanned inside a tile of
//   positions | node apply: adds the tiles before; the last tile has m_b and the chunk total and takes the capacity decision
//   HERE, before any table work (refused: status bit 0, header 0 chunks, n_nodes = 0) | insert: the frontier positions
//   with value i, then every entry with value n + k | flag: an entry is a first occurrence where its slot's value equals
//   n + k; counts per chunk, summed per tile of chunks | chunk apply: the exclusive prefix over chunks in place, n_out_b.
// Pass 2: nodes: the frontier is copied, a first-occurrence entry has position n + its chunk's prefix + its rank in the chunk
//   (ballot + popcount: lane order = offset order), writes nodes_out there and LEAVES THAT POSITION IN ITS SLOT (the only
//   writer of the slot; every other entry of the same source compares against a greater n + k' and stays unflagged whichever
//   of the two words it reads) | triples: cols and edge_index are pure streams at edge_off[b] + k, rows is one table read per
//   entry.  Pass 2 therefore consumes the workspace: a second emit needs a second count.
// A position's column begin and the edges before it are kept in the workspace by the plan kernel, so the scans never touch
// `nodes` or `ptrs` again: a chunk look-up is one binary search over the chunk prefix and three loads.
#include "chunk_scan.h"

namespace tg {

constexpr uint64_t NSF_MAX_EDGES = (uint64_t)1 << 31;  // m_b below it: n + k fits the slot's 32-bit value
// the header's words: {chunks of the batch (0 when refused), accepted}

enum { NSF_INSERT = 0, NSF_FLAG = 1, NSF_NODES = 2, NSF_TRIPLES = 3 };

struct NsfArgs {
    const int64_t *ptrs, *indices;
    const uint32_t *ptrs32, *indices32;
    int64_t n_major, n_edges_graph;
    const int64_t *nodes, *node_ptr;                   // node_ptr: batch 0 of the launch
    int64_t max_nodes, node_cap, id_bound;
    int64_t *n_nodes, *n_edges, *chunks;               // pass 1
    int32_t *status;
    const int64_t *node_off, *edge_off;                // pass 2
    int64_t *nodes_out, *rows, *cols, *edge_index;
    unsigned char *ws;
    int64_t batch_bytes, vals_off, npref_off, epref_off, col0_off, ntile_off, cpref_off, ctile_off;
    int64_t chunk_bound, table_cap, chunk_tiles;
    uint32_t cap_mask, hash_shift;
};

// a batch's part of the workspace
template <typename K> struct NsfBatch {
    unsigned long long *hdr, *npref, *epref, *ntile;
    long long *col0;
    uint32_t *vals, *cpref, *ctile;
    K *keys;
    __device__ __forceinline__ NsfBatch(const NsfArgs &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        hdr = reinterpret_cast<unsigned long long *>(base);
        keys = reinterpret_cast<K *>(base + CS_HEADER);
        vals = reinterpret_cast<uint32_t *>(base + a.vals_off);
        npref = reinterpret_cast<unsigned long long *>(base + a.npref_off); // [max_nodes + 1] chunks before a position
        epref = reinterpret_cast<unsigned long long *>(base + a.epref_off); // [max_nodes + 1] triples before a position
        col0 = reinterpret_cast<long long *>(base + a.col0_off);            // [max_nodes] the column's first offset
        ntile = reinterpret_cast<unsigned long long *>(base + a.ntile_off); // [node tiles][2] chunks, triples of a tile
        cpref = reinterpret_cast<uint32_t *>(base + a.cpref_off);           // [chunk_bound + 1] new nodes of / before a chunk
        ctile = reinterpret_cast<uint32_t *>(base + a.ctile_off);           // [chunk tiles]
    }
};

// batch b's frontier: nodes[base .. base + n)
__device__ __forceinline__ int64_t nsf_list(const NsfArgs &a, int64_t b, int64_t *base) {
    *base = a.node_ptr[b];
    return nsu_clamp(a.node_ptr[b + 1] - *base, a.max_nodes);
}

template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsf_clear_kernel(const NsfArgs a) {
    const NsfBatch<K> t(a, blockIdx.y);
    cs_clear<2>(t.keys, t.vals, a.table_cap, t.ctile, a.chunk_tiles, t.hdr, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                (int64_t)gridDim.x * blockDim.x);
}

// a tile of positions: the column, its chunks and entries, their exclusive prefixes inside the tile and the tile's sums
template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsf_plan_kernel(const NsfArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    int64_t base;
    const int64_t n = nsf_list(a, b, &base);
    const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsfBatch<K> t(a, b);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    unsigned long long c[NSU_PER], d[NSU_PER], my_c = 0, my_d = 0;
    bool outside = false;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        c[k] = d[k] = 0;
        const int64_t p = p0 + k;
        if (p < n) {
            const int64_t v = a.nodes[base + p];
            int64_t e0 = 0;
            if ((uint64_t)v >= (uint64_t)a.n_major) {
                outside = true;
            } else {
                // a graph's ptrs are trusted to ascend inside [0, n_edges]; the clamp keeps `indices` in range anyway
                e0 = nsu_clamp(csc_ptr(a.ptrs, a.ptrs32, v), a.n_edges_graph);
                const int64_t e1 = std::max(e0, nsu_clamp(csc_ptr(a.ptrs, a.ptrs32, v + 1), a.n_edges_graph));
                d[k] = (unsigned long long)(e1 - e0);
                c[k] = (d[k] + CS_CHUNK - 1) / CS_CHUNK;
            }
            t.col0[p] = e0;
        }
        my_c += c[k], my_d += d[k];
    }
    if (outside) atomicOr(a.status, 2);
    unsigned long long total_c, total_d;
    unsigned long long run_c = nsu_scan64(my_c, s_wave, &total_c);
    unsigned long long run_d = nsu_scan64(my_d, s_wave, &total_d);
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        if (p0 + k < n) t.npref[p0 + k] = run_c, t.epref[p0 + k] = run_d;
        run_c += c[k], run_d += d[k];
    }
    if (threadIdx.x == 0) t.ntile[2 * blockIdx.x] = total_c, t.ntile[2 * blockIdx.x + 1] = total_d;
}

// adds the sums of the tiles before; the last tile closes both prefixes and takes the capacity decision
template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsf_node_apply_kernel(const NsfArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    int64_t base;
    const int64_t n = nsf_list(a, b, &base);
    const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const NsfBatch<K> t(a, b);
    // the chunk and the triple sums of the tiles before, interleaved in ntile: one pass, so not cs_tiles_before twice
    unsigned long long before_c = 0, before_d = 0, base_c, base_d;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += CS_THREADS) before_c += t.ntile[2 * i], before_d += t.ntile[2 * i + 1];
    nsu_scan64(before_c, s_wave, &base_c);
    nsu_scan64(before_d, s_wave, &base_d);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k)
        if (p0 + k < n) t.npref[p0 + k] += base_c, t.epref[p0 + k] += base_d;
    if (tile0 + CS_TILE >= n && threadIdx.x == 0) { // the batch's last tile (tile 0 of an empty batch)
        const unsigned long long n_chunks = base_c + t.ntile[2 * blockIdx.x], m = base_d + t.ntile[2 * blockIdx.x + 1];
        t.npref[n] = n_chunks, t.epref[n] = m;
        a.n_edges[b] = (int64_t)m;
        if (a.chunks) a.chunks[b] = (int64_t)n_chunks;
        const unsigned long long distinct = (unsigned long long)n + std::min<unsigned long long>(m, (unsigned long long)a.id_bound);
        if (distinct > (unsigned long long)a.node_cap || n_chunks > (unsigned long long)a.chunk_bound || m >= NSF_MAX_EDGES) {
            atomicOr(a.status, 1);
            t.hdr[0] = 0, t.hdr[1] = 0;
        } else {
            t.hdr[0] = n_chunks, t.hdr[1] = 1;
        }
    }
}

// the four scans over the batch's chunks (the file's head comment)
template <typename K, bool I32, int MODE> __global__ void __launch_bounds__(CS_THREADS) nsf_scan_kernel(const NsfArgs a) {
    const int64_t b = blockIdx.y;
    const NsfBatch<K> t(a, b);
    if (t.hdr[1] == 0) return; // refused: uniform
    const unsigned long long n_chunks = t.hdr[0];
    int64_t base;
    const int64_t n = nsf_list(a, b, &base);
    if (MODE == NSF_INSERT && n_chunks) { // the frontier: value = position (nobody looks a batch without triples up)
        for (int64_t p = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * CS_THREADS) {
            const int64_t v = a.nodes[base + p];
            if ((uint64_t)v < (uint64_t)a.id_bound) { // any other word equals no source
                const uint32_t s = nsu_insert<K, true>(t.keys, a.cap_mask, a.hash_shift, (K)v);
                atomicMin(&t.vals[s], (uint32_t)p);
            }
        }
    }
    if (MODE == NSF_NODES && a.nodes_out) {
        int64_t *out = a.nodes_out + a.node_off[b];
        for (int64_t p = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * CS_THREADS)
            out[p] = a.nodes[base + p];
    }
    if (n_chunks == 0) return; // uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = CS_THREADS / 64;
    int unit = CS_UNIT;
    while (unit > 1 && cs_short_fill(n_chunks, unit, gridDim.x, waves)) unit >>= 1;
    const unsigned long long n_units = (n_chunks + unit - 1) / unit;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    int64_t *nodes_out = MODE == NSF_NODES && a.nodes_out ? a.nodes_out + a.node_off[b] : nullptr;
    const int64_t out0 = MODE == NSF_TRIPLES ? a.edge_off[b] : 0;
    for (unsigned long long u = (unsigned long long)blockIdx.x * waves + wave; u < n_units; u += (unsigned long long)gridDim.x * waves) {
        const unsigned long long c = u * unit + lane;
        long long my_i = 0, my_e0 = 0, my_k0 = 0;
        int my_len = 0;
        if (lane < unit && c < n_chunks) {
            const int64_t lo = cs_last_le(t.npref, n, c); // npref[0] = 0 <= c < n_chunks = npref[n]; it has chunks
            const long long rel = (long long)(c - t.npref[lo]) * CS_CHUNK;
            const long long k_lo = (long long)t.epref[lo];
            my_i = lo;
            my_e0 = t.col0[lo] + rel;
            my_k0 = k_lo + rel;
            my_len = (int)std::min<long long>(CS_CHUNK, (long long)t.epref[lo + 1] - my_k0);
        }
        uint32_t unit_new = 0;
        for (int q = 0; q < unit; ++q) {
            const unsigned long long cq = u * unit + q;
            if (cq >= n_chunks) break; // uniform
            const long long i = __shfl(my_i, q), e0 = __shfl(my_e0, q), k0 = __shfl(my_k0, q);
            const int len = __shfl(my_len, q);
            const uint32_t pos0 = MODE == NSF_NODES ? (uint32_t)n + t.cpref[cq] : 0;
            // the chunk's new nodes as pass 1 counted them: a workspace that is not pass 1's (a second emit) stays in range
            const uint32_t room = MODE == NSF_NODES ? t.cpref[cq + 1] - t.cpref[cq] : 0;
            uint32_t cnt = 0;
            for (int s = 0; s < len; s += 64) {
                const bool valid = s + lane < len;
                const int64_t e = e0 + s + lane;
                const uint32_t mark = (uint32_t)(n + k0 + s + lane); // n + k: below 2^30 + 2^31
                int64_t src = 0;
                if (valid) src = I32 ? (int64_t)a.indices32[e] : a.indices[e];
                if (MODE == NSF_INSERT) {
                    if (valid) {
                        const uint32_t slot = nsu_insert<K, true>(t.keys, a.cap_mask, a.hash_shift, (K)src);
                        atomicMin(&t.vals[slot], mark);
                    }
                } else if (MODE == NSF_TRIPLES) {
                    if (valid) {
                        const uint32_t slot = cs_find<false, true>(t.keys, t.vals, a.cap_mask, a.hash_shift, (K)src);
                        const int64_t o = out0 + k0 + s + lane;
                        a.rows[o] = slot != NSU_UNSEEN ? (int64_t)t.vals[slot] : -1;
                        a.cols[o] = i;
                        a.edge_index[o] = e;
                    }
                } else {
                    uint32_t slot = NSU_UNSEEN;
                    if (valid) slot = cs_find<false, true>(t.keys, t.vals, a.cap_mask, a.hash_shift, (K)src);
                    const bool first = slot != NSU_UNSEEN && t.vals[slot] == mark;
                    const unsigned long long firsts = __ballot(first);
                    const uint32_t rank = cnt + (uint32_t)__popcll(firsts & below);
                    if (MODE == NSF_NODES && first && rank < room) {
                        const uint32_t pos = pos0 + rank;
                        if (nodes_out) nodes_out[pos] = src;
                        t.vals[slot] = pos; // <= mark: the source's other entries stay unflagged
                    }
                    cnt += (uint32_t)__popcll(firsts);
                }
            }
            if (MODE == NSF_FLAG) {
                if (lane == 0) t.cpref[cq] = cnt;
                unit_new += cnt;
            }
        }
        if (MODE == NSF_FLAG) cs_unit_counted(t.ctile, u, unit, unit_new, lane);
    }
}

// the exclusive prefix over a tile of chunks, in place; the last tile writes n_out_b (0 for a refused batch)
template <typename K> __global__ void __launch_bounds__(CS_THREADS) nsf_chunk_apply_kernel(const NsfArgs a) {
    __shared__ uint32_t s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    const NsfBatch<K> t(a, b);
    const unsigned long long n_chunks = t.hdr[0];
    if (cs_tile_idle(n_chunks)) return;
    const CsTile<uint32_t> r = cs_chunk_apply_tile(t.cpref, t.ctile, n_chunks, s_wave);
    if (r.last && threadIdx.x == 0) {
        int64_t list;
        const int64_t n = nsf_list(a, b, &list);
        t.cpref[n_chunks] = r.base + r.total;
        a.n_nodes[b] = t.hdr[1] ? n + (int64_t)(r.base + r.total) : 0;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct NsfPlan {
    NsuPlan table;
    int64_t chunk_bound, node_tiles, chunk_tiles;
    int64_t vals_off, npref_off, epref_off, col0_off, ntile_off, cpref_off, ctile_off, batch_bytes;
};

static int nsf_plan(const tg_graph *csc, const tg_ns_full_in *in, int64_t id_bound, const char *who, NsfPlan &pl) {
    TG_REQUIRE(csc && in, "%s: null argument", who);
    TG_REQUIRE(in->max_nodes >= 0 && in->max_nodes <= NSU_MAX_NODES, "%s: max_nodes = %lld outside [0, 2^30]", who,
               (long long)in->max_nodes);
    TG_REQUIRE(in->node_cap >= in->max_nodes && in->node_cap <= NSU_MAX_NODES, "%s: node_cap = %lld outside [max_nodes = %lld, 2^30]",
               who, (long long)in->node_cap, (long long)in->max_nodes);
    // a frontier of distinct nodes has disjoint columns, the ones of cs_plan_chunks' default bound
    if (const int rc = cs_plan_chunks(csc, in->max_nodes, in->chunk_cap, who, pl.chunk_bound, pl.chunk_tiles)) return rc;
    if (const int rc = nsu_plan(in->node_cap, id_bound, who, pl.table)) return rc; // id_bound >= 1, the key width, the table
    TG_REQUIRE(id_bound >= csc->n_major, "%s: id_bound = %lld below n_major = %lld", who, (long long)id_bound,
               (long long)csc->n_major);
    const int64_t pitch = in->max_nodes;
    pl.node_tiles = pitch > 0 ? (pitch + CS_TILE - 1) / CS_TILE : 1;
    pl.vals_off = CS_HEADER + nsu_r256(pl.table.table_cap * pl.table.key_bytes);
    pl.npref_off = pl.vals_off + nsu_r256(pl.table.table_cap * 4);
    pl.epref_off = pl.npref_off + nsu_r256((pitch + 1) * 8);
    pl.col0_off = pl.epref_off + nsu_r256((pitch + 1) * 8);
    pl.ntile_off = pl.col0_off + nsu_r256(pitch * 8);
    pl.cpref_off = pl.ntile_off + nsu_r256(pl.node_tiles * 16);
    pl.ctile_off = pl.cpref_off + nsu_r256((pl.chunk_bound + 1) * 4);
    pl.batch_bytes = pl.ctile_off + nsu_r256(pl.chunk_tiles * 4);
    return TG_OK;
}

// what both passes check alike, and the kernel arguments of batch 0
static int nsf_common(const tg_graph *csc, const tg_ns_full_in *in, int64_t n_batches, int64_t id_bound, void *workspace,
                      int64_t workspace_bytes, const char *who, NsfPlan &pl, NsfArgs &a) {
    if (const int rc = nsf_plan(csc, in, id_bound, who, pl)) return rc;
    if (n_batches >= 0 && n_batches <= 0x7fffffff) // the text this pair has always refused such a launch with
        if (const int rc = cs_bytes_fit(pl.batch_bytes, n_batches, who)) return rc;
    if (const int rc = cs_check_launch(csc, n_batches, pl.batch_bytes, workspace, workspace_bytes, who)) return rc;
    TG_REQUIRE(in->node_ptr, "%s: null node_ptr", who);
    TG_REQUIRE(in->nodes || in->max_nodes == 0, "%s: null nodes", who);
    a = NsfArgs{};
    a.ptrs = csc->ptrs, a.indices = csc->indices, a.ptrs32 = csc->ptrs32, a.indices32 = csc->indices32;
    a.n_major = csc->n_major, a.n_edges_graph = csc->n_edges;
    a.nodes = in->nodes, a.node_ptr = in->node_ptr;
    a.max_nodes = in->max_nodes, a.node_cap = in->node_cap, a.id_bound = id_bound;
    a.ws = static_cast<unsigned char *>(workspace);
    a.batch_bytes = pl.batch_bytes, a.vals_off = pl.vals_off, a.npref_off = pl.npref_off, a.epref_off = pl.epref_off;
    a.col0_off = pl.col0_off, a.ntile_off = pl.ntile_off, a.cpref_off = pl.cpref_off, a.ctile_off = pl.ctile_off;
    a.chunk_bound = pl.chunk_bound, a.table_cap = pl.table.table_cap, a.chunk_tiles = pl.chunk_tiles;
    nsu_mask_shift(pl.table.table_cap, a.cap_mask, a.hash_shift);
    return TG_OK;
}

// the arguments of the round that starts at batch b0
static NsfArgs nsf_at(const NsfArgs &a0, int64_t b0) {
    NsfArgs a = a0;
    a.node_ptr += b0, a.ws += b0 * a.batch_bytes;
    if (a.n_nodes) a.n_nodes += b0;
    if (a.n_edges) a.n_edges += b0;
    if (a.chunks) a.chunks += b0;
    if (a.node_off) a.node_off += b0;
    if (a.edge_off) a.edge_off += b0;
    return a;
}

template <typename K, int MODE> static int nsf_launch_scan(const NsfArgs &a, int64_t nb, hipStream_t stream) {
    const dim3 grid(cs_scan_grid(nb), (unsigned)nb), block(CS_THREADS);
    if (a.indices32)
        hipLaunchKernelGGL((nsf_scan_kernel<K, true, MODE>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((nsf_scan_kernel<K, false, MODE>), grid, block, 0, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <typename K> static int nsf_count(const NsfArgs &a0, const NsfPlan &pl, int64_t n_batches, hipStream_t stream) {
    const dim3 block(CS_THREADS);
    const int64_t clear_blocks = (std::max(pl.table.table_cap, pl.chunk_tiles) + CS_THREADS - 1) / CS_THREADS;
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb_) {
        const NsfArgs a = nsf_at(a0, b0);
        const unsigned nb = (unsigned)nb_;
        hipLaunchKernelGGL(nsf_clear_kernel<K>, dim3((unsigned)std::min<int64_t>(clear_blocks, 1024), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        hipLaunchKernelGGL(nsf_plan_kernel<K>, dim3((unsigned)pl.node_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        hipLaunchKernelGGL(nsf_node_apply_kernel<K>, dim3((unsigned)pl.node_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        if (const int rc = nsf_launch_scan<K, NSF_INSERT>(a, nb_, stream)) return rc;
        if (const int rc = nsf_launch_scan<K, NSF_FLAG>(a, nb_, stream)) return rc;
        hipLaunchKernelGGL(nsf_chunk_apply_kernel<K>, dim3((unsigned)pl.chunk_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        return (int)TG_OK;
    });
}

template <typename K> static int nsf_emit(const NsfArgs &a0, int64_t n_batches, hipStream_t stream) {
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb) {
        const NsfArgs a = nsf_at(a0, b0);
        if (const int rc = nsf_launch_scan<K, NSF_NODES>(a, nb, stream)) return rc;
        return nsf_launch_scan<K, NSF_TRIPLES>(a, nb, stream);
    });
}

} // namespace tg

extern "C" int tg_ns_full_workspace_bytes(const tg_graph *csc, const tg_ns_full_in *in, int64_t id_bound, int64_t n_batches,
                                          int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ns_full_workspace_bytes";
    NsfPlan pl;
    if (const int rc = nsf_plan(csc, in, id_bound, who, pl)) return rc;
    return cs_answer_bytes(pl.batch_bytes, n_batches, who, bytes, bytes_min);
}

extern "C" int tg_ns_full_count(const tg_graph *csc, const tg_ns_full_in *in, int64_t n_batches, int64_t id_bound,
                                int64_t *n_nodes, int64_t *n_edges, int64_t *chunks, int32_t *status, void *workspace,
                                int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_full_count";
    NsfPlan pl;
    NsfArgs a0;
    if (const int rc = nsf_common(csc, in, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(n_nodes && n_edges && status, "%s: null n_nodes / n_edges / status", who);
    a0.n_nodes = n_nodes, a0.n_edges = n_edges, a0.chunks = chunks, a0.status = status;
    hipStream_t stream = (hipStream_t)stream_;
    return pl.table.key_bytes == 4 ? nsf_count<nsu_k32>(a0, pl, n_batches, stream) : nsf_count<nsu_k64>(a0, pl, n_batches, stream);
}

extern "C" int tg_ns_full_emit(const tg_graph *csc, const tg_ns_full_in *in, int64_t n_batches, int64_t id_bound,
                               const int64_t *node_off, const int64_t *edge_off, int64_t *nodes_out, int64_t *rows, int64_t *cols,
                               int64_t *edge_index, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ns_full_emit";
    NsfPlan pl;
    NsfArgs a0;
    if (const int rc = nsf_common(csc, in, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(edge_off && rows && cols && edge_index, "%s: null edge_off / rows / cols / edge_index", who);
    TG_REQUIRE(node_off || !nodes_out, "%s: nodes_out given without node_off", who);
    a0.node_off = node_off, a0.edge_off = edge_off, a0.nodes_out = nodes_out, a0.rows = rows, a0.cols = cols;
    a0.edge_index = edge_index;
    hipStream_t stream = (hipStream_t)stream_;
    return pl.table.key_bytes == 4 ? nsf_emit<nsu_k32>(a0, n_batches, stream) : nsf_emit<nsu_k64>(a0, n_batches, stream);
}
