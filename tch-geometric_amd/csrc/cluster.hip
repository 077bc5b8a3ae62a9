// Cluster-GCN mini-batches (tg_cluster_count / tg_cluster_emit, include/tchgeo.h): the induced subgraph of a union of
// clusters of a fixed node partition, word for word what tg_ns_induced_* gives over the expanded node lists.
//
// After the caller's renumbering cluster c is the id range [partptr[c], partptr[c+1]), so a batch is at most
// TG_CLUSTER_MAX_PARTS_PER_BATCH ranges and three costs of the hash pair fall away:
//   - no hash table: local(u) = base_k + (u - partptr[c_k]) for the first k whose range holds u.  The batch's distinct
//     non-empty ranges, sorted by start, sit in LDS (start, end, base - start: 12 bytes a range, 12 KiB at most); a
//     neighbour costs one binary search there and no global access besides its own word of `indices`;
//   - no idle lanes: a cluster's columns are consecutive, so its CSC entries are ONE offset range [ptrs[lo], ptrs[hi]).
//     It is cut into chunks of CS_CHUNK = 512 consecutive offsets that run across column boundaries; a wave takes 64
//     consecutive offsets a step whatever the columns' lengths.  A hub column is still split over many chunks;
//   - no node list: the positions are implied by the cluster list and are written once, by pass 2.
//
// The column of an offset (pass 2 only, and only for a hit): the lane that looks a chunk up searches `ptrs` once for the
// chunk's first column; after that the wave keeps a window of the next 64 column ends, one per lane, and an entry's column
// is the window's first column plus the number of ends <= its offset, an upper bound over the wave's 64 ascending words by
// __shfl (7 steps, no memory).  A window all of whose ends are passed moves on 64 columns (runs of empty columns, or many
// steps without a hit); offsets only grow, so it never moves back.  At degree 16 that is one load of `ptrs` per chunk.
// A chunk's 8 x 64 entries are loaded up front, so that their latencies overlap.
//
// Pass 1: plan (one workgroup per batch: ranges, base_k, the chunk prefix per cluster, the sort + dedup of (start, k),
//   the bounds that raise the status bits) | scan: hits per chunk, summed per tile of chunks | chunk apply: the exclusive
//   prefix over chunks in place, m_b.  Pass 2: nodes | scan again, a chunk's hits go to edge_off[b] + its prefix, ranked
//   in lane order = offset order by ballot + popcount.  The chunk size, the cpref / ctile scheme and the units of up to
//   16 chunks with their look-ups in lanes 0..15 are chunk_scan.h's; the unit shrinks by cs_short_fill.
#include "chunk_scan.h"

namespace tg {

constexpr int CL_MAX_PARTS = TG_CLUSTER_MAX_PARTS_PER_BATCH;
constexpr int CL_PER = CL_MAX_PARTS / CS_THREADS;    // list entries a plan thread owns
// the header's words: {chunks, n_b, list entries, table ranges} (0 on overflow)
static_assert(CL_MAX_PARTS % CS_THREADS == 0 && (CL_MAX_PARTS & (CL_MAX_PARTS - 1)) == 0, "the plan's sort is bitonic");

struct ClArgs {
    const int64_t *ptrs, *indices;
    const uint32_t *ptrs32, *indices32;
    int64_t n_major, n_edges_graph;
    const int64_t *partptr, *clusters, *n_clusters, *node_ids; // clusters / n_clusters: batch 0 of the launch
    int64_t n_parts, pitch;
    int64_t *n_nodes, *n_edges;                                // pass 1
    int32_t *status;
    const int64_t *node_off, *edge_off;                        // pass 2
    int64_t *nodes, *rows, *cols, *edge_index;
    unsigned char *ws;
    int64_t batch_bytes, e0_off, cpk_off, tab_off, cpref_off, ctile_off, chunk_bound, chunk_tiles;
};

// a batch's part of the workspace
struct ClBatch {
    unsigned long long *hdr, *cpref, *ctile;
    long long *e0, *e1;                     // [pitch] the cluster's offset range
    uint32_t *start, *size, *base, *cpk;    // [pitch] in list order; cpk [pitch + 1]: chunks before entry k
    uint32_t *t_start, *t_end, *t_delta;    // [pitch] the sorted distinct non-empty ranges
    __device__ __forceinline__ ClBatch(const ClArgs &a, int64_t b) {
        unsigned char *p = a.ws + b * a.batch_bytes;
        hdr = reinterpret_cast<unsigned long long *>(p);
        e0 = reinterpret_cast<long long *>(p + a.e0_off);
        e1 = e0 + a.pitch;
        cpk = reinterpret_cast<uint32_t *>(p + a.cpk_off);
        start = cpk + a.pitch + 1, size = start + a.pitch, base = size + a.pitch;
        t_start = reinterpret_cast<uint32_t *>(p + a.tab_off);
        t_end = t_start + a.pitch, t_delta = t_end + a.pitch;
        cpref = reinterpret_cast<unsigned long long *>(p + a.cpref_off); // [chunk_bound + 1] hits of / before a chunk
        ctile = reinterpret_cast<unsigned long long *>(p + a.ctile_off); // [chunk tiles]
    }
};

// one workgroup per batch
__global__ void __launch_bounds__(CS_THREADS) cl_plan_kernel(const ClArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    __shared__ unsigned long long s_key[CL_MAX_PARTS];
    __shared__ uint32_t s_size[CL_MAX_PARTS], s_base[CL_MAX_PARTS];
    const int64_t b = blockIdx.y;
    const ClBatch t(a, b);
    const int tid = threadIdx.x;
    const int q = (int)(a.n_clusters ? nsu_clamp(a.n_clusters[b], a.pitch) : a.pitch);
    const int64_t *list = a.clusters + b * a.pitch;
    for (int64_t s = tid; s < a.chunk_tiles; s += CS_THREADS) t.ctile[s] = 0;
    int64_t lo[CL_PER], hi[CL_PER], e0[CL_PER], e1[CL_PER];
    unsigned long long nch[CL_PER], my_n = 0, my_c = 0;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < CL_PER; ++j) {
        const int k = tid * CL_PER + j;
        lo[j] = hi[j] = e0[j] = e1[j] = 0;
        nch[j] = 0;
        if (k < q) {
            const int64_t c = list[k];
            if ((uint64_t)c >= (uint64_t)a.n_parts) {
                bad |= 2;
            } else {
                const int64_t p0 = a.partptr[c], p1 = a.partptr[c + 1];
                if (p0 < 0 || p1 > a.n_major || p0 > p1) {
                    bad |= 4;
                } else if (p1 > p0) {
                    lo[j] = p0, hi[j] = p1;
                    // a graph's ptrs are trusted to ascend inside [0, n_edges]; the clamp keeps `indices` in range anyway
                    e0[j] = nsu_clamp(csc_ptr(a.ptrs, a.ptrs32, p0), a.n_edges_graph);
                    e1[j] = std::max(e0[j], nsu_clamp(csc_ptr(a.ptrs, a.ptrs32, p1), a.n_edges_graph));
                    nch[j] = (unsigned long long)((e1[j] - e0[j] + CS_CHUNK - 1) / CS_CHUNK);
                }
            }
        }
        my_n += (unsigned long long)(hi[j] - lo[j]);
        my_c += nch[j];
    }
    if (bad) atomicOr(a.status, bad);
    unsigned long long n_b, n_chunks;
    unsigned long long run_n = nsu_scan64(my_n, s_wave, &n_b);
    unsigned long long run_c = nsu_scan64(my_c, s_wave, &n_chunks);
    const bool overflow = n_chunks > (unsigned long long)a.chunk_bound || n_b >= ((unsigned long long)1 << 31);
    if (overflow) { // uniform
        if (tid == 0) {
            atomicOr(a.status, 1);
            t.hdr[0] = t.hdr[1] = t.hdr[2] = t.hdr[3] = 0;
            a.n_nodes[b] = 0;
        }
        return;
    }
    int ns = 2; // the sort's width
    while (ns < q) ns <<= 1;
#pragma unroll
    for (int j = 0; j < CL_PER; ++j) {
        const int k = tid * CL_PER + j;
        if (k < ns) {
            s_size[k] = (uint32_t)(hi[j] - lo[j]);
            s_base[k] = (uint32_t)run_n;
            s_key[k] = hi[j] > lo[j] ? ((unsigned long long)lo[j] << 32) | (unsigned)k : ~0ull; // empty ranges sort last
        }
        if (k < q) {
            t.start[k] = (uint32_t)lo[j], t.size[k] = (uint32_t)(hi[j] - lo[j]), t.base[k] = (uint32_t)run_n;
            t.cpk[k] = (uint32_t)run_c;
            t.e0[k] = e0[j], t.e1[k] = e1[j];
        }
        run_n += (unsigned long long)(hi[j] - lo[j]);
        run_c += nch[j];
    }
    if (tid == 0) t.cpk[q] = (uint32_t)n_chunks;
    __syncthreads();
    for (int k2 = 2; k2 <= ns; k2 <<= 1) {
        for (int d = k2 >> 1; d > 0; d >>= 1) {
            for (int i = tid; i < ns; i += CS_THREADS) {
                const int o = i ^ d;
                if (o > i) {
                    const unsigned long long x = s_key[i], y = s_key[o];
                    if ((x > y) == ((i & k2) == 0)) s_key[i] = y, s_key[o] = x;
                }
            }
            __syncthreads();
        }
    }
    // the table: of the entries with one start (one cluster named again) the first in list order
    unsigned long long keep[CL_PER], mine = 0, n_tab;
#pragma unroll
    for (int j = 0; j < CL_PER; ++j) {
        const int i = tid * CL_PER + j;
        keep[j] = 0;
        if (i < ns && s_key[i] != ~0ull) keep[j] = i == 0 || (s_key[i - 1] >> 32) != (s_key[i] >> 32);
        mine += keep[j];
    }
    unsigned long long r = nsu_scan64(mine, s_wave, &n_tab);
#pragma unroll
    for (int j = 0; j < CL_PER; ++j) {
        if (keep[j]) {
            const unsigned long long key = s_key[tid * CL_PER + j];
            const uint32_t st = (uint32_t)(key >> 32), k = (uint32_t)key;
            t.t_start[r] = st, t.t_end[r] = st + s_size[k], t.t_delta[r] = s_base[k] - st;
            ++r;
        }
    }
    if (tid == 0) {
        t.hdr[0] = n_chunks, t.hdr[1] = n_b, t.hdr[2] = (unsigned long long)q, t.hdr[3] = n_tab;
        a.n_nodes[b] = (int64_t)n_b;
    }
}

// the ends of columns vb + 1 .. vb + 64 relative to offset e_begin, one per lane, ascending in the lane; columns past the
// cluster's last one read ptrs[hi], which is above every offset of the cluster.  Clamped so that an int holds it
__device__ __forceinline__ int cl_ends(const ClArgs &a, long long vb, long long hi, long long e_begin, int lane) {
    const long long d = csc_ptr(a.ptrs, a.ptrs32, std::min<long long>(vb + 1 + lane, hi)) - e_begin;
    return (int)std::max<long long>(-1, std::min<long long>(d, 2 * CS_CHUNK));
}

// how many of the wavefront's 64 ascending words `rel` are <= t: an upper bound by lane exchanges.  Every lane calls it
__device__ __forceinline__ int cl_upper_bound(int rel, int t) {
    int n = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1)
        if (__shfl(rel, n + step - 1) <= t) n += step;
    if (__shfl(rel, n) <= t) ++n;
    return n;
}

// EMIT = false: hits per chunk (and their sum per tile of chunks); true: the hits themselves
template <bool I32, bool EMIT> __global__ void __launch_bounds__(CS_THREADS) cl_scan_kernel(const ClArgs a) {
    __shared__ uint32_t s_start[CL_MAX_PARTS], s_end[CL_MAX_PARTS], s_delta[CL_MAX_PARTS];
    const int64_t b = blockIdx.y;
    const ClBatch t(a, b);
    const unsigned long long n_chunks = t.hdr[0];
    if (n_chunks == 0) return; // uniform
    const int q = (int)t.hdr[2], n_tab = (int)t.hdr[3]; // chunks: n_tab >= 1
    for (int i = threadIdx.x; i < n_tab; i += CS_THREADS) s_start[i] = t.t_start[i], s_end[i] = t.t_end[i], s_delta[i] = t.t_delta[i];
    __syncthreads();
    const uint32_t first = s_start[0], last = s_end[n_tab - 1]; // the table's span: most neighbours fall outside it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = CS_THREADS / 64;
    int unit = CS_UNIT;
    while (unit > 1 && cs_short_fill(n_chunks, unit, gridDim.x, waves)) unit >>= 1;
    const unsigned long long n_units = (n_chunks + unit - 1) / unit;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    const int64_t out0 = EMIT ? a.edge_off[b] : 0;
    for (unsigned long long u = (unsigned long long)blockIdx.x * waves + wave; u < n_units; u += (unsigned long long)gridDim.x * waves) {
        const unsigned long long c = u * unit + lane;
        long long my_e = 0, my_v = 0, my_hi = 0, my_i0 = 0;
        int my_len = 0;
        if (lane < unit && c < n_chunks) {
            const int k = cs_last_le(t.cpk, q, c); // the list entry: cpk[0] = 0 <= c < n_chunks = cpk[q]; it has chunks
            my_e = t.e0[k] + (int64_t)(c - t.cpk[k]) * CS_CHUNK;
            my_len = (int)std::min<int64_t>(CS_CHUNK, t.e1[k] - my_e);
            if (EMIT) { // pass 1 counts hits and needs no column
                const int64_t lo = t.start[k], hi = lo + t.size[k];
                // the chunk's first column: the last v in [lo, hi) with ptrs[v] <= my_e (ptrs[lo] <= my_e < ptrs[hi])
                int64_t v = lo, vh = hi;
                while (vh - v > 1) {
                    const int64_t mid = (v + vh) >> 1;
                    if (csc_ptr(a.ptrs, a.ptrs32, mid) <= my_e) v = mid; else vh = mid;
                }
                my_v = v, my_hi = hi;
                my_i0 = (long long)t.base[k] - lo; // position = column + my_i0
            }
        }
        unsigned long long unit_hits = 0;
        for (int w = 0; w < unit; ++w) {
            const unsigned long long cw = u * unit + w;
            if (cw >= n_chunks) break; // uniform
            const long long e_begin = __shfl(my_e, w);
            const int len = __shfl(my_len, w);
            uint32_t nbr[CS_CHUNK / 64]; // the chunk's entries, all loads in flight at once
#pragma unroll
            for (int j = 0; j < CS_CHUNK / 64; ++j) {
                const int o = j * 64 + lane;
                nbr[j] = 0;
                if (o < len) nbr[j] = I32 ? a.indices32[e_begin + o] : (uint32_t)a.indices[e_begin + o];
            }
            // pass 2: the window of 64 column ends from column vb on.  An entry's column is vb + the ends <= its offset while
            // fewer than all 64 are; else the window moves on 64 columns.  Offsets only grow, so it never has to move back
            const long long hi = EMIT ? __shfl(my_hi, w) : 0, i0 = EMIT ? __shfl(my_i0, w) : 0;
            long long vb = EMIT ? __shfl(my_v, w) : 0;
            int ends = 0;
            bool loaded = false;
            const int64_t out = EMIT ? out0 + (int64_t)t.cpref[cw] : 0;
            uint32_t cnt = 0;
#pragma unroll
            for (int j = 0; j < CS_CHUNK / 64; ++j) {
                if (j * 64 >= len) break; // uniform
                const int o = j * 64 + lane;
                uint32_t pos = NSU_UNSEEN;
                if (o < len && nbr[j] >= first && nbr[j] < last) {
                    int r = 0, rh = n_tab;
                    while (rh - r > 1) {
                        const int mid = (r + rh) >> 1;
                        if (s_start[mid] <= nbr[j]) r = mid; else rh = mid;
                    }
                    if (nbr[j] < s_end[r]) pos = nbr[j] + s_delta[r];
                }
                const unsigned long long hits = __ballot(pos != NSU_UNSEEN);
                if (EMIT && hits) { // uniform; only a hit needs its column
                    if (!loaded) ends = cl_ends(a, vb, hi, e_begin, lane), loaded = true;
                    long long col = 0;
                    bool done = pos == NSU_UNSEEN;
                    for (;;) {
                        const int n = cl_upper_bound(ends, o);
                        if (!done && (n < 64 || vb + 64 >= hi)) col = vb + n, done = true;
                        if (__all(done)) break; // uniform
                        vb += 64;
                        ends = cl_ends(a, vb, hi, e_begin, lane);
                    }
                    if (pos != NSU_UNSEEN) {
                        const int64_t dst = out + cnt + __popcll(hits & below);
                        a.rows[dst] = (int64_t)pos;
                        a.cols[dst] = col + i0;
                        a.edge_index[dst] = e_begin + o;
                    }
                }
                cnt += (uint32_t)__popcll(hits);
            }
            if (!EMIT) {
                if (lane == 0) t.cpref[cw] = cnt;
                unit_hits += cnt;
            }
        }
        if (!EMIT) cs_unit_counted(t.ctile, u, unit, unit_hits, lane);
    }
}

// the exclusive prefix over a tile of chunks, in place; the last tile writes m_b
__global__ void __launch_bounds__(CS_THREADS) cl_chunk_apply_kernel(const ClArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    const ClBatch t(a, b);
    const unsigned long long n_chunks = t.hdr[0];
    if (cs_tile_idle(n_chunks)) return;
    const CsTile<unsigned long long> r = cs_chunk_apply_tile(t.cpref, t.ctile, n_chunks, s_wave);
    if (r.last && threadIdx.x == 0) {
        t.cpref[n_chunks] = r.base + r.total;
        a.n_edges[b] = (int64_t)(r.base + r.total);
    }
}

// position i of the batch is vertex start_k + (i - base_k): the node list, written once
__global__ void __launch_bounds__(CS_THREADS) cl_nodes_kernel(const ClArgs a) {
    const int64_t b = blockIdx.y;
    const ClBatch t(a, b);
    if (t.hdr[1] == 0) return;
    const int q = (int)t.hdr[2];
    int64_t *out = a.nodes + a.node_off[b];
    for (int k = blockIdx.x; k < q; k += gridDim.x) {
        const int64_t lo = t.start[k], n = t.size[k], base = t.base[k];
        for (int64_t i = threadIdx.x; i < n; i += CS_THREADS) out[base + i] = a.node_ids ? a.node_ids[lo + i] : lo + i;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct ClPlan {
    int64_t chunk_bound, chunk_tiles, e0_off, cpk_off, tab_off, cpref_off, ctile_off, batch_bytes;
};

static int cl_plan(const tg_graph *csc, int64_t n_parts, int64_t pitch, const char *who, ClPlan &pl) {
    TG_REQUIRE(pitch >= 0 && pitch <= CL_MAX_PARTS, "%s: pitch_parts = %lld outside [0, %d]", who, (long long)pitch, CL_MAX_PARTS);
    // distinct clusters have disjoint offset ranges, the columns of cs_plan_chunks' default bound
    if (const int rc = cs_plan_chunks(csc, pitch, 0, who, pl.chunk_bound, pl.chunk_tiles)) return rc;
    if (csc->n_major > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: n_major = %lld above 2^31: ranges and positions are 32-bit words", who,
                    (long long)csc->n_major);
    TG_REQUIRE(n_parts >= 0, "%s: n_parts = %lld is negative", who, (long long)n_parts);
    pl.e0_off = CS_HEADER;
    pl.cpk_off = pl.e0_off + nsu_r256(2 * pitch * 8);
    pl.tab_off = pl.cpk_off + nsu_r256((4 * pitch + 1) * 4);
    pl.cpref_off = pl.tab_off + nsu_r256(3 * pitch * 4);
    pl.ctile_off = pl.cpref_off + nsu_r256((pl.chunk_bound + 1) * 8);
    pl.batch_bytes = pl.ctile_off + nsu_r256(pl.chunk_tiles * 8);
    return TG_OK;
}

// what both passes check alike, and the kernel arguments of batch 0
static int cl_common(const tg_graph *csc, const tg_cluster_in *in, int64_t n_batches, void *workspace, int64_t workspace_bytes,
                     const char *who, ClPlan &pl, ClArgs &a) {
    TG_REQUIRE(csc && in, "%s: null argument", who);
    if (const int rc = cl_plan(csc, in->n_parts, in->pitch_parts, who, pl)) return rc;
    if (const int rc = cs_check_launch(csc, n_batches, pl.batch_bytes, workspace, workspace_bytes, who)) return rc;
    TG_REQUIRE(in->partptr, "%s: null partptr", who);
    TG_REQUIRE(in->clusters || in->pitch_parts == 0, "%s: null clusters", who);
    a = ClArgs{};
    a.ptrs = csc->ptrs, a.indices = csc->indices, a.ptrs32 = csc->ptrs32, a.indices32 = csc->indices32;
    a.n_major = csc->n_major, a.n_edges_graph = csc->n_edges;
    a.partptr = in->partptr, a.clusters = in->clusters, a.n_clusters = in->n_clusters, a.node_ids = in->node_ids;
    a.n_parts = in->n_parts, a.pitch = in->pitch_parts;
    a.ws = static_cast<unsigned char *>(workspace);
    a.batch_bytes = pl.batch_bytes, a.e0_off = pl.e0_off, a.cpk_off = pl.cpk_off, a.tab_off = pl.tab_off;
    a.cpref_off = pl.cpref_off, a.ctile_off = pl.ctile_off, a.chunk_bound = pl.chunk_bound, a.chunk_tiles = pl.chunk_tiles;
    return TG_OK;
}

// the arguments of the launch that starts at batch b0
static ClArgs cl_at(const ClArgs &a0, int64_t b0) {
    ClArgs a = a0;
    a.ws += b0 * a.batch_bytes;
    if (a.clusters) a.clusters += b0 * a.pitch;
    if (a.n_clusters) a.n_clusters += b0;
    if (a.n_nodes) a.n_nodes += b0;
    if (a.n_edges) a.n_edges += b0;
    if (a.node_off) a.node_off += b0;
    if (a.edge_off) a.edge_off += b0;
    return a;
}

} // namespace tg

extern "C" int tg_cluster_workspace_bytes(const tg_graph *csc, int64_t n_parts, int64_t pitch_parts, int64_t n_batches,
                                          int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_cluster_workspace_bytes";
    ClPlan pl;
    if (const int rc = cl_plan(csc, n_parts, pitch_parts, who, pl)) return rc;
    return cs_answer_bytes(pl.batch_bytes, n_batches, who, bytes, bytes_min);
}

extern "C" int tg_cluster_count(const tg_graph *csc, const tg_cluster_in *in, int64_t n_batches, int64_t *n_nodes,
                                int64_t *n_edges, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_cluster_count";
    ClPlan pl;
    ClArgs a0;
    if (const int rc = cl_common(csc, in, n_batches, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(n_nodes && n_edges && status, "%s: null n_nodes / n_edges / status", who);
    a0.n_nodes = n_nodes, a0.n_edges = n_edges, a0.status = status;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 block(CS_THREADS);
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb_) {
        const ClArgs a = cl_at(a0, b0);
        const unsigned nb = (unsigned)nb_;
        hipLaunchKernelGGL(cl_plan_kernel, dim3(1, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        if (a.indices32)
            hipLaunchKernelGGL((cl_scan_kernel<true, false>), dim3(cs_scan_grid(nb_), nb), block, 0, stream, a);
        else
            hipLaunchKernelGGL((cl_scan_kernel<false, false>), dim3(cs_scan_grid(nb_), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        hipLaunchKernelGGL(cl_chunk_apply_kernel, dim3((unsigned)pl.chunk_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        return (int)TG_OK;
    });
}

extern "C" int tg_cluster_emit(const tg_graph *csc, const tg_cluster_in *in, int64_t n_batches, const int64_t *node_off,
                               const int64_t *edge_off, int64_t *nodes, int64_t *rows, int64_t *cols, int64_t *edge_index,
                               void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_cluster_emit";
    ClPlan pl;
    ClArgs a0;
    if (const int rc = cl_common(csc, in, n_batches, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(edge_off && rows && cols && edge_index, "%s: null edge_off / rows / cols / edge_index", who);
    TG_REQUIRE(node_off || !nodes, "%s: nodes given without node_off", who);
    a0.node_off = node_off, a0.edge_off = edge_off, a0.nodes = nodes, a0.rows = rows, a0.cols = cols, a0.edge_index = edge_index;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 block(CS_THREADS);
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb_) {
        const ClArgs a = cl_at(a0, b0);
        const unsigned nb = (unsigned)nb_;
        if (a.nodes && a.pitch > 0) {
            const unsigned gx = (unsigned)std::min<int64_t>(a.pitch, std::max<int64_t>(1, CS_SCAN_BLOCKS / nb_));
            hipLaunchKernelGGL(cl_nodes_kernel, dim3(gx, nb), block, 0, stream, a);
            TG_LAUNCH_CHECK();
        }
        if (a.indices32)
            hipLaunchKernelGGL((cl_scan_kernel<true, true>), dim3(cs_scan_grid(nb_), nb), block, 0, stream, a);
        else
            hipLaunchKernelGGL((cl_scan_kernel<false, true>), dim3(cs_scan_grid(nb_), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        return (int)TG_OK;
    });
}
