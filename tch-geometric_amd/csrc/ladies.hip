// Layer-wise importance sampling (tg_ladies_count / tg_ladies_emit, include/tchgeo_ladies.h): ONE budget of s nodes per
// layer for a whole mini-batch, FastGCN's with-replacement estimator under LADIES' layer-dependent law.
//
// The rule, per batch with frontier v_0 .. v_{n-1} (columns, triple order and out-of-range ids are tg_ns_full_*'s): triple k
// in (i, e) ascending order is (src = indices[e], col = i, e).  Entry weights: without `weights` q_e = max(1, 2^40 / (d_i *
// d_i)) in u64 division and w_e = 1.0 / (double)d_i (the row-normalised adjacency); with them x = (double)weights[e], q_e = 0
// unless x > 0, else (uint64)floor(min(x, 1.0)^2 * 2^32), and w_e = x.  Candidates = the distinct sources in order of first
// occurrence in triple order (the frontier is not pre-inserted); W_u = the sum of q_e over the entries of source u (64-bit
// integer atomic adds, so the order does not matter; parallel entries count separately); P = the exclusive prefix of W in
// candidate order, S = the total (max_nodes <= 2^22 and m_b < 2^31 keep S < 2^63).  Slot j of 0 .. s-1 takes one Philox
// block, draw(call key of (seed, call_id + b, TG_TAG_LADIES), id = j, 0, 0), t = floor(lo * S / 2^64) by a 128-bit product, and
// selects the one candidate with P_u <= t < P_u + W_u; c_u = the slots that selected u.  out_nodes = the frontier followed
// by every selected candidate that is no frontier node, ordered by its first selecting slot; node_count = c, node_weight
// = W per position; kept triples = those with c_src > 0 in triple order, row = the first position of src in out_nodes, and
// edge_weight = (float)(((double)c * (double)S) / ((double)s * (double)W) * w_e), five single IEEE operations (the library is
// built with -ffp-contract=off).  E[c_u] = s W_u / S, so a column's kept edges sum to an unbiased estimate of its full row.
// Sampling is WITH replacement: LADIES' own code samples without replacement and rescales by 1/p, which is biased; this
// form is unbiased and integer until the last step, so the operator is a function of (graph, frontiers, seed, call id).
//
// The machinery is chunk_scan.h's (columns cut into chunks of 512 offsets, a wave takes a unit of chunks, a hub column is
// many chunks all over the device) over ns_unique.h's table, whose slot carries five words here: the key, `first` (the
// first triple that names it, atomicMin), `pos` (the first frontier position of the id, later the position in out_nodes),
// W (atomicAdd, 64 bits) and `cnt` (c, by the draw).  The draw's dedup runs in LDS on saint_dedup.h's plan of s positions.
//
// Pass 1: clear | plan + node apply (ns_full's: column begin, chunks and triples before a position; the capacity decision)
//   | INSERT scan: the frontier with pos = i, every entry with first = k and W += q (q of the row-normalised mode is
//   computed once per chunk by the look-up lane) | FLAG scan: an entry is a candidate's first occurrence where first == k;
//   their number and the sum of their W per chunk | chunk apply: both exclusive prefixes over chunks, n_cand and S | ORDER
//   scan: candidate r = the chunk's prefix + the rank in the chunk gets cand_slot[r] and cand_P[r] | draw: one workgroup
//   per batch; a thread holds up to 8 slots (ceil(s / 1 024) of them live: the others issue no probe) and searches P for
//   all of them at once (every probe of a step is in flight before one is consumed), then inserts the candidate's index into an LDS table with the slot as value (atomicMin: the
//   first selecting slot), adds 1 to cnt; ranks the first selections that are no frontier node in slot order, leaves n + rank
//   in pos and the slot in sel[rank] | KEEP scan: entries whose source has cnt > 0, per chunk | chunk apply: their prefix,
//   n_edges.
// Pass 2, one scan: the frontier and sel[] give out_nodes, node_count and node_weight; a kept entry lands at edge_off[b] +
//   its chunk's prefix + its rank in the chunk (ballot + popcount: lane order = offset order).  It only reads the
//   workspace, so it may be repeated.
// Five scans of the columns against tg_ns_full's four: a candidate's place in the prefix needs the first occurrences
// counted (FLAG) before it can be named (ORDER), and the kept entries are known only after the draw (KEEP).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, VGPRs / SGPRs): scans 24-52 / 64-91
// (emit the largest), plan 64 / 58, node apply 30 / 56, chunk applies 44-52 / 62-73, clear 16 / 36, draw 55 / 94 with 64 B
// static and up to 144 KiB dynamic LDS; scratch 0 in every kernel.
#include "../../include/tchgeo_ladies.h"
#include "chunk_scan.h"
#include "saint_dedup.h"
#include "tg_scan.h"
#include "tg_device.h"

namespace tg {

constexpr uint64_t LD_MAX_EDGES = (uint64_t)1 << 31;  // m_b below it: k fits the slot's 32-bit `first`, S < 2^63
constexpr int LD_DRAW_THREADS = NSU_THREADS;          // 1 024: the draw's workgroup
constexpr int LD_DRAW_PER = TG_LADIES_MAX_SAMPLES / LD_DRAW_THREADS; // 8 slots a thread
static_assert(LD_DRAW_PER * LD_DRAW_THREADS == TG_LADIES_MAX_SAMPLES, "a thread's slots cover the budget");
// the header's words: {chunks of the batch (0 when refused), accepted, n_cand, S, new nodes}

enum { LD_INSERT = 0, LD_FLAG = 1, LD_ORDER = 2, LD_KEEP = 3, LD_EMIT = 4 };

struct LdArgs {
    const int64_t *ptrs, *indices;
    const uint32_t *ptrs32, *indices32;
    const float *weights;
    int64_t n_major, n_edges_graph;
    const int64_t *nodes, *node_ptr;                   // node_ptr: batch 0 of the launch
    int64_t max_nodes, node_cap, id_bound;
    uint64_t seed, call_id, call_stride;               // call_id: batch 0 of the launch
    uint32_t n_samples;
    int64_t *n_nodes, *n_edges, *n_cand, *total, *chunks; // pass 1
    int32_t *status;
    const int64_t *node_off, *edge_off;                // pass 2
    int64_t *nodes_out, *node_count, *node_weight, *rows, *cols, *edge_index;
    float *edge_weight;
    unsigned char *ws;
    int64_t batch_bytes, first_off, pos_off, cnt_off, w_off, npref_off, epref_off, col0_off, ntile_off, cpref_off, kpref_off,
        wpref_off, ctile_off, ktile_off, wtile_off, cslot_off, cp_off, sel_off;
    int64_t chunk_bound, table_cap, chunk_tiles;
    uint32_t cap_mask, hash_shift, draw_cap, draw_mask, draw_shift;
};

// a batch's part of the workspace
template <typename K> struct LdBatch {
    unsigned long long *hdr, *W, *npref, *epref, *ntile, *wpref, *wtile, *cand_P;
    long long *col0;
    uint32_t *first, *pos, *cnt, *cpref, *kpref, *ctile, *ktile, *cand_slot, *sel;
    K *keys;
    __device__ __forceinline__ LdBatch(const LdArgs &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        hdr = reinterpret_cast<unsigned long long *>(base);
        keys = reinterpret_cast<K *>(base + CS_HEADER);
        first = reinterpret_cast<uint32_t *>(base + a.first_off);              // [table] the first triple of the id
        pos = reinterpret_cast<uint32_t *>(base + a.pos_off);                  // [table] its first position in out_nodes
        cnt = reinterpret_cast<uint32_t *>(base + a.cnt_off);                  // [table] c
        W = reinterpret_cast<unsigned long long *>(base + a.w_off);            // [table]
        npref = reinterpret_cast<unsigned long long *>(base + a.npref_off);    // [max_nodes + 1] chunks before a position
        epref = reinterpret_cast<unsigned long long *>(base + a.epref_off);    // [max_nodes + 1] triples before a position
        col0 = reinterpret_cast<long long *>(base + a.col0_off);               // [max_nodes] the column's first offset
        ntile = reinterpret_cast<unsigned long long *>(base + a.ntile_off);    // [node tiles][2]
        cpref = reinterpret_cast<uint32_t *>(base + a.cpref_off);              // [chunk_bound + 1] candidates of / before a chunk
        kpref = reinterpret_cast<uint32_t *>(base + a.kpref_off);              // [chunk_bound + 1] kept entries of / before a chunk
        wpref = reinterpret_cast<unsigned long long *>(base + a.wpref_off);    // [chunk_bound + 1] W of its candidates
        ctile = reinterpret_cast<uint32_t *>(base + a.ctile_off);              // [chunk tiles] each
        ktile = reinterpret_cast<uint32_t *>(base + a.ktile_off);
        wtile = reinterpret_cast<unsigned long long *>(base + a.wtile_off);
        cand_slot = reinterpret_cast<uint32_t *>(base + a.cslot_off);          // [node_cap] candidate r's table slot
        cand_P = reinterpret_cast<unsigned long long *>(base + a.cp_off);      // [node_cap] and its exclusive prefix
        sel = reinterpret_cast<uint32_t *>(base + a.sel_off);                  // [s] the new nodes' table slots, in order
    }
};

// batch b's frontier: nodes[base .. base + n)
__device__ __forceinline__ int64_t ld_list(const LdArgs &a, int64_t b, int64_t *base) {
    *base = a.node_ptr[b];
    return nsu_clamp(a.node_ptr[b + 1] - *base, a.max_nodes);
}

// q_e and w_e of a weighted entry
__device__ __forceinline__ unsigned long long ld_q_of(float w) {
    const double x = (double)w;
    if (!(x > 0.0)) return 0;
    const double y = x < 1.0 ? x : 1.0;
    return (unsigned long long)(y * y * 4294967296.0); // exact: 48 bits of product, a power of two; <= 2^32
}

template <typename K> __global__ void __launch_bounds__(CS_THREADS) ld_clear_kernel(const LdArgs a) {
    const LdBatch<K> t(a, blockIdx.y);
    const int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    nsu_clear_tile<K, int64_t>(t.keys, t.first, a.table_cap, s0, stride);
    for (int64_t s = s0; s < a.table_cap; s += stride) t.pos[s] = NSU_UNSEEN, t.cnt[s] = 0, t.W[s] = 0;
    for (int64_t s = s0; s < a.chunk_tiles; s += stride) t.ctile[s] = 0, t.ktile[s] = 0, t.wtile[s] = 0;
    if (s0 < 8) t.hdr[s0] = 0;
}

// a tile of positions: the column, its chunks and entries, their exclusive prefixes inside the tile and the tile's sums
template <typename K> __global__ void __launch_bounds__(CS_THREADS) ld_plan_kernel(const LdArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    int64_t base;
    const int64_t n = ld_list(a, b, &base);
    const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const LdBatch<K> t(a, b);
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
template <typename K> __global__ void __launch_bounds__(CS_THREADS) ld_node_apply_kernel(const LdArgs a) {
    __shared__ unsigned long long s_wave[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    int64_t base;
    const int64_t n = ld_list(a, b, &base);
    const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;
    if (tile0 >= n && blockIdx.x != 0) return; // uniform
    const LdBatch<K> t(a, b);
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
        if (a.chunks) a.chunks[b] = (int64_t)n_chunks;
        const unsigned long long distinct = (unsigned long long)n + std::min<unsigned long long>(m, (unsigned long long)a.id_bound);
        if (distinct > (unsigned long long)a.node_cap || n_chunks > (unsigned long long)a.chunk_bound || m >= LD_MAX_EDGES) {
            atomicOr(a.status, 1);
            t.hdr[0] = 0, t.hdr[1] = 0;
            a.n_nodes[b] = 0, a.n_edges[b] = (int64_t)m, a.n_cand[b] = 0, a.total[b] = 0;
        } else {
            t.hdr[0] = n_chunks, t.hdr[1] = 1;
        }
    }
}

// the five scans over the batch's chunks (the file's head comment)
template <typename K, bool I32, int MODE> __global__ void __launch_bounds__(CS_THREADS) ld_scan_kernel(const LdArgs a) {
    const int64_t b = blockIdx.y;
    const LdBatch<K> t(a, b);
    if (t.hdr[1] == 0) return; // refused: uniform
    const unsigned long long n_chunks = t.hdr[0];
    int64_t base;
    const int64_t n = ld_list(a, b, &base);
    if (MODE == LD_INSERT && n_chunks) { // the frontier: pos = position (nobody looks a batch without triples up)
        for (int64_t p = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * CS_THREADS) {
            const int64_t v = a.nodes[base + p];
            if ((uint64_t)v < (uint64_t)a.id_bound) { // any other word equals no source
                const uint32_t s = nsu_insert<K, true>(t.keys, a.cap_mask, a.hash_shift, (K)v);
                atomicMin(&t.pos[s], (uint32_t)p);
            }
        }
    }
    if (MODE == LD_EMIT && (a.nodes_out || a.node_count || a.node_weight)) {
        const int64_t off = a.node_off[b];
        for (int64_t p = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * CS_THREADS) {
            const int64_t v = a.nodes[base + p];
            uint32_t s = NSU_UNSEEN;
            if ((uint64_t)v < (uint64_t)a.id_bound) s = cs_find<false, true>(t.keys, t.first, a.cap_mask, a.hash_shift, (K)v);
            if (a.nodes_out) a.nodes_out[off + p] = v;
            if (a.node_count) a.node_count[off + p] = s != NSU_UNSEEN ? (int64_t)t.cnt[s] : 0;
            if (a.node_weight) a.node_weight[off + p] = s != NSU_UNSEEN ? (int64_t)t.W[s] : 0;
        }
        const int64_t n_new = (int64_t)std::min<unsigned long long>(t.hdr[4], a.n_samples);
        for (int64_t r = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x; r < n_new; r += (int64_t)gridDim.x * CS_THREADS) {
            const uint32_t s = t.sel[r] & a.cap_mask;
            if (a.nodes_out) a.nodes_out[off + n + r] = (int64_t)t.keys[s];
            if (a.node_count) a.node_count[off + n + r] = (int64_t)t.cnt[s];
            if (a.node_weight) a.node_weight[off + n + r] = (int64_t)t.W[s];
        }
    }
    if (n_chunks == 0) return; // uniform
    const unsigned long long S = t.hdr[3];
    if ((MODE == LD_ORDER && t.hdr[2] == 0) || (MODE == LD_EMIT && S == 0)) return; // no candidate / nothing kept: uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = CS_THREADS / 64;
    int unit = CS_UNIT;
    while (unit > 1 && cs_short_fill(n_chunks, unit, gridDim.x, waves)) unit >>= 1;
    const unsigned long long n_units = (n_chunks + unit - 1) / unit;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    const int64_t out0 = MODE == LD_EMIT ? a.edge_off[b] : 0;
    const bool weighted = a.weights != nullptr;
    const double s_d = (double)a.n_samples, S_d = (double)S;
    for (unsigned long long u = (unsigned long long)blockIdx.x * waves + wave; u < n_units; u += (unsigned long long)gridDim.x * waves) {
        const unsigned long long c = u * unit + lane;
        long long my_i = 0, my_e0 = 0, my_k0 = 0;
        int my_len = 0;
        unsigned long long my_q = 0;
        double my_w = 0.0;
        if (lane < unit && c < n_chunks) {
            const int64_t lo = cs_last_le(t.npref, n, c); // npref[0] = 0 <= c < n_chunks = npref[n]; it has chunks
            const long long rel = (long long)(c - t.npref[lo]) * CS_CHUNK;
            const long long k_lo = (long long)t.epref[lo];
            my_i = lo;
            my_e0 = t.col0[lo] + rel;
            my_k0 = k_lo + rel;
            my_len = (int)std::min<long long>(CS_CHUNK, (long long)t.epref[lo + 1] - my_k0);
            const unsigned long long d = t.epref[lo + 1] - t.epref[lo]; // >= 1: the column has chunks; < 2^31
            if (MODE == LD_INSERT) my_q = std::max<unsigned long long>(1, ((unsigned long long)1 << 40) / (d * d));
            if (MODE == LD_EMIT) my_w = 1.0 / (double)d;
        }
        uint32_t unit_cnt = 0;
        unsigned long long unit_w = 0;
        for (int q = 0; q < unit; ++q) {
            const unsigned long long cq = u * unit + q;
            if (cq >= n_chunks) break; // uniform
            const long long i = __shfl(my_i, q), e0 = __shfl(my_e0, q), k0 = __shfl(my_k0, q);
            const int len = __shfl(my_len, q);
            const unsigned long long q_col = MODE == LD_INSERT ? __shfl(my_q, q) : 0;
            const double w_col = MODE == LD_EMIT ? __shfl(my_w, q) : 0.0;
            // the chunk's kept entries as pass 1 counted them: a workspace that is not pass 1's stays in range
            const uint32_t kept0 = MODE == LD_EMIT ? t.kpref[cq] : 0;
            const uint32_t room = MODE == LD_EMIT ? t.kpref[cq + 1] - kept0 : 0;
            const uint32_t cand0 = MODE == LD_ORDER ? t.cpref[cq] : 0;
            unsigned long long run_w = MODE == LD_ORDER ? t.wpref[cq] : 0; // ORDER: P before the step; FLAG: the lane's sum
            uint32_t cnt = 0;
            for (int s = 0; s < len; s += 64) {
                const bool valid = s + lane < len;
                const int64_t e = e0 + s + lane;
                const uint32_t k = (uint32_t)(k0 + s + lane); // < 2^31
                int64_t src = 0;
                if (valid) src = I32 ? (int64_t)a.indices32[e] : a.indices[e];
                if (MODE == LD_INSERT) {
                    if (valid) {
                        const unsigned long long qe = weighted ? ld_q_of(a.weights[e]) : q_col;
                        const uint32_t slot = nsu_insert<K, true>(t.keys, a.cap_mask, a.hash_shift, (K)src);
                        atomicMin(&t.first[slot], k);
                        if (qe) atomicAdd(&t.W[slot], qe);
                    }
                } else if (MODE == LD_FLAG || MODE == LD_ORDER) {
                    uint32_t slot = NSU_UNSEEN;
                    if (valid) slot = cs_find<false, true>(t.keys, t.first, a.cap_mask, a.hash_shift, (K)src);
                    const bool first = slot != NSU_UNSEEN && t.first[slot] == k;
                    const unsigned long long wv = first ? t.W[slot] : 0;
                    const unsigned long long firsts = __ballot(first);
                    if (MODE == LD_FLAG) {
                        run_w += wv;
                    } else {
                        const unsigned long long incl = wave_inclusive_scan(wv);
                        if (first) {
                            const uint32_t r = cand0 + cnt + (uint32_t)__popcll(firsts & below);
                            if ((int64_t)r < a.node_cap) t.cand_slot[r] = slot, t.cand_P[r] = run_w + incl - wv;
                        }
                        run_w += __shfl(incl, 63);
                    }
                    cnt += (uint32_t)__popcll(firsts);
                } else {
                    uint32_t slot = NSU_UNSEEN;
                    if (valid) slot = cs_find<false, true>(t.keys, t.first, a.cap_mask, a.hash_shift, (K)src);
                    const uint32_t c_u = slot != NSU_UNSEEN ? t.cnt[slot] : 0;
                    const bool kept = c_u != 0;
                    const unsigned long long keeps = __ballot(kept);
                    const uint32_t rank = cnt + (uint32_t)__popcll(keeps & below);
                    if (MODE == LD_EMIT && kept && rank < room) {
                        const int64_t o = out0 + kept0 + rank;
                        const double w_e = weighted ? (double)a.weights[e] : w_col;
                        a.rows[o] = (int64_t)t.pos[slot];
                        a.cols[o] = i;
                        a.edge_index[o] = e;
                        a.edge_weight[o] = (float)((((double)c_u * S_d) / (s_d * (double)t.W[slot])) * w_e);
                    }
                    cnt += (uint32_t)__popcll(keeps);
                }
            }
            if (MODE == LD_FLAG) {
                const unsigned long long w_chunk = wave_sum(run_w);
                if (lane == 0) t.cpref[cq] = cnt, t.wpref[cq] = w_chunk;
                unit_cnt += cnt, unit_w += w_chunk;
            }
            if (MODE == LD_KEEP) {
                if (lane == 0) t.kpref[cq] = cnt;
                unit_cnt += cnt;
            }
        }
        if (MODE == LD_FLAG) cs_unit_counted(t.ctile, u, unit, unit_cnt, lane), cs_unit_counted(t.wtile, u, unit, unit_w, lane);
        if (MODE == LD_KEEP) cs_unit_counted(t.ktile, u, unit, unit_cnt, lane);
    }
}

// the exclusive prefixes over a tile of chunks, in place.  KEPT false: candidates and their W, the last tile writes n_cand
// and S; KEPT true: the kept entries, the last tile writes n_edges
template <typename K, bool KEPT> __global__ void __launch_bounds__(CS_THREADS) ld_chunk_apply_kernel(const LdArgs a) {
    __shared__ uint32_t s_wave[CS_THREADS / 64];
    __shared__ unsigned long long s_wave64[CS_THREADS / 64];
    const int64_t b = blockIdx.y;
    const LdBatch<K> t(a, b);
    if (t.hdr[1] == 0) return; // refused: node apply wrote its words
    const unsigned long long n_chunks = t.hdr[0];
    if (cs_tile_idle(n_chunks)) return;
    if (KEPT) {
        const CsTile<uint32_t> r = cs_chunk_apply_tile(t.kpref, t.ktile, n_chunks, s_wave);
        if (r.last && threadIdx.x == 0) {
            t.kpref[n_chunks] = r.base + r.total;
            a.n_edges[b] = (int64_t)(r.base + r.total);
        }
    } else {
        const CsTile<uint32_t> r = cs_chunk_apply_tile(t.cpref, t.ctile, n_chunks, s_wave);
        const CsTile<unsigned long long> w = cs_chunk_apply_tile(t.wpref, t.wtile, n_chunks, s_wave64);
        if (r.last && threadIdx.x == 0) {
            t.cpref[n_chunks] = r.base + r.total, t.wpref[n_chunks] = w.base + w.total;
            t.hdr[2] = r.base + r.total, t.hdr[3] = w.base + w.total;
            a.n_cand[b] = (int64_t)(r.base + r.total), a.total[b] = (int64_t)(w.base + w.total);
        }
    }
}

// the draw of a batch: one workgroup.  LDS: keys[draw_cap] (a candidate's index), vals[draw_cap] (its first selecting
// slot), loc[s] (a slot's place in that table): saint_dedup.h's plan of s positions
template <typename K> __global__ void __launch_bounds__(LD_DRAW_THREADS) ld_draw_kernel(const LdArgs a) {
    extern __shared__ __align__(16) unsigned char ld_lds[];
    __shared__ uint32_t s_wave[LD_DRAW_THREADS / 64];
    const int64_t b = blockIdx.y;
    const LdBatch<K> t(a, b);
    if (t.hdr[1] == 0) return; // refused: uniform
    int64_t base;
    const int64_t n = ld_list(a, b, &base);
    // node_cap: cand_P's length (more candidates only where sources break the contract and lie outside [0, id_bound))
    const unsigned long long n_cand = std::min<unsigned long long>(t.hdr[2], (unsigned long long)a.node_cap), S = t.hdr[3];
    const int tid = threadIdx.x;
    if (n_cand == 0 || S == 0) { // uniform
        if (tid == 0) {
            if (n_cand) atomicOr(a.status, 4);
            t.hdr[4] = 0;
            a.n_nodes[b] = n;
        }
        return;
    }
    nsu_k32 *keys = reinterpret_cast<nsu_k32 *>(ld_lds);
    uint32_t *vals = keys + a.draw_cap;
    uint16_t *loc = reinterpret_cast<uint16_t *>(vals + a.draw_cap);
    for (uint32_t i = tid; i < a.draw_cap; i += LD_DRAW_THREADS) keys[i] = nsu_empty<nsu_k32>(), vals[i] = NSU_UNSEEN;
    const uint32_t s = a.n_samples;
    const CallKey ck = call_key(a.seed, a.call_id + (uint64_t)b * a.call_stride, TG_TAG_LADIES);
    const int live = (int)((s + LD_DRAW_THREADS - 1) / LD_DRAW_THREADS); // slots of a thread that exist at this budget: uniform
    unsigned long long tt[LD_DRAW_PER];
    uint32_t lo[LD_DRAW_PER];
#pragma unroll
    for (int k = 0; k < LD_DRAW_PER; ++k) {
        const uint32_t j = (uint32_t)tid + (uint32_t)k * LD_DRAW_THREADS;
        tt[k] = k < live && j < s ? bounded64(draw(ck, j, 0, 0).a(), S) : 0;
        lo[k] = 0;
    }
    // the last candidate with P <= t (P[0] = 0): one of W = 0 shares its P with its successor and is never the last
    for (uint32_t len = (uint32_t)n_cand; len > 1;) { // len is the same in every slot: a step's probes leave together
        const uint32_t half = len >> 1;
        unsigned long long p[LD_DRAW_PER];
#pragma unroll
        for (int k = 0; k < LD_DRAW_PER; ++k) p[k] = k < live ? t.cand_P[lo[k] + half] : ~0ull; // no probe for a slot past s
#pragma unroll
        for (int k = 0; k < LD_DRAW_PER; ++k)
            if (p[k] <= tt[k]) lo[k] += half;
        len -= half;
    }
    __syncthreads(); // the table is clear
#pragma unroll
    for (int k = 0; k < LD_DRAW_PER; ++k) {
        const uint32_t j = (uint32_t)tid + (uint32_t)k * LD_DRAW_THREADS;
        if (j < s) {
            const uint32_t ls = nsu_insert<nsu_k32, true>(keys, a.draw_mask, a.draw_shift, lo[k]);
            atomicMin(&vals[ls], j);
            loc[j] = (uint16_t)ls;
            atomicAdd(&t.cnt[t.cand_slot[lo[k]]], 1u);
        }
    }
    __syncthreads();
    // first selections that are no frontier node, ranked in slot order: a thread owns a run of slots
    const uint32_t per = (s + LD_DRAW_THREADS - 1) / LD_DRAW_THREADS; // <= 8
    const uint32_t p0 = std::min(s, (uint32_t)tid * per), p1 = std::min(s, p0 + per);
    uint32_t fresh = 0;
    for (uint32_t p = p0; p < p1; ++p)
        if (vals[loc[p]] == p && t.pos[t.cand_slot[keys[loc[p]]]] == NSU_UNSEEN) fresh |= 1u << (p - p0);
    uint32_t n_new;
    uint32_t rank = nsu_scan((uint32_t)__popc(fresh), s_wave, &n_new);
    for (uint32_t f = fresh; f;) {
        const uint32_t p = p0 + __ffs(f) - 1;
        f &= f - 1;
        const uint32_t slot = t.cand_slot[keys[loc[p]]];
        t.pos[slot] = (uint32_t)n + rank;
        t.sel[rank++] = slot;
    }
    if (tid == 0) {
        t.hdr[4] = n_new;
        a.n_nodes[b] = n + (int64_t)n_new;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct LdPlan {
    NsuPlan table;
    SaintPlan draw;
    int64_t chunk_bound, node_tiles, chunk_tiles, batch_bytes;
    int64_t first_off, pos_off, cnt_off, w_off, npref_off, epref_off, col0_off, ntile_off, cpref_off, kpref_off, wpref_off,
        ctile_off, ktile_off, wtile_off, cslot_off, cp_off, sel_off;
};

static int ld_plan(const tg_graph *csc, const tg_ladies_in *in, int64_t id_bound, const char *who, LdPlan &pl) {
    TG_REQUIRE(csc && in, "%s: null argument", who);
    TG_REQUIRE(in->max_nodes >= 0 && in->max_nodes <= TG_LADIES_MAX_NODES, "%s: max_nodes = %lld outside [0, 2^22]", who,
               (long long)in->max_nodes);
    TG_REQUIRE(in->node_cap >= in->max_nodes && in->node_cap <= NSU_MAX_NODES, "%s: node_cap = %lld outside [max_nodes = %lld, 2^30]",
               who, (long long)in->node_cap, (long long)in->max_nodes);
    TG_REQUIRE(in->n_samples >= 1 && in->n_samples <= TG_LADIES_MAX_SAMPLES, "%s: n_samples = %lld outside [1, 8192]", who,
               (long long)in->n_samples);
    if (const int rc = cs_plan_chunks(csc, in->max_nodes, in->chunk_cap, who, pl.chunk_bound, pl.chunk_tiles)) return rc;
    if (const int rc = nsu_plan(in->node_cap, id_bound, who, pl.table)) return rc; // id_bound >= 1, the key width, the table
    TG_REQUIRE(id_bound >= csc->n_major, "%s: id_bound = %lld below n_major = %lld", who, (long long)id_bound,
               (long long)csc->n_major);
    if (const int rc = saint_plan(in->n_samples, who, pl.draw)) return rc;       // the draw's LDS table
    const int64_t pitch = in->max_nodes, T = pl.table.table_cap, C = pl.chunk_bound;
    pl.node_tiles = pitch > 0 ? (pitch + CS_TILE - 1) / CS_TILE : 1;
    pl.first_off = CS_HEADER + nsu_r256(T * pl.table.key_bytes);
    pl.pos_off = pl.first_off + nsu_r256(T * 4);
    pl.cnt_off = pl.pos_off + nsu_r256(T * 4);
    pl.w_off = pl.cnt_off + nsu_r256(T * 4);
    pl.npref_off = pl.w_off + nsu_r256(T * 8);
    pl.epref_off = pl.npref_off + nsu_r256((pitch + 1) * 8);
    pl.col0_off = pl.epref_off + nsu_r256((pitch + 1) * 8);
    pl.ntile_off = pl.col0_off + nsu_r256(pitch * 8);
    pl.cpref_off = pl.ntile_off + nsu_r256(pl.node_tiles * 16);
    pl.kpref_off = pl.cpref_off + nsu_r256((C + 1) * 4);
    pl.wpref_off = pl.kpref_off + nsu_r256((C + 1) * 4);
    pl.ctile_off = pl.wpref_off + nsu_r256((C + 1) * 8);
    pl.ktile_off = pl.ctile_off + nsu_r256(pl.chunk_tiles * 4);
    pl.wtile_off = pl.ktile_off + nsu_r256(pl.chunk_tiles * 4);
    pl.cslot_off = pl.wtile_off + nsu_r256(pl.chunk_tiles * 8);
    pl.cp_off = pl.cslot_off + nsu_r256(in->node_cap * 4);
    pl.sel_off = pl.cp_off + nsu_r256(in->node_cap * 8);
    pl.batch_bytes = pl.sel_off + nsu_r256(in->n_samples * 4);
    return TG_OK;
}

// what both passes check alike, and the kernel arguments of batch 0
static int ld_common(const tg_graph *csc, const tg_ladies_in *in, const tg_rng *rng, int64_t n_batches, int64_t id_bound,
                     void *workspace, int64_t workspace_bytes, const char *who, LdPlan &pl, LdArgs &a) {
    if (const int rc = ld_plan(csc, in, id_bound, who, pl)) return rc;
    TG_REQUIRE(rng, "%s: null rng", who);
    if (n_batches >= 0 && n_batches <= 0x7fffffff)
        if (const int rc = cs_bytes_fit(pl.batch_bytes, n_batches, who)) return rc;
    if (const int rc = cs_check_launch(csc, n_batches, pl.batch_bytes, workspace, workspace_bytes, who)) return rc;
    TG_REQUIRE(in->node_ptr, "%s: null node_ptr", who);
    TG_REQUIRE(in->nodes || in->max_nodes == 0, "%s: null nodes", who);
    a = LdArgs{};
    a.ptrs = csc->ptrs, a.indices = csc->indices, a.ptrs32 = csc->ptrs32, a.indices32 = csc->indices32;
    a.weights = in->weights;
    a.n_major = csc->n_major, a.n_edges_graph = csc->n_edges;
    a.nodes = in->nodes, a.node_ptr = in->node_ptr;
    a.max_nodes = in->max_nodes, a.node_cap = in->node_cap, a.id_bound = id_bound;
    a.seed = rng->seed, a.call_id = rng->call_id, a.n_samples = (uint32_t)in->n_samples;
    a.call_stride = in->call_stride > 0 ? (uint64_t)in->call_stride : 1;
    a.ws = static_cast<unsigned char *>(workspace);
    a.batch_bytes = pl.batch_bytes, a.first_off = pl.first_off, a.pos_off = pl.pos_off, a.cnt_off = pl.cnt_off, a.w_off = pl.w_off;
    a.npref_off = pl.npref_off, a.epref_off = pl.epref_off, a.col0_off = pl.col0_off, a.ntile_off = pl.ntile_off;
    a.cpref_off = pl.cpref_off, a.kpref_off = pl.kpref_off, a.wpref_off = pl.wpref_off;
    a.ctile_off = pl.ctile_off, a.ktile_off = pl.ktile_off, a.wtile_off = pl.wtile_off;
    a.cslot_off = pl.cslot_off, a.cp_off = pl.cp_off, a.sel_off = pl.sel_off;
    a.chunk_bound = pl.chunk_bound, a.table_cap = pl.table.table_cap, a.chunk_tiles = pl.chunk_tiles;
    nsu_mask_shift(pl.table.table_cap, a.cap_mask, a.hash_shift);
    a.draw_cap = (uint32_t)pl.draw.nsu.table_cap;
    nsu_mask_shift(pl.draw.nsu.table_cap, a.draw_mask, a.draw_shift);
    return TG_OK;
}

// the arguments of the round that starts at batch b0
static LdArgs ld_at(const LdArgs &a0, int64_t b0) {
    LdArgs a = a0;
    a.node_ptr += b0, a.ws += b0 * a.batch_bytes, a.call_id += (uint64_t)b0 * a.call_stride;
    if (a.n_nodes) a.n_nodes += b0;
    if (a.n_edges) a.n_edges += b0;
    if (a.n_cand) a.n_cand += b0;
    if (a.total) a.total += b0;
    if (a.chunks) a.chunks += b0;
    if (a.node_off) a.node_off += b0;
    if (a.edge_off) a.edge_off += b0;
    return a;
}

template <typename K, int MODE> static int ld_launch_scan(const LdArgs &a, int64_t nb, hipStream_t stream) {
    const dim3 grid(cs_scan_grid(nb), (unsigned)nb), block(CS_THREADS);
    if (a.indices32)
        hipLaunchKernelGGL((ld_scan_kernel<K, true, MODE>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((ld_scan_kernel<K, false, MODE>), grid, block, 0, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <typename K> static int ld_count(const LdArgs &a0, const LdPlan &pl, int64_t n_batches, hipStream_t stream) {
    const dim3 block(CS_THREADS);
    const int64_t clear_blocks = (std::max(pl.table.table_cap, pl.chunk_tiles) + CS_THREADS - 1) / CS_THREADS;
    const int64_t dyn = pl.draw.nsu.lds_bytes - NSU_STATIC_LDS; // at most 144 KiB, at s = 8 192
    static std::atomic<int64_t> raised[64];
    if (n_batches > 0 && dyn > 64 * 1024) { // above a launch's default limit: it must fit the device's, and is raised to the most
        if (!nsu_fits(pl.draw.nsu, nsu_device_lds_limit()))
            return fail(TG_ERR_UNSUPPORTED, "tg_ladies_count: the draw of n_samples = %u needs %lld bytes of LDS, more than the device has",
                        a0.n_samples, (long long)pl.draw.nsu.lds_bytes);
        if (const int rc = saint_raise_lds(reinterpret_cast<const void *>(&ld_draw_kernel<K>), raised, dyn)) return rc;
    }
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb_) {
        const LdArgs a = ld_at(a0, b0);
        const unsigned nb = (unsigned)nb_;
        hipLaunchKernelGGL(ld_clear_kernel<K>, dim3((unsigned)std::min<int64_t>(clear_blocks, 1024), nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        hipLaunchKernelGGL(ld_plan_kernel<K>, dim3((unsigned)pl.node_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        hipLaunchKernelGGL(ld_node_apply_kernel<K>, dim3((unsigned)pl.node_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        if (const int rc = ld_launch_scan<K, LD_INSERT>(a, nb_, stream)) return rc;
        if (const int rc = ld_launch_scan<K, LD_FLAG>(a, nb_, stream)) return rc;
        hipLaunchKernelGGL((ld_chunk_apply_kernel<K, false>), dim3((unsigned)pl.chunk_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        if (const int rc = ld_launch_scan<K, LD_ORDER>(a, nb_, stream)) return rc;
        hipLaunchKernelGGL(ld_draw_kernel<K>, dim3(1, nb), dim3(LD_DRAW_THREADS), (size_t)dyn, stream, a);
        TG_LAUNCH_CHECK();
        if (const int rc = ld_launch_scan<K, LD_KEEP>(a, nb_, stream)) return rc;
        hipLaunchKernelGGL((ld_chunk_apply_kernel<K, true>), dim3((unsigned)pl.chunk_tiles, nb), block, 0, stream, a);
        TG_LAUNCH_CHECK();
        return (int)TG_OK;
    });
}

template <typename K> static int ld_emit(const LdArgs &a0, int64_t n_batches, hipStream_t stream) {
    return cs_rounds(n_batches, [&](int64_t b0, int64_t nb) { return ld_launch_scan<K, LD_EMIT>(ld_at(a0, b0), nb, stream); });
}

} // namespace tg

extern "C" int tg_ladies_workspace_bytes(const tg_graph *csc, const tg_ladies_in *in, int64_t id_bound, int64_t n_batches,
                                         int64_t *bytes, int64_t *bytes_min) {
    using namespace tg;
    const char *who = "tg_ladies_workspace_bytes";
    LdPlan pl;
    if (const int rc = ld_plan(csc, in, id_bound, who, pl)) return rc;
    return cs_answer_bytes(pl.batch_bytes, n_batches, who, bytes, bytes_min);
}

extern "C" int tg_ladies_count(const tg_graph *csc, const tg_ladies_in *in, const tg_rng *rng, int64_t n_batches,
                               int64_t id_bound, int64_t *n_nodes, int64_t *n_edges, int64_t *n_cand, int64_t *total,
                               int64_t *chunks, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ladies_count";
    LdPlan pl;
    LdArgs a0;
    if (const int rc = ld_common(csc, in, rng, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(n_nodes && n_edges && n_cand && total && status, "%s: null n_nodes / n_edges / n_cand / total / status", who);
    a0.n_nodes = n_nodes, a0.n_edges = n_edges, a0.n_cand = n_cand, a0.total = total, a0.chunks = chunks, a0.status = status;
    hipStream_t stream = (hipStream_t)stream_;
    return pl.table.key_bytes == 4 ? ld_count<nsu_k32>(a0, pl, n_batches, stream) : ld_count<nsu_k64>(a0, pl, n_batches, stream);
}

extern "C" int tg_ladies_emit(const tg_graph *csc, const tg_ladies_in *in, const tg_rng *rng, int64_t n_batches,
                              int64_t id_bound, const int64_t *node_off, const int64_t *edge_off, int64_t *nodes_out,
                              int64_t *node_count, int64_t *node_weight, int64_t *rows, int64_t *cols, int64_t *edge_index,
                              float *edge_weight, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ladies_emit";
    LdPlan pl;
    LdArgs a0;
    if (const int rc = ld_common(csc, in, rng, n_batches, id_bound, workspace, workspace_bytes, who, pl, a0)) return rc;
    TG_REQUIRE(edge_off && rows && cols && edge_index && edge_weight, "%s: null edge_off / rows / cols / edge_index / edge_weight",
               who);
    TG_REQUIRE(node_off || !(nodes_out || node_count || node_weight), "%s: nodes_out / node_count / node_weight given without node_off",
               who);
    a0.node_off = node_off, a0.edge_off = edge_off, a0.nodes_out = nodes_out, a0.node_count = node_count;
    a0.node_weight = node_weight, a0.rows = rows, a0.cols = cols, a0.edge_index = edge_index, a0.edge_weight = edge_weight;
    hipStream_t stream = (hipStream_t)stream_;
    return pl.table.key_bytes == 4 ? ld_emit<nsu_k32>(a0, n_batches, stream) : ld_emit<nsu_k64>(a0, n_batches, stream);
}
