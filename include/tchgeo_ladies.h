/* Layer-wise importance sampling (FastGCN's estimator with LADIES' layer-dependent law, Zou et al., NeurIPS 2019) behind
 * libtchgeo_hip.so: tg_ladies_count / tg_ladies_emit (csrc/ladies.hip).  Plain C99; an additive part of the C ABI of
 * tchgeo.h, kept in a header of its own.
 *
 * A layer draws ONE budget of s = n_samples nodes for a whole mini-batch: a node's probability is proportional to the
 * squared norm of its column in the frontier's rows of the normalised adjacency, and the kept edges are rescaled so that
 * the layer's aggregation stays an unbiased estimate.  Everything is integer until the last step, so the operator is a
 * function of (graph, frontiers, seed, call id).  Sampling is WITH replacement: LADIES' own code samples without
 * replacement and then rescales by 1/p, which is biased; the with-replacement form is unbiased and needs no floating-point
 * keys.
 *
 * The rule, for every batch b independently, with its frontier v_0 .. v_{n-1} = nodes[node_ptr[b] .. node_ptr[b+1]) (n
 * clamped to [0, max_nodes]; the nodes are expected distinct).  Columns, triple order and out-of-range ids are exactly
 * tg_ns_full_*'s:
 *   col(i) = the CSC column [ptrs[v_i], ptrs[v_i+1]) of length d_i; an id outside [0, csc->n_major) is a column of length 0
 *            and raises status bit 1 (value 2)
 *   triple k = (src_k = indices[e], col = i, edge_index = e), for i ascending and e ascending; m_b = their number
 * Entry weights:
 *   weights == NULL   the row-normalised adjacency (what LADIES' code uses):
 *                     q_e = max(1, 2^40 / (d_i * d_i)) in unsigned 64-bit integer division, w_e = 1.0 / (double)d_i
 *   weights given     (float32 per CSC entry, the caller's Laplacian entries): x = (double)weights[e];
 *                     q_e = 0 unless x > 0 (a NaN is not), else q_e = (uint64)floor(min(x, 1.0)^2 * 2^32), every step exact
 *                     in double; w_e = x
 * Candidates = the distinct src_k in order of first occurrence in triple order (the frontier is NOT pre-inserted).
 *   W_u = the sum of q_e over the entries with src = u (64-bit integer adds: the order does not matter; parallel entries
 *   count separately); P = the exclusive prefix of W in candidate order; S_b = the total.  max_nodes <= 2^22 gives
 *   S <= 2^62 without weights, m_b < 2^31 gives S < 2^63 with them.
 * Draws: slot j in 0 .. s-1 takes ONE Philox block, w = draw(call key of (rng->seed, rng->call_id + b, TG_TAG_LADIES),
 *   id = j, d0 = 0, d1 = 0) (call_stride > 1: rng->call_id + b * call_stride, for a loader that numbers the layers of
 *   a mini-batch consecutively), lo = w0 | w1 << 32, t = floor(lo * S_b / 2^64) by a 128-bit product; the slot selects the one
 *   candidate u with P_u <= t < P_u + W_u (one with W_u = 0 is never selected); c_u = the number of slots that selected u.
 *   1 <= s <= 8192.  S_b = 0 selects nothing; with candidates present it raises status bit 2 (value 4).
 * Outputs:
 *   out_nodes = v_0 .. v_{n-1}, followed by every selected candidate that is no frontier node, ordered by its first
 *               selecting slot; n_out_b = len(out_nodes)
 *   node_count / node_weight per position of out_nodes: c and W of the node there (0 where a frontier node was not drawn /
 *               is no candidate; a frontier id outside [0, id_bound) has 0 and 0)
 *   total[b] = S_b, n_cand[b] = the number of candidates
 *   kept triples = those with c_src > 0, in triple order: row = the FIRST position of src in out_nodes, col = i,
 *               edge_index = e, edge_weight (float32) =
 *               (float)(((double)c_u * (double)S_b) / ((double)s * (double)W_u) * w_e): five single IEEE operations in that
 *               order (the library is built with -ffp-contract=off).  E[c_u] = s * W_u / S_b, so the kept edges of column i
 *               sum to an unbiased estimate of the full row.
 * Two exact passes with tg_ns_full_*'s division of work (chunks of 512 CSC offsets spread over the device: a hub column is
 * many chunks) and capacity rule.  tg_ladies_count scans, accumulates, draws and counts: n_nodes[b] = n_out_b, n_edges[b] =
 * the kept triples, n_cand[b], total[b], chunks[b] (may be NULL) = the sum over positions of ceil(d_i / 512).  The caller
 * forms the exclusive prefixes node_off / edge_off; tg_ladies_emit, with the same arguments and the SAME untouched
 * workspace, writes out_nodes / node_count / node_weight at node_off[b] (each may be NULL: nothing is written for it) and
 * the kept triples to rows / cols / edge_index / edge_weight[edge_off[b] ..).  Nothing outside those ranges is written.
 * Emit leaves the workspace as it found it.  Neither call allocates, synchronises or reads back.
 * Capacity, decided per batch before any table work: the table holds the frontier and the candidates, so a batch with
 * n + min(m_b, id_bound) > node_cap, with chunks[b] > the chunk bound (chunk_cap; <= 0: max_nodes + ceil(csc->n_edges /
 * 512)) or with m_b >= 2^31 is refused: status bit 0 (value 1), n_nodes[b] = n_cand[b] = total[b] = 0, n_edges[b] = m_b (ALL
 * its triples, the figure the need is made of) and chunks[b] exact, so the caller can repeat with a workspace of that size;
 * pass 2 writes nothing for it; other batches are unaffected.
 * Hash keys are 32-bit while id_bound (>= csc->n_major) <= 2^31, else 64-bit; indices32 / ptrs32 are used when given, with
 * equal results.  Limits: max_nodes in [0, 2^22], node_cap in [max_nodes, 2^30], n_samples in [1, 8192], the chunk bound <=
 * 2^31.  Null buffers, sizes outside those limits, id_bound < csc->n_major and a short or misaligned (8 bytes) workspace
 * are refused with TG_ERR_INVALID before anything is launched; n_batches = 0 launches nothing; more batches than one grid's
 * y extent run in rounds.
 * The workspace holds all n_batches at once, bytes = n_batches * bytes_min, and with r(x) = x rounded up to 256, T = the
 * least power of two >= max(64, (4 * node_cap + 2) / 3), k = the key's bytes, C = the chunk bound, t = C / 1024 + 1 and
 * p = max_nodes:
 *   bytes_min = 256 + r(T k) + 3 r(4 T) + r(8 T) + 2 r(8 (p + 1)) + r(8 p) + r(16 max(1, ceil(p / 1024)))
 *             + 2 r(4 (C + 1)) + r(8 (C + 1)) + 2 r(4 t) + r(8 t) + r(4 node_cap) + r(8 node_cap) + r(4 s) */
#ifndef TCHGEO_LADIES_H
#define TCHGEO_LADIES_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_TAG_LADIES 18u
#define TG_LADIES_MAX_SAMPLES 8192
#define TG_LADIES_MAX_NODES 4194304 /* 2^22 */

typedef struct {
    const int64_t *nodes;     /* device, flat: batch b's frontier is nodes[node_ptr[b] .. node_ptr[b+1]) */
    const int64_t *node_ptr;  /* device [n_batches + 1], ascending from any base */
    int64_t max_nodes;        /* the caller's bound on node_ptr[b+1]-node_ptr[b]; a longer list is clamped to it */
    int64_t node_cap;         /* distinct nodes (frontier + candidates) per batch the workspace's table holds */
    int64_t chunk_cap;        /* chunks per batch the workspace holds; <= 0: max_nodes + ceil(n_edges / 512) */
    int64_t n_samples;        /* s: the layer's budget of draws, 1 .. 8192 */
    const float *weights;     /* device, per CSC entry; NULL: the row-normalised adjacency */
    int64_t call_stride;      /* batch b draws under rng->call_id + b * call_stride; <= 0: 1 */
} tg_ladies_in;

/* only the sizes of `in` (max_nodes, node_cap, chunk_cap, n_samples) are read */
TG_API int tg_ladies_workspace_bytes(const tg_graph *csc, const tg_ladies_in *in, int64_t id_bound, int64_t n_batches,
                                     int64_t *bytes, int64_t *bytes_min /* one batch */);
/* pass 1: n_nodes, n_edges, n_cand, total, chunks: device int64 [n_batches] (chunks may be NULL); status: device int32,
 * zeroed by the caller */
TG_API int tg_ladies_count(const tg_graph *csc, const tg_ladies_in *in, const tg_rng *rng, int64_t n_batches,
                           int64_t id_bound, int64_t *n_nodes, int64_t *n_edges, int64_t *n_cand, int64_t *total,
                           int64_t *chunks, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);
/* pass 2: node_off, edge_off: device [n_batches], the caller's exclusive prefixes of n_nodes and n_edges */
TG_API int tg_ladies_emit(const tg_graph *csc, const tg_ladies_in *in, const tg_rng *rng, int64_t n_batches,
                          int64_t id_bound, const int64_t *node_off, const int64_t *edge_off, int64_t *nodes_out,
                          int64_t *node_count, int64_t *node_weight, int64_t *rows, int64_t *cols, int64_t *edge_index,
                          float *edge_weight, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
