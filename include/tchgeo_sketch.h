/* Subgraph sketches for link prediction (Chamberlain et al., Graph Neural Networks for Link Prediction with Subgraph
 * Sketching, ICLR 2023: ELPH and BUDDY) behind libtchgeo_hip.so: tg_sketch_init, tg_sketch_propagate, tg_sketch_links
 * (csrc/sketch.hip).  Plain C99; an additive part of the C ABI of tchgeo.h, kept in a header of its own.
 *
 * THE RULE.
 * Parameters.
 *   - n_perm is a multiple of 64 in [64, 256].
 *   - hll_p is in [8, 10], and m_reg = 2^hll_p.
 *   - hops = h is in [1, 3].
 *   - seed is a uint64.
 * Row layout.  A sketch row is W = n_perm + m_reg / 4 uint32 words: the n_perm MinHash words, then the m_reg registers, one
 *   byte each.  Register j sits in word n_perm + j / 4 at bits 8 (j mod 4) and up.  A sketch is a device array [h + 1, n, W],
 *   hop-major, owned by the caller.  tg_sketch_bytes gives its size.
 * Hop 0, tg_sketch_init.  For a vertex x in [0, n):
 *   - D(x, j, t) = philox4x32_10(c0 = lo32(x), c1 = hi32(x), c2 = j, c3 = t, k0 = lo32(seed), k1 = hi32(seed)).
 *   - M_0(x)[4j + i] = word i of D(x, j, 0x736B6D68).
 *   - Let (w0, w1, ., .) = D(x, 0, 0x736B686C).  Then R_0(x) is all zero, except for register w0 & (m_reg - 1), which holds
 *     1 + clz32(w1).  clz32(0) = 32, so ranks lie in [1, 33].
 * A hop, tg_sketch_propagate(g, prev, next).
 *   - M_l(x)[k] = min of M_{l-1}(x)[k] and M_{l-1}(y)[k] over every entry y of x's row of g's major.
 *   - R_l is the same with max, per register.
 *   - The vertex itself always takes part, so the sketches describe closed balls: N_l(x) is every vertex within l hops, with
 *     N_0(x) = {x}.
 *   - Parallel entries and self loops change nothing, because min and max are idempotent.
 *   - An entry outside [0, n) is skipped and raises status bit 1.  Nothing outside the arrays is read.
 *   - g->n_major is n.  Callers who want the undirected notion pass a symmetric graph.
 *   - prev == next, or ranges that overlap, are refused.
 * A link, tg_sketch_links.  Slot i is (u, v) = (src[i], dst[i]).  For a, b in 1..h the outputs are:
 *   match[i][a-1][b-1]  int32   the number of k < n_perm with M_a(u)[k] == M_b(v)[k]
 *   usum[i][a-1][b-1]   uint64  sum over the registers j of 2^(33 - max(R_a(u)[j], R_b(v)[j])).  It is at most 2^43, an
 *                               exact integer
 *   uzero[i][a-1][b-1]  int32   the number of registers where that max is 0
 *   nsum[i][s][a-1], nzero[i][s][a-1]  same types: the same two words for the single sketch of end s (0 = u, 1 = v) at hop a
 *   - An end outside [0, n) raises status bit 1.  The slot's words are all 0 and the other slots are unaffected.
 *   - u == v is allowed.
 *   - Every output is an integer function of (sketch, link).  It depends on neither order nor form.
 * Refusals.  These are refused with TG_ERR_INVALID before any launch, and tg_last_error names the cause:
 *   - null required buffers;
 *   - parameters outside the ranges above;
 *   - n outside [1, 2^31];
 *   - m outside [0, 2^31);
 *   - an unknown form;
 *   - a short or misaligned workspace.
 *   m = 0 launches nothing.
 * Every call is stream-ordered.  It allocates nothing, does not synchronise and reads nothing back.  `status` is one device
 * int32, zeroed by the caller and OR-ed into.
 *
 * BESIDE THE RULE.  Status bit 1 has the value TG_SKETCH_STATUS_RANGE = 2, as in tchgeo_cn.h.  A register that holds more than
 * 33 (no sketch of this library does) counts as 2^0 in usum / nsum.  Sketch arrays are 16-byte aligned (a row is a multiple
 * of 256 bytes); all five outputs of tg_sketch_links are required.  Row pointers that contradict g->n_edges are clamped into
 * [0, n_edges]; lists that then outgrow the workspace raise TG_SKETCH_STATUS_GRAPH and the rows concerned are not written.
 *
 * FORMS of tg_sketch_propagate (equal words: min and max have no order):
 *   TG_SKETCH_FORM_WAVE   one wavefront owns a destination row.  No workspace (it may be NULL).
 *   TG_SKETCH_FORM_GROUP  one workgroup owns a row; its four wavefronts combine their partial rows through LDS.  No workspace.
 *   TG_SKETCH_FORM_SPLIT  every row with an entry is cut into segments of at most split_seg entries, a workgroup each; the
 *                         partial rows go to the workspace and a combine pass folds them with the vertex's own row.
 *   TG_SKETCH_FORM_AUTO   the wave kernel takes rows up to wave_max entries, lists longer rows up to group_max for the group
 *                         kernel and the rest, with their segments, for the split kernels, which follow on the same stream.
 *   Tuning (NULL or a zero field = the TG_SKETCH_* default): wave_max in [0, 2^30], group_max in [0, 2^30] (AUTO takes
 *   max(group_max, wave_max)), split_seg in [TG_SKETCH_SPLIT_SEG_MIN, TG_SKETCH_SPLIT_SEG].
 *   Workspace, 16-byte aligned, with r256(x) = x rounded up to a multiple of 256, E = g->n_edges, and for a threshold t
 *   over(t) = min(n, E / (t + 1)), the most rows that can be longer than t:
 *     _WAVE, _GROUP: 0 bytes.
 *     G = over(wave_max) under AUTO, 0 under _SPLIT: the group list.
 *     S = over(max(group_max, wave_max)) under AUTO, over(0) under _SPLIT: the split rows.
 *     Q = S + E / split_seg: the segments.
 *     bytes = 256 + r256(4 G) + r256(8 S) + r256(8 Q) + Q * W * 4: three counters, the lists, the partial rows.
 *   The call clears the counters itself, with a kernel. */
#ifndef TCHGEO_SKETCH_H
#define TCHGEO_SKETCH_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_SKETCH_TAG_MINHASH 0x736B6D68 /* "skmh" */
#define TG_SKETCH_TAG_HLL 0x736B686C     /* "skhl" */
#define TG_SKETCH_MAX_HOPS 3
#define TG_SKETCH_WAVE_MAX 64        /* AUTO: the longest row that stays with the wave kernel */
#define TG_SKETCH_GROUP_MAX 4096     /* AUTO: the longest row that stays with the group kernel */
#define TG_SKETCH_SPLIT_SEG 2048     /* entries per segment of the split kernel at most, and the default */
#define TG_SKETCH_SPLIT_SEG_MIN 64
#define TG_SKETCH_WAVE_GROUPS 2048   /* workgroups (of four wavefronts) of a wave-per-item grid at most */
#define TG_SKETCH_GROUP_GROUPS 2048  /* workgroups of a workgroup-per-item grid at most */
#define TG_SKETCH_FORM_AUTO 0
#define TG_SKETCH_FORM_WAVE 1
#define TG_SKETCH_FORM_GROUP 2
#define TG_SKETCH_FORM_SPLIT 3
#define TG_SKETCH_STATUS_RANGE 2
#define TG_SKETCH_STATUS_GRAPH 4

typedef struct {
    int32_t n_perm;
    int32_t hll_p;
    int32_t hops;
    int32_t reserved; /* 0 */
    uint64_t seed;
} tg_sketch_params;

typedef struct {
    int32_t wave_max;
    int32_t group_max;
    int32_t split_seg;
} tg_sketch_tuning;

typedef struct {
    int32_t *match;  /* device [m, h, h] */
    uint64_t *usum;  /* device [m, h, h] */
    int32_t *uzero;  /* device [m, h, h] */
    uint64_t *nsum;  /* device [m, 2, h] */
    int32_t *nzero;  /* device [m, 2, h] */
} tg_sketch_link_out;

/* *bytes = (hops + 1) * n * W * 4, *row_words (may be NULL) = W.  Touches no device. */
TG_API int tg_sketch_bytes(const tg_sketch_params *p, int64_t n, int64_t *bytes, int64_t *row_words);
/* hop 0 into sketch[0 .. n * W) */
TG_API int tg_sketch_init(const tg_sketch_params *p, int64_t n, uint32_t *sketch, void *stream);
/* *form_taken (may be NULL): the form a call runs.  Touches no device. */
TG_API int tg_sketch_propagate_workspace_bytes(const tg_sketch_params *p, int64_t n, int64_t n_edges, int32_t form,
                                               const tg_sketch_tuning *tuning, int64_t *bytes, int32_t *form_taken);
/* prev, next: [n, W] each, n = g->n_major */
TG_API int tg_sketch_propagate(const tg_graph *g, const tg_sketch_params *p, const uint32_t *prev, uint32_t *next, int32_t form,
                               const tg_sketch_tuning *tuning, int32_t *status, void *workspace, int64_t workspace_bytes,
                               void *stream);
/* sketch: the whole [h + 1, n, W] array */
TG_API int tg_sketch_links(const tg_sketch_params *p, int64_t n, const uint32_t *sketch, const int64_t *src, const int64_t *dst,
                           const tg_sketch_link_out *out, int64_t m, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
