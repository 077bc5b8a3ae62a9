/* A balanced label-propagation partitioner (Raghavan et al. 2007; Ugander and Backstrom 2013; PuLP; Spinner) behind
 * libtchgeo_hip.so: tg_lp_sizes, tg_lp_propose, tg_lp_commit (csrc/lp.hip).  It makes the node partition ClusterData takes.
 * Plain C99; an additive part of the C ABI of tchgeo.h, kept in a header of its own.
 *
 * THE RULE.  View g (CSR or CSC, rows ascending or not: the rule is order-free), n = g->n_major.  Parts P in [1, 2^20].
 *   `label` is a device int32 [n] with values in [0, P), `size` a device int64 [P], cap >= 1, `seed` a uint64 and `round` a
 *   uint64 that acts as the call id.  One round is a propose and a commit: synchronous, integers only, a pure function of
 *   (graph, labels, parameters, seed, round).
 *
 * PROPOSE.  For vertex v with l0 = label[v]:
 *   cnt[l]  = the number of entries w of v's row with 0 <= w < n, w != v and label[w] = l.  Parallel entries count with their
 *             multiplicity; self loops and entries outside [0, n) count nowhere.
 *   best    = the label l != l0 with the largest cnt[l] > 0; ties go to the smaller l.
 *   gain    = cnt[best] - cnt[l0].  v is a MOVER iff best exists and gain > 0.
 *   skey[v] = (best << 44) | ((4095 - min(gain, 4095)) << 32) | h(v) for a mover, all ones otherwise (a uint64), where
 *             h(v) = word 0 of the draw (call key of (seed, round, TG_TAG_LP), id = v, d0 = 0, d1 = 0): the call key is
 *             Philox4x32-10(key = seed, counter = (round, TG_TAG_LP, "tchg")) words 0 and 1, the draw Philox4x32-10(key = call
 *             key, counter = (0, 0, v low, v high)).
 *   cut_entries (a device uint64, ADDED to): over all v, the number of counted entries whose label differs from l0.  The sum
 *             is an integer, so it depends on neither order nor form.
 *   A label outside [0, P) breaks the contract (tg_lp_sizes finds one): an entry that carries it counts nowhere, a vertex that
 *   carries it is no mover and adds nothing; nothing out of bounds is touched.
 *
 * COMMIT.
 *   free[l] = max(0, cap - size[l]), all P values taken before anything changes.
 *   The movers are ordered ascending by (skey, v): by target, then the larger gain, then h, then v.  Within the movers of one
 *   target l the first free[l] are admitted; the others stay where they are.  For an admitted v: size[label[v]] -= 1,
 *   size[l] += 1, label[v] = l.  `moved` (a device int64, ADDED to) += the number admitted.
 *   A leaver's place is NOT credited to free within the round: that keeps every size <= cap under synchronous moves.  If
 *   every size starts <= cap it stays so; a part above cap has free = 0 and only shrinks.
 *   An skey whose target field is >= P and that is not all ones raises status bit 1 (value 2); that vertex does not move and
 *   takes no one's place.
 *
 * FORMS of propose (equal words):
 *   TG_LP_FORM_WAVE   one wavefront owns a row: tiles of 64 entries, the labels sorted in registers, runs folded into a table
 *                     in LDS from the second tile on.  Rows of any length (a long row with many labels takes several passes).
 *   TG_LP_FORM_GROUP  one workgroup owns a row; its table lives in LDS while min(row length, P) <= TG_LP_LDS_LABELS and is a
 *                     dense counter array in the workspace otherwise.
 *   TG_LP_FORM_AUTO   the wave kernel takes the rows of at most wave_max entries (0 = TG_LP_WAVE_MAX, the largest allowed) and
 *                     lists the others for the group kernel, which follows on the same stream.
 *
 * WORKSPACE.  tg_lp_workspace_bytes gives one size that serves propose and commit alike (they never overlap in time on a
 *   stream): the larger of
 *     propose  256 (a counter) + [AUTO] r256(4 n) (the list) + [not WAVE and P > TG_LP_LDS_LABELS] TG_LP_DENSE_GROUPS *
 *              r256(8 P) (counters and touched labels of the resident workgroups); the call clears what it reads;
 *     commit   r256(8 P) (free) + r256(4 P) (a target's first place) + 2 r256(4 n) (vertices in and out) + r256(8 n) (sorted
 *              keys) + the temporary storage of the radix sort for n pairs.
 *   with r256 rounding up to 256.  16-byte aligned.
 *
 * LIMITS: P in [1, TG_LP_MAX_PARTS], cap >= 1, wave_max in [0, TG_LP_WAVE_MAX], n in [0, 2^31) and fewer than 2^32 entries
 *   (more is TG_ERR_UNSUPPORTED).  Null required buffers, sizes outside the limits, an unknown form and a short or misaligned
 *   workspace are refused with TG_ERR_INVALID before anything is launched; n = 0 launches nothing.  Every call is
 *   stream-ordered, allocates nothing, does not synchronise and reads nothing back.  `status`: one device int32, zeroed by the
 *   caller, OR-ed into.  indices32 / ptrs32 are used when given, with equal words. */
#ifndef TCHGEO_LP_H
#define TCHGEO_LP_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_TAG_LP 20u             /* DESIGN.md "Randomness": the next free tag */
#define TG_LP_MAX_PARTS 1048576   /* 2^20 */
#define TG_LP_WAVE_MAX 512        /* AUTO: the longest row that stays with the wave kernel; eight tiles, all gathered ahead */
#define TG_LP_LDS_LABELS 2048     /* the most distinct labels the group kernel's LDS table holds (at load 1/2) */
#define TG_LP_WAVE_GROUPS 2048    /* workgroups (of four wavefronts) of the wave kernel's grid at most */
#define TG_LP_GROUP_GROUPS 1024   /* workgroups of the group kernel's grid at most while every table is in LDS */
#define TG_LP_DENSE_GROUPS 32     /* and while P > TG_LP_LDS_LABELS: each owns 8 P bytes of the workspace */
#define TG_LP_FORM_AUTO 0
#define TG_LP_FORM_WAVE 1
#define TG_LP_FORM_GROUP 2
#define TG_LP_STATUS_LABEL 1      /* tg_lp_sizes: a label outside [0, P) */
#define TG_LP_STATUS_TARGET 2     /* tg_lp_commit: an skey with a target >= P that is not all ones */

/* *form_taken (may be NULL): the form a propose runs.  Touches no device. */
TG_API int tg_lp_workspace_bytes(int64_t n, int32_t n_parts, int32_t form, int32_t wave_max, int64_t *bytes,
                                 int32_t *form_taken);
/* size[l] = the number of v with label[v] = l; clears `size` itself.  A label outside [0, P) raises status bit 0 and is not
 * counted. */
TG_API int tg_lp_sizes(const int32_t *label, int64_t n, int32_t n_parts, int64_t *size, int32_t *status, void *stream);
TG_API int tg_lp_propose(const tg_graph *g, const int32_t *label, int32_t n_parts, uint64_t seed, uint64_t round, int32_t form,
                         int32_t wave_max, uint64_t *skey, uint64_t *cut_entries, int32_t *status, void *workspace,
                         int64_t workspace_bytes, void *stream);
TG_API int tg_lp_commit(int32_t *label, int64_t *size, int64_t n, int32_t n_parts, int64_t cap, const uint64_t *skey,
                        int64_t *moved, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
