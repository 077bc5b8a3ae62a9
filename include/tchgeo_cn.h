/* Common neighbours per candidate link (the classical link heuristics -- common neighbours, Jaccard, Adamic-Adar, resource
 * allocation -- and the per-link lists that Neural Common Neighbor, Neo-GNN and BUDDY take as mini-batch input) behind
 * libtchgeo_hip.so: tg_cn_links (csrc/cn.hip).  Plain C99; an additive part of the C ABI of tchgeo.h, kept in a header of its
 * own.
 *
 * THE RULE.  Slot i holds the link (u, v) = (src[i], dst[i]) on the view g.
 *   A(x) = the set of DISTINCT entries of x's row of g's major: a CSC view gives in-neighbours; callers who want the undirected
 *     notion pass a symmetric graph.  Parallel entries count once.  Rows ascend (tg_graph's contract; tg_coo_to_csx makes them
 *     so) and their entries are below 2^32, the id width of the library's u32 shadows.
 *   exclude_ends = 1: entries equal to u or to v are no members (this removes the target link and self loops);
 *   exclude_ends = 0: they are (the bipartite use, where the two id spaces differ).
 *   C = A(u) n A(v).  u == v is allowed: C = A(u).
 *
 * OUTPUT per slot:
 *   count[i]     = |C|, always exact.
 *   cn[i][.]       a row of pitch cn_cap: the min(|C|, cn_cap) smallest members of C by id ascending; nothing behind them is
 *                  written.  |C| > cn_cap raises status bit 0 (value 1); that is no refusal: count, score and adjacent stay
 *                  exact.
 *   adjacent[i]    (optional) bit 0 = v occurs in u's row, bit 1 = u occurs in v's row, both taken before any exclusion.  With
 *                  tables every entry is below id_bound, so a bit is 0 where the id looked for is >= id_bound.
 *   score[i][k]    (with n_tables > 0) for k < n_tables <= TG_CN_MAX_TABLES: the uint64 sum over ALL w in C, not only the
 *                  listed part, of tables[k][w].  `tables` is a device uint32 array [n_tables, id_bound] of fixed-point
 *                  per-vertex weights in units of 2^-32, clamped to 2^32 - 1.  The sum is an integer, so it depends on
 *                  neither order nor form.  An entry >= id_bound in a row is then a contract violation like any id out of
 *                  range; without tables id_bound is unused.
 *   An endpoint outside [0, g->n_major) raises status bit 1 (value 2): the slot gets count 0, adjacent 0 and scores 0, its cn
 *   row is not written and the other slots are unaffected.
 *   Rows that do not ascend break tg_graph's contract: the words are then unspecified, but every search is bounded by the row
 *   ends, so nothing outside the two rows is read and nothing outside cn_cap is written.
 *
 * FORMS (equal words):
 *   TG_CN_FORM_WAVE   one wavefront owns a link: tiles of 64 entries of the shorter row, the matching span of the longer row
 *                     bracketed by a 64-ary search, spans up to TG_CN_WINDOW entries searched in LDS.  No workspace.
 *   TG_CN_FORM_GROUP  one workgroup owns a link, in rounds of TG_CN_GROUP_TILES tiles.
 *   TG_CN_FORM_AUTO   the wave kernel takes the links whose shorter row has at most wave_max entries (0 = TG_CN_WAVE_MAX) and
 *                     lists the others for the group kernel, which follows on the same stream.
 *   Workspace: 0 bytes for _WAVE (it may be NULL), else 256 + 4 * m rounded up to 256: a counter, then the list.  4-byte
 *   aligned.  The call clears the counter itself.
 *
 * LIMITS: cn_cap in [1, 2^20], n_tables in [0, TG_CN_MAX_TABLES], tables need id_bound >= 1 and score, wave_max >= 0, m in
 *   [0, 2^31); g->n_major above 2^31 is TG_ERR_UNSUPPORTED.  Null required buffers (src, dst, count, cn, status, the graph's
 *   arrays), sizes outside the limits, an unknown form and a short or misaligned workspace are refused with TG_ERR_INVALID
 *   before anything is launched; m = 0 launches nothing.  The call is stream-ordered, allocates nothing, does not synchronise
 *   and reads nothing back.  `status`: one device int32, zeroed by the caller, OR-ed into.  indices32 / ptrs32 are used when
 *   given, with equal words. */
#ifndef TCHGEO_CN_H
#define TCHGEO_CN_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_CN_MAX_CAP 1048576  /* 2^20 */
#define TG_CN_MAX_TABLES 4
#define TG_CN_WINDOW 512       /* words of LDS per wavefront: the longest span of the longer row searched there */
#define TG_CN_WAVE_MAX 4096    /* AUTO: the longest shorter row that stays with the wave kernel */
#define TG_CN_GROUP_TILES 256  /* tiles of 64 entries per round of the group kernel */
#define TG_CN_WAVE_GROUPS 2048 /* workgroups (of four wavefronts) of the wave kernel's grid at most */
#define TG_CN_GROUP_GROUPS 1024 /* workgroups of the group kernel's grid at most */
#define TG_CN_FORM_AUTO 0
#define TG_CN_FORM_WAVE 1
#define TG_CN_FORM_GROUP 2
#define TG_CN_STATUS_CAP 1
#define TG_CN_STATUS_RANGE 2

typedef struct {
    const int64_t *src;     /* device [m]: u */
    const int64_t *dst;     /* device [m]: v */
    const uint32_t *tables; /* device [n_tables, id_bound] or NULL */
    int64_t id_bound;       /* the tables' pitch; unused without tables */
    int32_t cn_cap;         /* listed members per slot at most; the pitch of cn */
    int32_t n_tables;
    int32_t exclude_ends;   /* 0 or 1 */
    int32_t wave_max;       /* AUTO's threshold; 0 = TG_CN_WAVE_MAX */
} tg_cn_in;

typedef struct {
    int64_t *count;    /* device [m] */
    int64_t *cn;       /* device [m, cn_cap] */
    int64_t *adjacent; /* device [m] or NULL */
    uint64_t *score;   /* device [m, n_tables]; NULL only with n_tables = 0 */
} tg_cn_out;

/* *form_taken (may be NULL): the form a call runs.  Touches no device. */
TG_API int tg_cn_workspace_bytes(int64_t m, int32_t form, int64_t *bytes, int32_t *form_taken);
TG_API int tg_cn_links(const tg_graph *g, const tg_cn_in *in, const tg_cn_out *out, int64_t m, int32_t form, int32_t *status,
                       void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
