/* SEAL enclosing subgraphs with a cap on the new vertices of every hop (SEAL-OGB's max_nodes_per_hop: Zhang et al., NeurIPS
 * 2021, "Labeling Trick"; github.com/facebookresearch/SEAL_OGB's k_hop_subgraph) behind libtchgeo_hip.so:
 * tg_seal_nodes_capped (csrc/seal_capped.hip).  Plain C99; an additive part of the C ABI, in a header of its own.  tg_seal_in,
 * tg_seal_out, the forms, the status bits and every limit are tchgeo_seal.h's.
 *
 * THE RULE.  Slot i is a link (u, v) on the view g with call id c_i: c_i = call_ids[i] where the array is given, else
 *   call_id0 + i.  max_per_hop[t - 1] = k_t is a host array of num_hops int32 words.
 *   S_0 = N_0 = {u, v}.
 *   For t = 1..h, the fringe F_t is every vertex y not in N_{t-1} that is an entry of the row of some x in S_{t-1}.  It is a
 *     set: parallel entries, self loops and several parents count once.  Hop t expands S_{t-1}, not N_{t-1}.
 *   If k_t = 0 (uncapped) or |F_t| <= k_t, then S_t = F_t.
 *   Otherwise S_t is the k_t members of F_t with the smallest (key_t(y), y), compared lexicographically.  key_t(y) is the
 *     64-bit word w1 << 32 | w0 of the draw (call key of (seed, c_i, TG_TAG_SEAL_HOP), id = y, d0 = t, d1 = 0): the call key is
 *     Philox4x32-10(key = seed, counter = (c_i, TG_TAG_SEAL_HOP, "tchg")) words 0 and 1, the draw Philox4x32-10(key = call
 *     key, counter = (d0, d1, id low, id high)), as DESIGN.md "Randomness" has it.
 *   N_t = N_{t-1} united with S_t.  A vertex dropped in hop t is not in N_t and may be found again, under a fresh key, in hop
 *     t + 1.  This matches SEAL-OGB.
 *   N = N_h.  From there on du, dv, z, z_max, the output order (u, v, then ascending id) and rounds are those of
 *     tchgeo_seal.h, unchanged.
 *   Refusals per slot are unchanged: bit 1, an end outside the graph (checked first); bit 2, u == v; bit 0, |N| > node_cap.
 *   cut[i] (optional, int64) has bit t - 1 set iff |F_t| > k_t > 0.  A refused slot gets cut = 0.
 * The keys are independent per (slot, hop, vertex), so S_t is a uniform k_t-subset of F_t.  Nothing depends on the order of
 * insertion, on the form, or on which slot of which launch holds the link: the result is a function of (graph, link, parameters,
 * seed, call id).
 *
 * THE POOL.  A capped hop gathers its candidates in a pool in LDS, in both forms: TG_SEAL_POOL_PLACES(k) places of open
 *   addressing and TG_SEAL_POOL_CAP(k) listed candidates.  A hop whose fringe passes TG_SEAL_POOL_CAP(k_t) is compacted to its
 *   k_t smallest while it runs; the result does not depend on that.
 *
 * FORMS and WORKSPACE: tg_seal_nodes', with the same formula.  The LDS form's reach does not shrink: node_cap <=
 *   TG_SEAL_LDS_CAP takes it at every cap (fewer workgroups stay resident on a CU).
 *   tg_seal_capped_workspace_bytes reports the form taken all the same.
 *
 * LIMITS: k_t in [0, TG_SEAL_HOP_CAP_MAX]; everything else as tg_seal_nodes.  A null caps or max_per_hop, a cap outside the
 *   limits and everything tg_seal_nodes refuses are refused with TG_ERR_INVALID before anything is launched; m = 0 launches
 *   nothing.  The call is stream-ordered, allocates nothing, does not synchronise and reads nothing back; max_per_hop is read
 *   before the call returns. */
#ifndef TCHGEO_SEAL_CAPPED_H
#define TCHGEO_SEAL_CAPPED_H

#include "tchgeo_seal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_TAG_SEAL_HOP 19u /* DESIGN.md "Randomness": the next free tag */
#define TG_SEAL_HOP_CAP_MAX 1024
#define TG_SEAL_POOL_PLACES(k) ((k) <= 256 ? 1024 : (k) <= 512 ? 2048 : 4096) /* the least power of two >= max(1024, 4 k) */
#define TG_SEAL_POOL_CAP(k) (TG_SEAL_POOL_PLACES(k) / 2)

typedef struct {
    const int32_t *max_per_hop; /* host [num_hops]: k_t, 0 = the hop is not capped */
    uint64_t seed;
    const int64_t *call_ids;    /* device [m] or NULL */
    int64_t call_id0;           /* c_i = call_id0 + i when call_ids is NULL */
    int64_t *cut;               /* device [m] or NULL */
} tg_seal_caps;

/* max_cap: the largest k_t of the call.  *form_taken (may be NULL): the form a call with these sizes runs.  Touches no device. */
TG_API int tg_seal_capped_workspace_bytes(int64_t m, int32_t node_cap, int32_t max_cap, int32_t form, int64_t *bytes,
                                          int32_t *form_taken);
TG_API int tg_seal_nodes_capped(const tg_graph *g, const tg_seal_in *in, const tg_seal_caps *caps, const tg_seal_out *out,
                                int64_t m, int32_t form, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
