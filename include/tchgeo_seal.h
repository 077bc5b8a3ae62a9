/* SEAL enclosing subgraphs with double-radius node labels (Zhang and Chen, NeurIPS 2018; the labeling trick of Zhang et al.,
 * NeurIPS 2021; PyG's examples/seal_link_pred.py: k_hop_subgraph + shortest_path per link) behind libtchgeo_hip.so:
 * tg_seal_nodes (csrc/seal.hip).  Plain C99; an additive part of the C ABI of tchgeo.h, kept in a header of its own.
 *
 * THE RULE.  Slot i holds the link (u, v) = (src[i], dst[i]) on the view g.
 *   Neighbours: the neighbours of x are the entries of x's row of g's major, as tg_random_walk and tg_ppr_topk read it.  A
 *     CSC view walks in-edges, which is PyG's k_hop_subgraph with flow="source_to_target"; callers who want SEAL's undirected
 *     subgraph pass a symmetric graph.  Parallel entries and self loops change nothing.
 *   Node set: N = every vertex at distance <= h = num_hops from u or from v in the whole graph.  This BFS masks nothing: it
 *     passes through u and v.
 *   Distances: du(x), for x in N \ {v}, is the BFS distance from u to x using only vertices of N \ {v}; dv(x) is the same
 *     from v, over N \ {u}.  Both have UNBOUNDED depth: a shortest path that leaves N does not count, a path longer than h that
 *     stays inside N does.  du(v) = dv(u) = -1, and an unreached vertex gets -1.  Removing v for du and u for dv removes the
 *     target link and all its parallel entries in both directions.
 *   Label: z(u) = z(v) = 1; z(x) = 0 if du(x) < 0 or dv(x) < 0; otherwise, with d = du + dv,
 *     z(x) = 1 + min(du, dv) + (d div 2) * (d div 2 + d mod 2 - 1), computed in 64 bits.  If z_max > 0, z is then clamped to
 *     z_max.  As a check: (1,1) -> 2, (1,2) -> 3, (1,3) -> 4, (2,2) -> 5, (1,4) -> 6, (2,3) -> 7.
 *
 * OUTPUT per slot, in rows of pitch node_cap: count[i] = |N|; nodes[i][.] = u, then v, then the other vertices of N by id
 *   ascending; z[i][.] (int64) and, where given, du[i][.] and dv[i][.] (int64) in that order.  Nothing behind count[i] in a row
 *   is written.  rounds[i] (optional) = the number of restricted rounds that reached a new vertex: a round is one step of
 *   both restricted searches together, so this is the largest du or dv of the slot.
 *
 * REFUSALS per slot: each gives count[i] = 0, writes nothing else for the slot and leaves the other slots unaffected.
 *   more than node_cap vertices in N: status bit 0 (value 1).  The vertices of a hop are a set, so this does not depend on the
 *     order of insertion.
 *   an endpoint outside [0, g->n_major): status bit 1 (value 2); checked first.
 *   u == v: status bit 2 (value 4).
 *
 * FORMS (equal words): one workgroup owns a slot from its first hop to its rows of output.
 *   TG_SEAL_FORM_LDS        the table lives in LDS: node_cap <= TG_SEAL_LDS_CAP; no workspace
 *   TG_SEAL_FORM_WORKSPACE  the table lives in the caller's workspace: node_cap up to TG_SEAL_MAX_CAP
 *   TG_SEAL_FORM_AUTO       _LDS up to its limit, else _WORKSPACE
 *   Workspace: 8-byte aligned; 0 bytes for the LDS form (it may be NULL), else with T = the least power of two >=
 *   max(1024, 2 * node_cap) and G = min(m, TG_SEAL_WS_GROUPS): bytes = G * (16 * T + T / 4 + 4 * node_cap rounded up to 256).
 *
 * LIMITS: num_hops in [1, 64], node_cap in [2, 2^20], z_max >= 0, m in [0, 2^31); g->n_major above 2^31 is TG_ERR_UNSUPPORTED
 *   (ids are 32-bit words with 2^32 - 1 for an empty place).  Null required buffers, sizes outside the limits, an unknown form,
 *   the LDS form above its cap and a short or misaligned workspace are refused with TG_ERR_INVALID before anything is launched;
 *   m = 0 launches nothing.  The call is stream-ordered, allocates nothing, does not synchronise and reads nothing back.
 *   `status`: one device int32, zeroed by the caller, OR-ed into.  indices32 / ptrs32 are used when given, with equal words. */
#ifndef TCHGEO_SEAL_H
#define TCHGEO_SEAL_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_SEAL_MAX_HOPS 64
#define TG_SEAL_MAX_CAP 1048576 /* 2^20 */
#define TG_SEAL_LDS_CAP_SMALL 512 /* node_cap up to here: a table of 1024 places in LDS */
#define TG_SEAL_LDS_CAP 2048      /* up to here: a table of 4096 places in LDS */
#define TG_SEAL_WS_GROUPS 128     /* workgroups (tables) of the workspace form */
#define TG_SEAL_FORM_AUTO 0
#define TG_SEAL_FORM_LDS 1
#define TG_SEAL_FORM_WORKSPACE 2
#define TG_SEAL_STATUS_CAP 1
#define TG_SEAL_STATUS_RANGE 2
#define TG_SEAL_STATUS_SAME 4

typedef struct {
    const int64_t *src; /* device [m]: u */
    const int64_t *dst; /* device [m]: v */
    int32_t num_hops;   /* h */
    int32_t node_cap;   /* vertices per slot at most; the pitch of the output rows */
    int64_t z_max;      /* 0: labels are not clamped */
} tg_seal_in;

typedef struct {
    int64_t *count;  /* device [m] */
    int64_t *nodes;  /* device [m, node_cap] */
    int64_t *z;      /* device [m, node_cap] */
    int64_t *du;     /* device [m, node_cap] or NULL */
    int64_t *dv;     /* device [m, node_cap] or NULL */
    int64_t *rounds; /* device [m] or NULL */
} tg_seal_out;

/* *form_taken (may be NULL): the form a call with these sizes runs.  Touches no device. */
TG_API int tg_seal_workspace_bytes(int64_t m, int32_t node_cap, int32_t form, int64_t *bytes, int32_t *form_taken);
TG_API int tg_seal_nodes(const tg_graph *g, const tg_seal_in *in, const tg_seal_out *out, int64_t m, int32_t form,
                         int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
