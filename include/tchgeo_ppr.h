/* Approximate personalised PageRank by forward push (Andersen, Chung and Lang, FOCS 2006; the sampler of ShaDow-GNN and of
 * PPRGo; PyG's torch_geometric.utils.ppr.get_ppr) behind libtchgeo_hip.so: tg_ppr_topk (csrc/ppr.hip).  Plain C99; an
 * additive part of the C ABI of tchgeo.h, kept in a header of its own.
 *
 * Mass is counted in units of 2^-31 (U = 2^31): every estimate and every residual fits a uint32 and every sum is an integer
 * add whose order does not matter, so the operator is a function of (graph, seeds, parameters).
 *
 * THE RULE, for slot i with seed s = seeds[i] on the view g:
 *   Pushes go along the entries of g's major as tg_random_walk reads it (a CSR view gives the usual out-edge PPR); parallel
 *   entries count separately; d(v) = the length of v's row.
 *   State: a table of touched vertices with an estimate p[v] and a residual r[v]; it starts as {s: p = 0, r = U}.
 *   A round; every decision reads the residuals as they stood when the round began:
 *     v with d(v) > 0: q = floor(floor(r[v] * (2^32 - alpha_q) / 2^32) / d(v)); v is ACTIVE iff r[v] >= eps_q * d(v) (a
 *       64-bit compare) and q >= 1.  An active v adds a = floor(alpha_q * q * d(v) / (2^32 - alpha_q)) to p[v], adds q to the
 *       residual of the target of every one of its entries (which touches it) and keeps r[v] - a - q * d(v).
 *     v with d(v) = 0 is active iff r[v] >= 1; it moves its whole residual into p[v].
 *     A vertex that is not active keeps its residual and still receives.
 *   The slot ends after the first round without an active vertex, or after max_rounds rounds.
 *   rounds[i] = the rounds that had an active vertex; activations[i] = A = the (vertex, round) pairs that were active.
 *
 * PROPERTIES
 *   sum p + sum r = U after every round.  An activation takes a + q d out of r[v] (a + q d <= r[v]: q d <= r (1 - alpha) and
 *     a <= q d alpha / (1 - alpha) <= r alpha, alpha = alpha_q / 2^32) and puts a into p[v] and q into d residuals; a sink
 *     moves its residual into its estimate; nothing else changes either sum.
 *   -A <= U * ppr_s(v) - p[v] <= sum r + A for every v, ppr_s = exact PPR with restart alpha and a self loop at every empty
 *     row.  An exact push of rho = q d / (1 - alpha) from v puts alpha rho = a + f into p[v], 0 <= f < 1, and q on every
 *     entry, and keeps U ppr_s(x) = p[x] + sum_u r[u] ppr_u(x) (the push invariant, linear in p and r; emptying a sink into
 *     p is the limit of pushes round its self loop).  An activation is that push with f left behind in r[v] instead of
 *     p[v]: after A of them U ppr_s(x) - p[x] = sum_u r[u] ppr_u(x) + sum_j f_j ([x = v_j] - ppr_{v_j}(x)), the first sum
 *     in [0, sum r], every term of the second in (-1, 1).
 *
 * CAPACITY: a slot that has touched more than node_cap distinct vertices after some round is refused: status bit 0 (value 1),
 *   count[i] = 0 and nothing else is written for it.  The touched vertices of a round are a set, so the refusal does not
 *   depend on the order of insertion.  A seed outside [0, g->n_major) gives count[i] = 0, nothing else, and status bit 1
 *   (value 2).
 *
 * OUTPUT per slot, rows of pitch k (as tg_pinsage_hop lays out neighbors / visits): the seed first, whatever its rank; then
 *   the other touched vertices with p > 0 by p descending, then id ascending; count[i] = min(k, 1 + their number).
 *   nodes[i][j], score[i][j] (the p words) and weight[i][j] (float32: (float)p * 2^-31f, one conversion and one exact
 *   scaling) for j < count[i]; nothing behind count[i] in a row is written.  Per slot, for the conservation law and the bound
 *   above: touched[i], rounds[i], activations[i], residual[i] = sum r and mass[i] = sum p over the whole table.  weight and
 *   each of the five may be NULL.
 *
 * FORMS (equal words): one workgroup owns a slot from its first round to its row of output.
 *   TG_PPR_FORM_LDS        the table lives in LDS: node_cap <= TG_PPR_LDS_CAP; no workspace
 *   TG_PPR_FORM_WORKSPACE  the table lives in the caller's workspace: node_cap up to TG_PPR_MAX_CAP
 *   TG_PPR_FORM_AUTO       _LDS up to its limit, else _WORKSPACE
 *   Workspace: 8-byte aligned; 0 bytes for the LDS form (it may be NULL), else with T = the least power of two >=
 *   max(1024, 2 * node_cap) and G = min(m, TG_PPR_WS_GROUPS): bytes = G * (16 * T + 4 * node_cap rounded up to 256).
 *
 * LIMITS: alpha_q in [1, 2^32 - 1], eps_q in [1, 2^31], max_rounds in [1, 65536], node_cap in [1, 2^20], k in [1, node_cap],
 *   m in [0, 2^31); g->n_major above 2^31 is TG_ERR_UNSUPPORTED (ids are 32-bit words with 2^32 - 1 for an empty place).
 *   Null buffers, sizes outside the limits, an unknown form, the LDS form above its cap and a short or misaligned workspace
 *   are refused with TG_ERR_INVALID before anything is launched; m = 0 launches nothing.  The call is stream-ordered,
 *   allocates nothing, does not synchronise and reads nothing back.  `status`: one device int32, zeroed by the caller,
 *   OR-ed into.  indices32 / ptrs32 are used when given, with equal words. */
#ifndef TCHGEO_PPR_H
#define TCHGEO_PPR_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_PPR_UNIT 2147483648ll /* U = 2^31 */
#define TG_PPR_MAX_ROUNDS 65536
#define TG_PPR_MAX_CAP 1048576 /* 2^20 */
#define TG_PPR_LDS_CAP_SMALL 512 /* node_cap up to here: a table of 1024 places in LDS */
#define TG_PPR_LDS_CAP 2048      /* up to here: a table of 4096 places in LDS */
#define TG_PPR_WS_GROUPS 128     /* workgroups (tables) of the workspace form */
#define TG_PPR_FORM_AUTO 0
#define TG_PPR_FORM_LDS 1
#define TG_PPR_FORM_WORKSPACE 2

typedef struct {
    const int64_t *seeds; /* device [m] */
    uint32_t alpha_q;     /* restart probability * 2^32 */
    uint32_t eps_q;       /* push threshold per unit of degree, in units of 2^-31 */
    int32_t max_rounds;
    int32_t k;            /* pitch of the output rows */
    int32_t node_cap;     /* touched vertices per slot at most */
} tg_ppr_in;

typedef struct {
    int64_t *count;       /* device [m] */
    int64_t *nodes;       /* device [m, k] */
    int64_t *score;       /* device [m, k]: p */
    float *weight;        /* device [m, k] or NULL: p * 2^-31 */
    int64_t *touched, *rounds, *activations, *residual, *mass; /* device [m] each, or NULL */
} tg_ppr_out;

/* *form_taken (may be NULL): the form a call with these sizes runs.  Touches no device. */
TG_API int tg_ppr_workspace_bytes(int64_t m, int32_t k, int32_t node_cap, int32_t form, int64_t *bytes, int32_t *form_taken);
TG_API int tg_ppr_topk(const tg_graph *g, const tg_ppr_in *in, const tg_ppr_out *out, int64_t m, int32_t form,
                       int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
