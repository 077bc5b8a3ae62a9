/* Streaming last-k neighbour state (the sampler of the memory-based temporal GNNs: TGN, Rossi et al. 2020; PyG's
 * torch_geometric.nn.models.tgn.LastNeighborLoader) behind libtchgeo_hip.so: tg_lastn_reset / _insert / _sample / _replay
 * (csrc/lastn.hip).  Plain C99; an additive part of the C ABI of tchgeo.h, kept in a header of its own.
 *
 * A second kind of adjacency beside the finished CSC: device resident, fed events as they happen, bounded per node.  At any
 * moment it answers "the k most recent interactions of these nodes" in O(k) per node without rebuilding anything, and it does
 * so behind tg_ns_homo_batched's output contract: tg_ns_homo_unique, tg_ns_homo_compact and tg_gather_rows apply unchanged.
 * Deterministic: no draw is made anywhere.
 *
 * STATE (public layout; the bytes are a pure function of the insertion history, so a plain copy is a checkpoint):
 *   count[n_nodes]    int64: entries ever inserted for the node; the array is padded to a multiple of 256 bytes
 *   slot[n_nodes][k]  16 bytes each, {int64 nbr, int64 e_id}, behind the counts
 *   entry number c of a node (0-based, in insertion order) lives in slot c % k; a slot never written holds {-1, -1}
 *   state_bytes = r256(8 * n_nodes) + 16 * n_nodes * k;  1 <= k <= 64, 1 <= n_nodes <= 2^31; `state` 16-byte aligned
 *
 * INSERT: event j of (src, dst, e_id) gives entry 2j = (node dst_j, nbr src_j, e_id_j) and, under `symmetric`, entry 2j+1 =
 *   (node src_j, nbr dst_j, e_id_j); without `symmetric` only the first exists.  e_id == NULL: e_id_j = e_base + j.  Entries
 *   are appended to their node's history in entry order (a self loop under `symmetric` is two entries of one node, as in
 *   PyG).  An entry whose node lies outside [0, n_nodes) is dropped and raises status bit 1 (value 2); the neighbour is not
 *   checked.  A node with old count n and c entries in the call gets its entry of batch-rank r in slot (n + r) % k; only
 *   ranks >= c - k are written, so no slot has two writers and the result does not depend on scheduling; count becomes n + c.
 *   n_events in [0, 2^22]; 0 launches nothing.  Two forms leave equal state bytes:
 *     TG_LASTN_FORM_LDS   one workgroup: the packed words (node, entry index) are sorted in LDS, a node's entries are then
 *                         one run and the rank is the place in the run.  At most TG_LASTN_LDS_ENTRIES entries (events, or
 *                         2 * events under `symmetric`); needs no workspace.
 *     TG_LASTN_FORM_GRID  any size, with the workspace: a table keyed by node counts the call's entries per node, then k
 *                         rounds of a maximum over the not yet placed entry indices name the newest, second newest, ...
 *                         entry of every node; a last launch writes the counts (every round reads the old ones).
 *     TG_LASTN_FORM_AUTO  _LDS up to its limit, else _GRID.
 *   workspace_bytes >= tg_lastn_insert_workspace_bytes (0 where the LDS form is taken; the workspace may then be NULL), 8-byte
 *   aligned.  With T = the least power of two >= max(64, 2 * entries): bytes = r256(8 T) + 5 r256(4 T) + r256(4 entries).
 *
 * SAMPLE: tg_ns_homo_batched's output contract with the ring as the adjacency.  Per batch b: samples = seeds ++ hop-1
 *   samples ++ ..., rows[e] = n_seeds + e, cols[e] = position of the parent in samples, edge_index[e] = the entry's e_id,
 *   layer_offsets[h] = (len(samples), len(edges), len(samples)) when hop h starts, counts = {n_samples, n_edges}; capacities
 *   from tg_ns_homo_capacity; tg_ns_out.rows_prefilled is honoured; `states` is not touched.  A frontier vertex v
 *   contributes its min(fanout[h], min(count_v, k)) newest entries, newest first: entries count_v - 1, count_v - 2, ...
 *   1 <= fanout[h] <= k, 0 <= n_hops <= TG_MAX_HOPS.  A seed outside [0, n_nodes) contributes nothing and raises status bit 1
 *   (value 2); a stored neighbour outside the range is emitted as a sample and is an empty frontier slot in the next hop
 *   (no status).  Words past the counts are not written.  No workspace.  One workgroup per batch walks the hops.
 *
 * REPLAY: G = ceil(n_events / step_events) steps in ONE call: step g samples row g of `seeds` ([G, n_seeds]) into batch g
 *   of `out`, then inserts events [g * step_events, min((g + 1) * step_events, n_events)) symmetrically with e_id = e_base +
 *   index.  A chain of launches on the caller's stream (the kernels of tg_lastn_sample and tg_lastn_insert under
 *   TG_LASTN_FORM_AUTO), word for word the G pairs of calls; no host round trip, no kernel waits on another.
 *   workspace: tg_lastn_replay_workspace_bytes(step_events) = the insert's for step_events symmetric events.
 *
 * Every call is stream-ordered, allocates nothing, does not synchronise and reads nothing back.  `status`: one device int32,
 * zeroed by the caller, OR-ed into.  Null pointers, sizes outside the limits, a short state, a short or misaligned
 * workspace and an unknown form are refused with TG_ERR_INVALID before anything is launched. */
#ifndef TCHGEO_LASTN_H
#define TCHGEO_LASTN_H

#include "tchgeo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_LASTN_MAX_K 64
#define TG_LASTN_MAX_NODES 2147483648ll /* 2^31 */
#define TG_LASTN_MAX_EVENTS 4194304     /* 2^22 per insert / replay call */
#define TG_LASTN_LDS_ENTRIES 4096       /* entries the one-workgroup insert sorts in LDS */
#define TG_LASTN_FORM_AUTO 0
#define TG_LASTN_FORM_LDS 1
#define TG_LASTN_FORM_GRID 2

typedef struct {
    void *state;         /* device, 16-byte aligned */
    int64_t state_bytes; /* >= tg_lastn_state_bytes(n_nodes, k) */
    int64_t n_nodes;
    int32_t k;
} tg_lastn;

/* touches no device */
TG_API int tg_lastn_state_bytes(int64_t n_nodes, int32_t k, int64_t *bytes);
/* counts = 0, every slot = {-1, -1} */
TG_API int tg_lastn_reset(const tg_lastn *st, void *stream);

/* *form_taken (may be NULL): the form a call with these sizes runs */
TG_API int tg_lastn_insert_workspace_bytes(int64_t n_events, int32_t symmetric, int32_t form, int64_t *bytes,
                                           int32_t *form_taken);
TG_API int tg_lastn_insert(const tg_lastn *st, const int64_t *src, const int64_t *dst, const int64_t *e_id /* NULL: e_base + j */,
                           int64_t e_base, int64_t n_events, int32_t symmetric, int32_t *status, void *workspace,
                           int64_t workspace_bytes, int32_t form, void *stream);

/* seeds: device [n_batches, n_seeds]; out: n_batches slabs */
TG_API int tg_lastn_sample(const tg_lastn *st, const int64_t *seeds, int64_t n_batches, int64_t n_seeds, const int64_t *fanout,
                           int32_t n_hops, const tg_ns_out *out, int32_t *status, void *stream);

TG_API int tg_lastn_replay_workspace_bytes(int64_t step_events, int64_t *bytes);
/* seeds: device [G, n_seeds]; out: G slabs, G = ceil(n_events / step_events) */
TG_API int tg_lastn_replay(const tg_lastn *st, const int64_t *src, const int64_t *dst, int64_t e_base, int64_t n_events,
                           int64_t step_events, const int64_t *seeds, int64_t n_seeds, const int64_t *fanout, int32_t n_hops,
                           const tg_ns_out *out, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
