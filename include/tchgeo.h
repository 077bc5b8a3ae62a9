/*
 * tchgeo.h -- C ABI of the MI355X (gfx950) graph-sampling backend that replaces
 * tch-geometric's CPU samplers (reference: the files under src/algo) behind its Python
 * operator surface (reference: src/python.rs, tch_geometric/tch_geometric.pyi).
 *
 * Conventions
 *  - plain C: raw device pointers + sizes, no torch / HIP types in signatures
 *    (`stream` is a hipStream_t passed as void*; NULL = the default stream);
 *  - every entry point is stream-ordered and never synchronises, allocates or
 *    frees: the caller owns every buffer, including outputs and workspaces;
 *  - all indices are int64 (reference: src/utils/types.rs:4-9), weights are
 *    float64 (python.rs:214), timestamps int64 (python.rs:149);
 *  - return value: TG_OK or a TG_ERR_* code; tg_last_error() gives the text of
 *    the last failure on the calling thread;
 *  - randomness: counter-addressed Philox4x32-10.  A draw is named by
 *    (seed, call_id, operator tag, id, d0, d1); results do not depend on
 *    launch geometry, and equal the CPU oracle's philox-mode bit for bit.
 *    (The reference's own stream -- one sequential Xoshiro256++ threaded
 *    through every vertex with data-dependent rejection, utils/random.rs +
 *    rand 0.8.5 -- cannot be reproduced by any parallel device; DESIGN.md.)
 */
#ifndef TCHGEO_H
#define TCHGEO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_API __attribute__((visibility("default")))

#define TG_OK 0
#define TG_ERR_INVALID 1     /* bad argument (null pointer, negative size, unsupported fan-out ...) */
#define TG_ERR_HIP 2         /* a HIP runtime call failed */
#define TG_ERR_UNSUPPORTED 3 /* valid request this build does not implement */

#define TG_MAX_HOPS 8
#define TG_MAX_FANOUT 32 /* per-hop fan-out handled by the register-resident sampler; larger fan-outs (<= 255 while
                            the LDS holds them) take a slower LDS-resident form with identical results */

/* Adjacency resident in HBM, borrowed for the call: replaces
 * SparseGraph{ptrs,indices} (src/data/graph.rs:34-38) and EdgeAttr
 * (graph.rs:104-120).  CSC for neighbor sampling / HGT, CSR for walks and
 * negative sampling; rows must be sorted ascending inside a column
 * (to_csc/to_csr guarantee it, src/data/storage.rs:112,119). */
typedef struct {
    const int64_t *ptrs;       /* [n_major + 1] */
    const int64_t *indices;    /* [n_edges] */
    const double *weights;     /* [n_edges] or NULL  (WeightedSampler, neighbor_sampling.rs:131-158) */
    const int64_t *timestamps; /* [n_edges] or NULL  (TemporalFilter, neighbor_sampling.rs:36-77) */
    int64_t n_major;
    int64_t n_edges;
    const uint32_t *indices32; /* optional u32 shadow of `indices` (all ids < 2^32): same values, half the bytes per
                                  gathered line; NULL = not provided.  Outputs stay int64 either way. */
    const uint32_t *ptrs32;    /* optional u32 shadow of `ptrs` (n_edges < 2^32): 4 B per offset, so the whole
                                  offset table of RMAT-24 (67 MB) stays in the Infinity Cache; NULL = not provided */
    int64_t max_degree;        /* optional: the longest column (row) of the graph, 0 = unknown (n_edges is assumed).  The
                                  window-ordered launch packs sampled positions into max_degree's bits; a
                                  value SMALLER than the truth is a contract violation like an out-of-range id.
                                  tg_graph_max_degree computes it on the device. */
} tg_graph;

typedef struct {
    uint64_t seed;
    uint64_t call_id; /* batch b of a batched call uses call_id + b */
} tg_rng;

/* Sampler variants of python.rs:210-216 */
#define TG_SAMPLER_UNIFORM 0      /* UnweightedSampler<false> -- the default (python.rs:215) */
#define TG_SAMPLER_UNIFORM_REPL 1 /* UnweightedSampler<true> */
#define TG_SAMPLER_WEIGHTED 2     /* WeightedSampler<f64> */
/* Additive (the reference has no such sampler; PyG calls it temporal_strategy="last"): the k MOST RECENT admitted edges.
 * For a frontier vertex w with filter state s, column [ptrs[w], ptrs[w+1]) and fan-out k:
 *   admitted  the edges the temporal filter passes (TG_FILTER_NONE: all; STATIC / RELATIVE / DYNAMIC with `forward`
 *             exactly as neighbor_sampling.rs:55-67, in wrapping int64 arithmetic like the other filtered kernels);
 *   rank      forward == 0: the larger timestamp first; forward == 1: the smaller timestamp first (under TG_FILTER_NONE
 *             the configuration's `forward` still selects the direction); ties: the smaller edge pointer first; the
 *             comparison is on the full int64 timestamp;
 *   output    the first min(k, n_admitted) edges in rank order, with the per-vertex bookkeeping of
 *             neighbor_sampling.rs:210-218; a sample's state is the filter's `mutate` (the edge's timestamp under DYNAMIC,
 *             s otherwise; without a filter no states are kept and `states` may be NULL).
 * No random draw is made: rng, id_base, ids and call_ids do not influence the result.  Fan-outs 1..64 per hop,
 * tg_graph.timestamps required, columns of fewer than 2^32 - 1 edges (checked against the graph's sizes: a graph of
 * 2^32 - 1 edges or more must state tg_graph.max_degree, and that must be below the limit); anything else is TG_ERR_INVALID.  Taken by
 * tg_ns_hop_recent and, with a workspace, tg_ns_homo_batched_ws; every other entry point rejects or ignores the id. */
#define TG_SAMPLER_RECENT 3
/* Additive: LAYER-NEIGHBOR sampling (LABOR-0, Balin & Catalyurek, NeurIPS 2023; DGL's LaborSampler, GraphBolt's
 * sample_layer_neighbor).  Every graph vertex t gets ONE variate per call id and layer, shared by every frontier vertex
 * of that call; a frontier vertex keeps the k admitted edges whose neighbours have the smallest variates.  For ONE
 * frontier vertex with distinct neighbours this is a uniform k-subset (the rank order of iid keys is a uniform
 * permutation); ACROSS frontier vertices of a mini-batch the choices are maximally correlated, so fewer distinct vertices
 * are sampled.  For a frontier vertex v holding graph vertex w, with call id c (call_ids[v], else rng.call_id; in a
 * batched launch rng.call_id + b), filter state s, fan-out k, hop h:
 *   admitted  as TG_SAMPLER_RECENT: tg_filter_pass in wrapping int64, every edge under TG_FILTER_NONE;
 *   key       of edge pointer e with t = indices[e]: a >> 1, a = the low 64 bits of the draw (call key of (rng.seed, c,
 *             tag), id = t, d0 = layer, d1 = 0); layer = h for TG_SAMPLER_LABOR, 0 for TG_SAMPLER_LABOR_SHARED (the same
 *             variates at every hop: LABOR's layer dependency); tag = rng_tag, 0 meaning TG_TAG_LABOR.  A 63-bit
 *             non-negative int64: an empty entry (INT64_MAX, position 2^32 - 1) ranks behind every edge;
 *   rank      the smaller key first; ties (parallel edges to the same t) to the smaller edge pointer;
 *   output    the first min(k, n_admitted) edges in rank order; bookkeeping and the filter's mutate as TG_SAMPLER_RECENT.
 * ids and id_base do not influence the result; weights are ignored; timestamps are needed only under a filter.  Fan-outs
 * 1..64, columns shorter than 2^32 - 1 edges (TG_SAMPLER_RECENT's check), no seed_ids / seed_call_ids; anything else is
 * TG_ERR_INVALID before any launch.  Taken by tg_ns_hop_labor and, with a workspace, tg_ns_homo_batched_ws; every other
 * entry point rejects the ids. */
#define TG_SAMPLER_LABOR 4         /* fresh variates per hop      */
#define TG_SAMPLER_LABOR_SHARED 5  /* the same variates at every hop (LABOR's layer dependency) */
#define TG_TAG_LABOR 14u           /* first number no TAG_* uses */
/* tg_ns_hop_labor: a column of more than this many edges is scanned by one workgroup of 16 wavefronts, not by one
 * wavefront.  Results do not depend on the value. */
#define TG_LABOR_LONG_COLUMN 32768
/* Filter variants of python.rs:218-249 */
#define TG_FILTER_NONE (-1)
#define TG_FILTER_STATIC 0   /* TEMPORAL_SAMPLE_STATIC   (neighbor_sampling.rs:32) */
#define TG_FILTER_RELATIVE 1 /* TEMPORAL_SAMPLE_RELATIVE */
#define TG_FILTER_DYNAMIC 2  /* TEMPORAL_SAMPLE_DYNAMIC */

typedef struct {
    int32_t sampler;     /* TG_SAMPLER_* */
    int32_t filter_mode; /* TG_FILTER_* */
    int32_t forward;     /* TemporalFilter FORWARD */
    uint32_t rng_tag;    /* operator tag of the draw address; 0 = the homogeneous default.  The heterogeneous
                            sampler runs one relation-hop at a time with TG_TAG_NS_HETERO | relation << 8 */
    int64_t win_lo, win_hi;       /* inclusive window (python.rs:150) */
    const int64_t *seeds_state;   /* [n_batches * n_seeds] initial filter state, or NULL */
    int64_t id_base;              /* draw id of slot i is id_base + i (slot of the vertex in its sample list) */
    /* Remote-frontier mode (range-partitioned graphs, n_hops == 1 only): seed i of batch b is some OTHER sampler's
     * frontier vertex; it is sampled with that sampler's draws: id = seed_ids[b*n_seeds+i], call id =
     * seed_call_ids[b*n_seeds+i] (instead of id_base + i and rng.call_id + b).  Both NULL = off. */
    const int64_t *seed_ids;
    const int64_t *seed_call_ids;
} tg_ns_config;

#define TG_TAG_NS_HOMO 1u
#define TG_TAG_NS_HETERO 2u

/* Per-batch output slabs of neighbor_sampling_homogenous.  Batch b owns
 * samples[b*cap_nodes ..], rows/cols/edge_index[b*cap_edges ..],
 * layer_offsets[b*n_hops*3 ..], counts[b*2 ..] = {n_samples, n_edges}.
 * `states` ([n_batches*cap_nodes]) is workspace for temporal filters, else NULL. */
typedef struct {
    int64_t *samples;
    int64_t *rows;
    int64_t *cols;
    int64_t *edge_index;
    int64_t *layer_offsets;
    int64_t *counts;
    int64_t *states;
    int64_t cap_nodes; /* >= tg_ns_homo_capacity() */
    int64_t cap_edges;
    /* rows[e] = n_seeds + e whatever was sampled: for a given n_seeds the `rows` slab of every batch is the same arange in
     * every launch.  0 = off.  1 + n_seeds = the caller states that rows[b*cap_edges + e] == n_seeds + e for EVERY
     * e < cap_edges of every batch (tg_ns_rows_fill writes that); a launch whose own n_seeds matches MAY then leave `rows`
     * unwritten.  The unfiltered, unweighted tg_ns_homo_batched / _ws launches do (the fused per-batch kernel and both
     * pipelines of the window-ordered form: 8 of the 32 bytes written per sampled edge); the weighted / filtered samplers
     * and the partitioned emit passes ignore the field and write `rows`, which is always correct.  A launch with another
     * n_seeds writes `rows` as with 0 -- the slab then no longer holds what the field states, and the caller clears it.
     * Readers of `rows` (tg_ns_homo_compact, tg_ns_homo_unique, tg_ns_induced_*, the partitioned protocol) never look at
     * the field: the pointer is always valid and always holds the values.  Whoever overwrites `rows` (tg_ns_homo_unique
     * with an in-place result) ends the statement: pass 0 from then on.  Zero-initialise the struct (tg_ns_out o = {0}). */
    int64_t rows_prefilled;
} tg_ns_out;

/* rows[b*cap_edges + e] = n_seeds + e for e < cap_edges, b < n_batches: what tg_ns_out.rows_prefilled = 1 + n_seeds
 * states.  One streaming pass, once per slab (not per launch).  `rows` 8-byte aligned.  Stream-ordered. */
TG_API int tg_ns_rows_fill(int64_t *rows, int64_t n_batches, int64_t cap_edges, int64_t n_seeds, void *stream);

/* *max_degree_dev (device int64) = the longest column of `g` (reads ptrs32 when given, else ptrs).  Stream-ordered. */
TG_API int tg_graph_max_degree(const tg_graph *g, int64_t *max_degree_dev, void *stream);

TG_API const char *tg_version(void);
TG_API const char *tg_last_error(void);

/* Worst-case slab sizes for n_seeds seeds and fan-outs k_0..k_{H-1}:
 * cap_edges = sum_h n_seeds*k_0*...*k_h, cap_nodes = n_seeds + cap_edges. */
TG_API int tg_ns_homo_capacity(int64_t n_seeds, const int64_t *fanout, int32_t n_hops, int64_t *cap_nodes,
                        int64_t *cap_edges);

/* neighbor_sampling_homogenous (src/algo/neighbor_sampling.rs:162-230; binding
 * python.rs:187-271) for n_batches independent seed batches in one launch.
 * seeds: [n_batches * n_seeds] device int64.  Output layout per batch is the
 * reference's: samples = seeds ++ hop-1 samples ++ ..., rows[e] = n_seeds + e,
 * cols[e] = slot of the parent, edge_index[e] = CSC edge pointer,
 * layer_offsets[h] = (len(samples), len(edges), len(samples)) when hop h starts. */
TG_API int tg_ns_homo_batched(const tg_graph *csc, const int64_t *seeds, int64_t n_batches, int64_t n_seeds,
                       const int64_t *fanout, int32_t n_hops, const tg_ns_config *cfg, const tg_rng *rng,
                       const tg_ns_out *out, void *stream);

/* The same operator with a caller-provided workspace (tg_ns_homo_workspace_bytes; 256-byte aligned).  With it, a
 * launch of many batches (unweighted, unfiltered samplers, fan-outs <= TG_MAX_FANOUT) runs hop by hop over the whole
 * device and issues the `indices[edge_ptr]` gathers of a hop in ADDRESS order (items of the hop's frontier
 * counting-sorted by window of their column start, windows dealt to XCDs), so that each 128-byte line of `indices` is
 * fetched about once per hop instead of once per sampled neighbour.  Outputs are identical to tg_ns_homo_batched
 * (output positions are fixed by per-batch prefix sums, neighbor_sampling.rs:212-217); launches that do not qualify
 * fall through to it.  workspace == NULL is tg_ns_homo_batched.  `mode`: TG_NS_FORM_AUTO picks the form by launch size
 * (many batches against a graph far larger than the L2s), _WINDOWED takes it whenever the launch qualifies, _FUSED never. */
#define TG_NS_FORM_AUTO 0
#define TG_NS_FORM_WINDOWED 1
#define TG_NS_FORM_FUSED 2
#define TG_NS_FORM_WINDOWED_WIDE 3 /* _WINDOWED with the 24-byte work items that launches beyond 32-bit offsets use */
/* (the size includes the staged pipeline's stage slots only while tg_ns_win_tuning.staged is on at the time of the query;
 * a launch whose workspace lacks them takes the push form) */
TG_API int tg_ns_homo_workspace_bytes(int64_t n_batches, int64_t n_seeds, const int64_t *fanout, int32_t n_hops,
                               int64_t *n_bytes);
/* The same for a given graph: the staged pipeline's stage slots are then sized by the graph's bit widths (vertex ids and
 * tg_graph.max_degree: one 64-byte chunk per frontier vertex where the pairs {neighbour, position} fit, else two); without
 * a graph the larger size is assumed, and under tg_ns_win_tuning.staged = 2 (AUTO) the slots are included from 2 048
 * batches on, so that a launch whose graph has one-chunk slots can take the staged pipeline with it. */
TG_API int tg_ns_homo_workspace_bytes_for(const tg_graph *csc, int64_t n_batches, int64_t n_seeds, const int64_t *fanout,
                                   int32_t n_hops, int64_t *n_bytes);
/* The workspace for a launch with THIS sampler / filter configuration: the window-ordered form's for the plain samplers
 * (as above); for the weighted sampler or a temporal filter with at most 256 batches, the workspace of the FLAT path -- the
 * launch then runs hop by hop over the whole device (tg_ns_hop_scan / tg_ns_hop_weighted_groups on all batches' frontiers
 * at once) instead of one workgroup per batch: 64 weighted batches of 1 024 seeds on RMAT-24 53 -> 15 ms, temporal 5.5 ->
 * 2.3 ms; 8 batches 47 -> 2.2 / 5.2 -> 0.55 ms.  Results are tg_ns_homo_batched's bit for bit (the per-batch kernel runs behind the flat path whenever that could
 * not finish: a column-group bound reached, a non-positive weight sum).  0 bytes: the launch takes no workspace.
 * TG_SAMPLER_RECENT (with or without a filter) has no per-batch kernel: it takes the flat path at ANY batch count with
 * tg_ns_hop_recent as the hop, nothing can overflow and nothing is queued behind it; the workspace is REQUIRED
 * (tg_ns_homo_batched, a null, short or misaligned workspace, and seed_ids / seed_call_ids are TG_ERR_INVALID).
 * TG_SAMPLER_LABOR / TG_SAMPLER_LABOR_SHARED likewise, with tg_ns_hop_labor as the hop (hop h passes layer h, or 0 when
 * shared) and its long-column list inside the workspace; tg_ns_homo_batched_form reports TG_NS_FORM_FUSED for them. */
TG_API int tg_ns_homo_batched_workspace_bytes(const tg_graph *csc, int64_t n_batches, int64_t n_seeds, const int64_t *fanout,
                                       int32_t n_hops, const tg_ns_config *cfg, int64_t *n_bytes);
TG_API int tg_ns_homo_batched_ws(const tg_graph *csc, const int64_t *seeds, int64_t n_batches, int64_t n_seeds,
                          const int64_t *fanout, int32_t n_hops, const tg_ns_config *cfg, const tg_rng *rng,
                          const tg_ns_out *out, void *workspace, int64_t workspace_bytes, int32_t mode, void *stream);

/* Which form a tg_ns_homo_batched_ws call with these arguments runs: *form = TG_NS_FORM_FUSED (the per-batch kernel; also
 * reported for the weighted / filtered samplers, which take neither), _WINDOWED (16-byte work items) or _WINDOWED_WIDE;
 * *n_windows (optional) = windows the hop's frontier is sorted into.  A pure query: nothing is launched. */
TG_API int tg_ns_homo_batched_form(const tg_graph *csc, int64_t n_batches, int64_t n_seeds, const int64_t *fanout,
                            int32_t n_hops, const tg_ns_config *cfg, const tg_ns_out *out, int64_t workspace_bytes,
                            int32_t mode, int32_t *form, int32_t *n_windows);

/* Which PIPELINE of the window-ordered form the call takes under the current tuning: *staged = 1 the staged one (gather
 * into stage slots, then emit; needs the larger workspace), 0 the push one or no window-ordered form at all.  A pure query. */
TG_API int tg_ns_homo_batched_pipeline(const tg_graph *csc, int64_t n_batches, int64_t n_seeds, const int64_t *fanout,
                                int32_t n_hops, const tg_ns_config *cfg, const tg_ns_out *out, int64_t workspace_bytes,
                                int32_t mode, int32_t *staged);

/* Tuning of the window-ordered form (process-wide; defaults come from TG_WIN_* environment variables read once).
 * Outputs never depend on it.  _set: a zero field (negative for the four flags) keeps the current value. */
typedef struct {
    int64_t window_bytes;    /* bytes of the gathered array per window (default 512 KiB) */
    int32_t gather_blocks;   /* workgroups of the persistent gather kernel (default 256) */
    int32_t gather_threads;  /* its workgroup size (default 512) */
    int32_t emit_threads;    /* workgroup size of the emit kernels (default 256) */
    int32_t direct_hop0;     /* hop 0 issues its gathers itself, unordered (default 1) */
    int32_t fuse_first_hops; /* seeds + hop 0 + hop 1's emit pass in one kernel (default 1) */
    int32_t fold_hist;       /* emit kernels persistent, window histogram of the items kept in LDS instead of a pass of its
                                own over the items (default 1; needs the two flags above and >= 2 hops) */
    int32_t emit_blocks;     /* workgroups of the persistent emit kernels (default 768, at most 1024) */
    int32_t staged;          /* gather first, emit afterwards through packed 64-byte stage slots: 0 = never,
                                1 = whenever it applies, 2 (default) = where it measures faster than the push form: launches
                                of >= 2 048 batches whose slots are one chunk; launches it does not fit -- ordered fan-outs
                                > 30, ids beyond 32 bits, a workspace without the slots -- take the push form anyway;
                                < 0 in _set keeps */
    int32_t stage_round_chunks;   /* staged emit kernel: 64-slot chunks per round (default 2: the smaller tile lets five workgroups share a CU, emit 3.15 -> 3.07 ms; at most 16) */
    int32_t stage_gather_threads; /* staged gather kernel: workgroup size (default 512) */
    int32_t stage_gather_blocks;  /* ... and workgroups (default 512) */
    int32_t stage_emit_threads;   /* staged emit kernel: workgroup size (default 256) */
    int32_t stage_parts;          /* staged form: the last hop runs in this many parts (batch ranges), part p's emit pass on
                                     a side stream beside part p + 1's sort and gather (default 1 = one stream: measured, the overlap
                                     buys nothing -- both kernels are bound by vector-ALU work -- and every part costs 0.2 ms) */
    int32_t stage_part_min_batches; /* ... as long as every part keeps at least this many batches (default 1024) */
    int32_t stage_sort_blocks;      /* staged form: workgroups of the item sort = rows of its histogram = persistent workgroups
                                       of the first kernel (at most 1024).  Default -1 = auto: as many as stay resident on the
                                       device -- per CU what the first kernel's LDS request and its 128 VGPRs allow, as
                                       hipOccupancyMaxActiveBlocksPerMultiprocessor confirms (MI355X, u32 `ptrs32` shadow: 4 x 256);
                                       _set: 0 keeps, < 0 = auto; _get reports -1 for auto */
    int32_t stage_fine;             /* staged form: second sort level (tiles of the coarse-sorted items ordered by vertex in LDS,
                                       so that a gather workgroup's slice lies in a few columns; default 1; < 0 in _set keeps) */
    int32_t stage_concurrent;       /* staged form, two hops, several parts: the parts' whole chains alternate between the caller's
                                       stream and the side stream (default 0; < 0 in _set keeps) */
    int32_t stage_split;            /* staged form: rows / cols / edge_index of an ordered hop are written by a pass of their own on
                                       the side stream, beside the hop's sort and gather; the emit pass writes `samples` only
                                       (< 0 in _set keeps) */
    int32_t stage_split_round_chunks; /* ... whose tiles hold this many 64-slot chunks (default 4; 0 in _set keeps) */
    int32_t store_align64;          /* the emit passes' store instructions start on 64-byte boundaries (the elements before the
                                       first boundary are stored alone): non-temporal stores of a chunk that two instructions
                                       share go out as two partial writes (default 1; 0: 16-byte boundaries; < 0 in _set keeps) */
    int32_t stage_fine_sub_bits;    /* staged form: the second sort level orders a window's vertices into 1 << this many sub-ranges
                                       (4 .. 7, default 7: the finer the order, the fewer columns a gather workgroup's slice touches --
                                       gather 2.39 / 2.26 / 2.11 / 2.01 ms at 4 / 5 / 6 / 7, the sort 0.46 / 0.47 / 0.52 / 0.56; 0 in _set keeps) */
    int32_t stage_fine_blocks;      /* staged form: workgroups of the second sort level's two passes (default 2048, rounded up to a
                                       multiple of 8; 0 in _set keeps) */
} tg_ns_win_tuning;
TG_API int tg_ns_win_tuning_get(tg_ns_win_tuning *t);
TG_API int tg_ns_win_tuning_set(const tg_ns_win_tuning *t);

/* The staged pipeline's first kernel (seeds, hop 0, the items of hop 1).  _first_lds_bytes: the workgroup size (*threads,
 * optional) and dynamic LDS request it takes for `emit_threads`, the launch's largest fan-out, the coarse buckets and
 * windows of the graph, and the form of its column starts (narrow = 1: u32, graphs with the `ptrs32` shadow) -- pure
 * arithmetic, no device needed.  _first_launch: what the last staged launch of this process gave it (rows = persistent
 * workgroups, workgroups_per_cu = what auto derived, 0 under a forced stage_sort_blocks).  Measurement and tests only. */
TG_API int tg_ns_win_first_lds_bytes(int32_t emit_threads, int32_t kmax, int32_t n_coarse_buckets, int32_t n_windows,
                              int32_t narrow, int32_t *threads, int64_t *lds_bytes);
TG_API int tg_ns_win_first_launch(int32_t *rows, int32_t *workgroups_per_cu, int32_t *threads, int32_t *narrow, int64_t *lds_bytes);

/* Per-stage times of the window-ordered launch: tg_ns_win_stage_timing(1) makes every later launch record HIP events
 * between its kernels (on its stream); tg_ns_win_stage_times waits for the last launch and returns up to `cap` stage
 * durations in ms with their names (24 bytes each, "<stage>.h<hop>").  Measurement only. */
TG_API int tg_ns_win_stage_timing(int32_t enable);
TG_API int tg_ns_win_stage_times(float *ms, char *names, int32_t cap, int32_t *n);

/* One hop of the unweighted, unfiltered sampler over a flat frontier, spread over the whole device (the
 * per-vertex work of neighbor_sampling.rs:195-218 without the per-batch bookkeeping).  Used where the frontier
 * is not "one seed batch": the owner side of the range-partitioned sampler, relation-hops of the heterogeneous
 * sampler.  Vertex i of the frontier is sampled with draw id ids[i] (or id_base + i) and call id call_ids[i]
 * (or rng.call_id); vertices < 0 are empty slots.  Outputs are sized for the worst case m * fanout;
 * offsets[m] is the number of samples.  No synchronisation.  Fan-outs up to 4096: above 128 one wavefront per vertex
 * runs the ticket chain with its displaced entries in LDS (the batched kernel stops at 255). */
typedef struct {
    const int64_t *vertices; /* [m] */
    const int64_t *ids;      /* [m] or NULL */
    const int64_t *call_ids; /* [m] or NULL */
    int64_t m;
    int64_t id_base;
    int32_t fanout;
    int32_t sampler;  /* TG_SAMPLER_UNIFORM or TG_SAMPLER_UNIFORM_REPL (tg_ns_hop_recent: TG_SAMPLER_RECENT;
                         tg_ns_hop_labor: TG_SAMPLER_LABOR / _LABOR_SHARED) */
    uint32_t rng_tag; /* 0 = TG_TAG_NS_HOMO (tg_ns_hop_labor: TG_TAG_LABOR) */
    uint32_t _reserved;
} tg_hop_in;

typedef struct {
    int64_t *cnt;       /* [m] samples per frontier vertex */
    int64_t *offsets;   /* [m + 1] exclusive prefix of cnt */
    int64_t *neighbors; /* [m * fanout] indices[edge_ptr], grouped by frontier vertex in reservoir-slot order */
    int64_t *edge_ptrs; /* [m * fanout] */
    int64_t *parents;   /* [m * fanout] index of the frontier vertex */
} tg_hop_out;

TG_API int tg_ns_hop_workspace_bytes(int64_t m, int64_t *bytes);
TG_API int tg_ns_hop(const tg_graph *csc, const tg_hop_in *in, const tg_rng *rng, const tg_hop_out *out,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* The same flat hop for the unweighted samplers UNDER A TEMPORAL FILTER (neighbor_sampling.rs:36-77): columns are
 * cut into groups of 512 edges that are counted all over the device, then every vertex draws its ranks (ticket
 * form) and fetches them.  `states` is the filter state of every frontier vertex, states_out [m * fanout] that of
 * every sample.  group_cap bounds the number of 512-edge groups the frontier's columns may have
 * (sum of ceil(deg / 512)); if it is reached status[0] (device int32, zeroed by the caller) becomes 1 and all
 * counts are 0 -- retry with a larger workspace. */
typedef struct {
    int32_t filter_mode; /* TG_FILTER_STATIC / RELATIVE / DYNAMIC */
    int32_t forward;
    int64_t win_lo, win_hi; /* inclusive window */
    const int64_t *states;  /* [m]  Fan-outs up to 1024 (above 64 the ticket chain keeps its displaced
 * entries in LDS). */
} tg_hop_filter;

TG_API int tg_ns_hop_scan_workspace_bytes(int64_t m, int32_t fanout, int64_t group_cap, int64_t *bytes);
TG_API int tg_ns_hop_scan(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *filter, const tg_rng *rng,
                          const tg_hop_out *out, int64_t *states_out, int32_t *status, void *workspace,
                          int64_t workspace_bytes, int64_t group_cap, void *stream);

/* The flat hop of TG_SAMPLER_RECENT (in->sampler must say so; semantics at the define): one wavefront per frontier vertex
 * streams the column's timestamps 64 at a time and keeps the best 64 one per lane; a chunk none of whose admitted edges
 * beats the current k-th entry is skipped after one ballot.  A hub column is scanned by ONE wavefront.  `filter` NULL =
 * no filter, most recent first; a filter with filter_mode = TG_FILTER_NONE admits every edge and carries `forward`.
 * Outputs as tg_ns_hop_scan's (cnt, offsets with offsets[m] the total, neighbors / edge_ptrs / parents grouped by frontier
 * vertex, here in RANK order); states_out [m * fanout] may be NULL without a filter and is then not written.  Vertices < 0
 * are empty slots.  No workspace, no status word (nothing can overflow), no synchronisation; fan-outs 1..64. */
TG_API int tg_ns_hop_recent(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *filter, const tg_hop_out *out,
                            int64_t *states_out, void *stream);

/* The flat hop of TG_SAMPLER_LABOR / TG_SAMPLER_LABOR_SHARED (in->sampler must be one of them; semantics at the defines;
 * `layer` is the d0 of the key's address and is used as given: the caller passes the hop for TG_SAMPLER_LABOR and 0 for
 * _SHARED).  tg_ns_hop_recent's shape with a Philox draw of the neighbour's id as the key: one wavefront per frontier
 * vertex for columns of up to TG_LABOR_LONG_COLUMN edges; longer ones are listed in the workspace (m + 32 words:
 * tg_ns_hop_labor_workspace_bytes) and taken by a second kernel, one workgroup of 16 wavefronts per long vertex, whose 16
 * partial lists meet in LDS.  Same result word for word either way.  `filter` NULL or filter_mode = TG_FILTER_NONE: every
 * edge is admitted and the timestamps are not read.  Outputs as tg_ns_hop_recent's.  No status word, no synchronisation. */
TG_API int tg_ns_hop_labor_workspace_bytes(int64_t m, int64_t *bytes);
TG_API int tg_ns_hop_labor(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *filter, const tg_rng *rng,
                           int32_t layer, const tg_hop_out *out, int64_t *states_out, void *workspace,
                           int64_t workspace_bytes, void *stream);
/* Measurement and tests only: the long-column threshold of later tg_ns_hop_labor launches of this process (0 restores
 * TG_LABOR_LONG_COLUMN); *previous (optional) = the value it replaces.  Results do not depend on it. */
TG_API int tg_ns_hop_labor_long_column(int64_t edges, int64_t *previous);

/* The flat hop for the WEIGHTED sampler (sampling.rs:28-55), with or without a temporal filter (filter = NULL or
 * filter_mode = TG_FILTER_NONE: none).  One wavefront per frontier vertex all over the device; a column's
 * left-to-right f64 running sum is kept exactly.  status[0] |= 2 where the reference panics (sum <= 0).
 * Workspace: tg_ns_hop_scan_workspace_bytes(m, fanout, 1). */
TG_API int tg_ns_hop_weighted(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *filter, const tg_rng *rng,
                              const tg_hop_out *out, int64_t *states_out, int32_t *status, void *workspace,
                              int64_t workspace_bytes, void *stream);
/* The same hop in the GROUP FORM: the columns are cut into the 512-edge groups of the filtered hop above; chunk totals and
 * draws run flat over the groups of ALL frontier columns, the carries of the blocked running sum per column between
 * them -- a hub column no longer occupies one wavefront or one workgroup while the device idles (RMAT-24, 64 batches of
 * 1 024 seeds: 39.7 -> 15.3 ms).  Same draws, same sums, same result.  group_cap >= 1024 bounds the frontier's groups as in
 * tg_ns_hop_scan (reached: status[0] |= 1, all counts 0 -- retry with more); workspace:
 * tg_ns_hop_weighted_workspace_bytes(m, fanout, group_cap) (64 bytes more per group than the filtered hop's).
 * tg_ns_hop_segments with the weighted sampler takes this form under the same condition and needs the same workspace. */
TG_API int tg_ns_hop_weighted_workspace_bytes(int64_t m, int32_t fanout, int64_t group_cap, int64_t *bytes);
TG_API int tg_ns_hop_weighted_groups(const tg_graph *csc, const tg_hop_in *in, const tg_hop_filter *filter, const tg_rng *rng,
                                     const tg_hop_out *out, int64_t *states_out, int32_t *status, void *workspace,
                                     int64_t workspace_bytes, int64_t group_cap, void *stream);

/* neighbor_sampling_heterogenous (src/algo/neighbor_sampling.rs:233-356; binding python.rs:275-395) in ONE launch for
 * n_batches independent seed batches, unweighted samplers without filter (the surface's default).  Node types and
 * relations are indexed in the caller's `node_types` / `edge_types` order, which is also the order relations are
 * visited in every hop (the reference iterates a HashMap there).  Host arrays describe the problem; the pointers
 * inside are device pointers.  Batch b owns samples[t][b*cap_nodes[t] ..], rows/cols/edge_index[r][b*cap_edges[r] ..],
 * layer_offsets[((b*n_rels + r)*n_hops + h)*3 ..] = (len(samples[src]), len(edges r), len(samples[dst])) when hop h
 * reaches relation r (:314-315), counts[b*(n_types+n_rels) ..] = {len(samples[t])..., len(edges r)...}.
 * Draw address: tag TG_TAG_NS_HETERO | r << 8, id = slot of the frontier vertex in its type's list, call id
 * rng.call_id + b.  Weighted / filtered heterogeneous sampling is driven per (hop, relation) through
 * tg_ns_homo_batched / tg_ns_hop_scan / tg_ns_hop_weighted with the same addresses. */
#define TG_HET_MAX_TYPES 8
#define TG_HET_MAX_RELS 16
typedef struct {
    int32_t n_types, n_rels, n_hops;
    int32_t sampler;               /* TG_SAMPLER_UNIFORM or TG_SAMPLER_UNIFORM_REPL */
    const int32_t *rel_src;        /* [n_rels] node type sampled FROM (CSC rows) */
    const int32_t *rel_dst;        /* [n_rels] node type whose frontier is expanded (CSC columns) */
    const tg_graph *graphs;        /* [n_rels] CSC per relation */
    const int64_t *fanout;         /* [n_rels * n_hops]; 0 = relation not sampled in that hop */
    const int64_t *const *inputs;  /* [n_types] device [n_batches * n_inputs[t]], NULL where n_inputs[t] == 0 */
    const int64_t *n_inputs;       /* [n_types] seeds per batch */
} tg_het_problem;

typedef struct {
    int64_t *const *samples;    /* [n_types] device slabs [n_batches * cap_nodes[t]] */
    const int64_t *cap_nodes;   /* [n_types] >= tg_ns_hetero_capacity() */
    int64_t *const *rows;       /* [n_rels] device slabs [n_batches * cap_edges[r]] */
    int64_t *const *cols;
    int64_t *const *edge_index;
    const int64_t *cap_edges;   /* [n_rels] */
    int64_t *layer_offsets;     /* device [n_batches * n_rels * n_hops * 3] */
    int64_t *counts;            /* device [n_batches * (n_types + n_rels)] */
} tg_het_out;

TG_API int tg_ns_hetero_capacity(const tg_het_problem *problem, int64_t *cap_nodes, int64_t *cap_edges);
TG_API int tg_ns_hetero_batched(const tg_het_problem *problem, int64_t n_batches, const tg_rng *rng, const tg_het_out *out,
                                void *stream);

/* Device-side bookkeeping for neighbor_sampling_heterogenous (neighbor_sampling.rs:292-352) when its (hop, relation)
 * steps run as flat hops -- temporal filters, the weighted sampler, sizes beyond the fused launch: list lengths,
 * frontier slices and edge counts live in `meta` (device, tg_het_meta_words int64 words:
 * len[T] | fbeg[T] | fend[T] | ne[R] | layer_offsets[R][H][3] | scratch words; the caller initialises len = fend =
 * number of inputs, fbeg = 0, ne = 0), so a call needs no read-back between steps.  Per hop, per relation in
 * `edge_types` order: tg_het_step_begin (frontier = list[dst][fbeg, fend) into a buffer of cap_f slots padded with -1,
 * draw ids = slot in the list, layer_offsets[rel][hop]) -> tg_ns_hop / tg_ns_hop_scan / tg_ns_hop_weighted with m =
 * cap_f -> tg_het_step_end (append samples / states to list[src], (row, col, edge pointer) to the relation's lists,
 * advance the lengths; status |= 4 if a capacity were exceeded); after the relations tg_het_hop_end. */
TG_API int tg_het_meta_words(int32_t n_types, int32_t n_rels, int32_t n_hops, int64_t *words);
TG_API int tg_het_step_begin(const int64_t *list_dst, const int64_t *state_dst, int64_t *meta, int32_t n_types, int32_t n_rels,
                             int32_t n_hops, int32_t src, int32_t dst, int32_t rel, int32_t hop, int64_t cap_f,
                             int64_t *frontier, int64_t *fstate, int64_t *ids, void *stream);
TG_API int tg_het_step_end(const tg_hop_out *out, const int64_t *states_out, int64_t cap_f, int32_t fanout, int64_t *meta,
                           int32_t n_types, int32_t n_rels, int32_t n_hops, int32_t src, int32_t rel, int64_t *list_src,
                           int64_t *state_src, int64_t cap_list, int64_t *rows, int64_t *cols, int64_t *edge_index,
                           int64_t cap_edges, int32_t *status, void *stream);
TG_API int tg_het_hop_end(int64_t *meta, int32_t n_types, int32_t n_rels, int32_t n_hops, void *stream);

/* The same hop with ALL its relations in one set of launches (a per-call operator is bound by its number of launches).
 * A hop's frontier is fixed when the hop starts (neighbor_sampling.rs:345-348 advance the slices at its end), so the
 * relations' frontiers are concatenated (entry j owns slots [begin, begin + cap) of the concatenation, cap = its
 * worst-case frontier size), sampled by ONE tg_ns_hop_segments call, and their appends are replayed in relation order:
 *   tg_het_hop_begin_all  snapshots lengths / edge counts / frontier starts; builds the concatenated frontier (-1
 *                         padded), its draw ids and filter states.
 *   tg_ns_hop_segments    the flat filtered / weighted hop over a frontier made of up to TG_HOP_MAX_SEGMENTS segments,
 *                         each with its own graph, fan-out and draw tag (hop_in.fanout / rng_tag are ignored;
 *                         hop_in.sampler = TG_SAMPLER_WEIGHTED takes tg_ns_hop_weighted's algorithm, the unweighted
 *                         samplers tg_ns_hop_scan's and need a filter).  Outputs are compact over the concatenation, so a
 *                         segment's samples are contiguous; `parents` index the concatenation.  Workspace:
 *                         tg_ns_hop_scan_workspace_bytes(m, largest fan-out, group_cap).
 *   tg_het_hop_end_all    for the entries in order: layer_offsets[rel][hop], append samples / states / edges, advance
 *                         lengths and edge counts; `last` != 0 also sets the next hop's frontier slices.  out_cap: an
 *                         upper bound of the hop's samples (sizes the launch).
 * layout_dev (device, [segments + 1], NULL = none): the frontier WITHOUT its padding -- tg_het_hop_begin_all packs the
 * segments' real frontiers back to back and writes their starts and the total there; tg_ns_hop_segments and
 * tg_het_hop_end_all then work on the real length (the host-side begin / cap / m stay the worst case that sizes the
 * launches).  Needs m <= 2^17 and group_cap <= 2^20.
 * Entries list EVERY relation sampled in the hop, in `edge_types` order, also those whose frontier is necessarily empty
 * (segment = -1: only their layer offset is recorded).  More than TG_HET_HOP_MAX_ENTRIES relations or
 * TG_HOP_MAX_SEGMENTS segments: several begin / sample / end rounds, `last` on the final one. */
#define TG_HOP_MAX_SEGMENTS 8
#define TG_HET_HOP_MAX_ENTRIES 16
typedef struct {
    const tg_graph *graph;
    int64_t begin;    /* first frontier slot of the segment; ascending, segment 0 starts at 0 */
    int32_t fanout;
    uint32_t rng_tag; /* 0 = TG_TAG_NS_HOMO */
} tg_hop_segment;
typedef struct {
    int32_t rel, src, dst;
    int32_t segment;                      /* >= 0: the relation has a frontier segment in this round; -1: none */
    int64_t begin, cap;                   /* its slots in the concatenated frontier */
    const int64_t *list_dst, *state_dst;  /* sample list / filter states of the dst type (the frontier is read there) */
    int64_t *list_src, *state_src;        /* sample list / filter states of the src type (samples are appended) */
    int64_t cap_list_src;
    int64_t *rows, *cols, *edge_index;    /* the relation's edge lists */
    int64_t cap_edges;
} tg_het_entry;
TG_API int tg_ns_hop_segments(const tg_hop_segment *segments, int32_t n_segments, const tg_hop_in *in,
                              const int64_t *layout_dev, const tg_hop_filter *filter, const tg_rng *rng,
                              const tg_hop_out *out, int64_t *states_out, int32_t *status, void *workspace,
                              int64_t workspace_bytes, int64_t group_cap, void *stream);
TG_API int tg_het_hop_begin_all(const tg_het_entry *entries, int32_t n_entries, int64_t *meta, int32_t n_types, int32_t n_rels,
                                int32_t n_hops, int64_t m_total, int64_t *frontier, int64_t *fstate, int64_t *ids,
                                int64_t *layout_dev, void *stream);
TG_API int tg_het_hop_end_all(const tg_het_entry *entries, int32_t n_entries, const tg_hop_out *out, const int64_t *states_out,
                              int64_t m_total, int64_t out_cap, const int64_t *layout_dev, int64_t *meta, int32_t n_types,
                              int32_t n_rels, int32_t n_hops, int32_t hop, int32_t last, int32_t *status, void *stream);

/* neighbor_sampling_homogenous over a RANGE-PARTITIONED CSC (graphs beyond one GPU's HBM; host protocol in
 * tch_geometric/partitioned.py; SURVEY.md 8(e) mode 2).  The origin rank keeps ordinary
 * tg_ns_out slabs; per hop: tg_part_requests (origin) -> all-to-all -> tg_part_count + tg_part_sample (owner) ->
 * all-to-all -> tg_part_emit (origin).  Results equal tg_ns_homo_batched on the replicated graph bit for bit (requests
 * carry the requester's draw address).  EVERY size stays on the device (kernels read the number of requests from
 * device memory): with world == 1 nothing is read back; with world > 1 the host reads only the all-to-all split sizes.
 *  - request: 16 bytes {int64 vertex; uint32 batch; uint32 slot}; the requester's call id = its first call id + batch.
 *  - request_cap = n_batches * the widest frontier (< 2^32); workspace: tg_part_workspace_bytes, 256-byte aligned.
 *  - tg_part_begin: copies the seeds into the slabs, frontier = the seeds.
 *  - tg_part_requests: `requests` [<= request_cap] grouped by owner = min(vertex / shard_size, world-1);
 *    send_counts[world + 1] (device): requests per owner, then their total.
 *  - tg_part_count: owner of columns [v_lo, v_lo + shard.n_major).  m_dev: number of received requests (device);
 *    m_cap: host-known upper bound of it (sizes the launches and the prefix sum); seg_off[world + 1] (host): requests of
 *    requesting rank p are [seg_off[p], seg_off[p+1]); seg_call0[world] (host): that rank's first call id.
 *    -> cnt[m] u32 samples per request, off[m + 1] their exclusive prefix (off[m] = total), reply_counts[world + 1] (device): reply entries
 *    per requesting rank, then their total.  scan_tmp: tg_part_scan_workspace_bytes(m_cap).
 *  - tg_part_sample: reply [sum cnt] entries = (neighbour id, global edge pointer = local pointer + e_lo), compact, in
 *    request order; unweighted samplers, fanout <= TG_MAX_FANOUT.
 *  - reply_format (the same value on every rank; entry size in int64 words in brackets):
 *    TG_PART_REPLY_PAIRS [2] neighbour, edge pointer; TG_PART_REPLY_TRIPLES [3] + the sample's filter state;
 *    TG_PART_REPLY_PACKED [1] neighbour | edge pointer << 32 -- valid when the whole graph has < 2^32 vertices and
 *    < 2^32 edges, halves what the reply all-to-all moves; TG_PART_REPLY_PACKED_STATE [2] packed word, filter state.
 *  - tg_part_emit: cnt / reply as returned to the origin (request order); cnt_prefix: the exclusive prefix of cnt if
 *    the caller already holds it (world == 1: tg_part_count's `off`), else NULL; hop_cap = n_batches * this hop's
 *    widest frontier; compacts the replies into the slabs in slot order, advances the frontier, writes layer_offsets[hop],
 *    counts. */
#define TG_PART_REPLY_PACKED 1
#define TG_PART_REPLY_PAIRS 2
#define TG_PART_REPLY_TRIPLES 3
#define TG_PART_REPLY_PACKED_STATE 4
TG_API int tg_part_workspace_bytes(int64_t n_batches, int64_t request_cap, int32_t world, int64_t *bytes);
TG_API int tg_part_scan_workspace_bytes(int64_t n, int64_t *bytes);
TG_API int tg_part_begin(const int64_t *seeds, const int64_t *seeds_state, int64_t n_batches, int64_t n_seeds, int32_t n_hops,
                         const tg_ns_out *out, int64_t request_cap, int32_t world, void *workspace, void *stream);
TG_API int tg_part_requests(const tg_ns_out *out, int64_t n_batches, int64_t request_cap, int64_t shard_size, int32_t world,
                            void *workspace, void *requests, int64_t *request_states, int64_t *send_counts, void *stream);
TG_API int tg_part_count(const tg_graph *shard, int64_t v_lo, const void *requests, const int64_t *m_dev, int64_t m_cap,
                         int32_t world, const int64_t *seg_off, const uint64_t *seg_call0, int32_t fanout, int32_t sampler,
                         uint32_t *cnt, int64_t *off, int64_t *reply_counts, void *scan_tmp, int64_t scan_tmp_bytes,
                         void *stream);
TG_API int tg_part_sample(const tg_graph *shard, int64_t v_lo, int64_t e_lo, const void *requests, const int64_t *m_dev,
                          int64_t m_cap, int32_t world, const int64_t *seg_off, const uint64_t *seg_call0, int32_t fanout,
                          int32_t sampler, uint64_t seed, const uint32_t *cnt, const int64_t *off, int64_t *reply,
                          int32_t reply_format, void *stream);
/* Temporal filters and the weighted sampler (neighbor_sampling.rs:36-77, :131-158) on a partitioned graph: the origin
 * also sends every frontier vertex's filter state (seeds_state / request_states [<= request_cap], grouped like the
 * requests; NULL = no filter); the owner unpacks the requests into the flat-hop input arrays (tg_part_unpack: vertices
 * rebased to the shard, -1 for padding; draw ids = the requesters' slots; call ids = the requesters'), runs
 * tg_ns_hop_scan / tg_ns_hop_weighted over them (m = m_cap, shard.timestamps / shard.weights = the shard's slices) and
 * packs the hop's compact outputs into the reply (tg_part_pack: cnt u32, entries in reply_format, reply_counts).
 * tg_part_emit with a reply_format that carries the filter state also fills the `states` slab.  Same draws as the replicated sampler, so the same results. */
/* tg_part_sample with a workspace (tg_part_sample_workspace_bytes(m_cap); 256-byte aligned): hops with many requests
 * (>= 2^21) against a large shard are first counting-sorted by the WINDOW of their column (found from the vertex id through
 * a vertex -> window table) and sampled in that order, XCD by XCD, so that the `indices[edge_ptr]` gathers hit L2 instead
 * of costing a line request each; the replies are the same words in the same places.  workspace == NULL or a small hop:
 * tg_part_sample. */
TG_API int tg_part_sample_workspace_bytes(int64_t m_cap, int64_t *bytes);
/* when tg_part_sample_ws orders a hop (process-wide; defaults 2^21 requests, 2^24 shard edges; negative = keep).  Results
 * never depend on it; tests lower the thresholds to run the ordered path on small graphs. */
TG_API int tg_part_sample_order_thresholds(int64_t min_requests, int64_t min_edges);
TG_API int tg_part_sample_ws(const tg_graph *shard, int64_t v_lo, int64_t e_lo, const void *requests, const int64_t *m_dev,
                      int64_t m_cap, int32_t world, const int64_t *seg_off, const uint64_t *seg_call0, int32_t fanout,
                      int32_t sampler, uint64_t seed, const uint32_t *cnt, const int64_t *off, int64_t *reply,
                      int32_t reply_format, void *workspace, int64_t workspace_bytes, void *stream);
/* Slot replies (unweighted, unfiltered sampling; round 4).  Instead of tg_part_count + tg_part_sample's compact reply the
 * owner answers every request with ONE fixed-size packed slot -- {column start : 32, cnt : 8, fanout x {neighbour :
 * vertex_bits, position inside the column : position_bits}} in W = 16 or 32 32-bit words (tg_part_slot_words; 0 = no
 * format: fan-out > 16 or more than 1024 bits) -- written at the request's index: slots [m_cap][W], 64-byte aligned.
 * The reply all-to-all carries W words per request with the request exchange's split sizes mirrored, so the host reads
 * back ONE set of sizes per hop instead of two, and neither side runs a count / prefix pass.  vertex_bits = bits of the
 * largest vertex id of the WHOLE graph, position_bits = bits of (longest column of the whole graph - 1): every rank
 * passes the same values.  A shard holds < 2^32 edges.  workspace: tg_part_sample_workspace_bytes(m_cap) (hops with many
 * requests are sampled in window order, as tg_part_sample_ws) or NULL.  order_scale (>= 1) multiplies the request threshold
 * of that ordering for this hop: a call's FIRST hop asks about its seeds -- mostly short columns that are read whole, one
 * or two lines each -- and pays for the ordering only from about 4 x as many requests on (pass 4 there, 1 for later hops).
 * tg_part_emit_slots: slots as returned to the origin (its send-buffer order); e_lo_of: host [world], the global edge
 * offset of every rank's shard -- a sample's edge pointer = e_lo_of[owner] + column start + position.
 * Same draws as tg_part_sample, so the same results as the replicated sampler. */
TG_API int tg_part_slot_words(int32_t fanout, int32_t vertex_bits, int32_t position_bits, int32_t *words);
TG_API int tg_part_sample_slots(const tg_graph *shard, int64_t v_lo, const void *requests, const int64_t *m_dev, int64_t m_cap,
                                int32_t world, const int64_t *seg_off, const uint64_t *seg_call0, int32_t fanout,
                                int32_t sampler, uint64_t seed, int32_t vertex_bits, int32_t position_bits, int32_t order_scale,
                                void *slots, void *workspace, int64_t workspace_bytes, void *stream);
TG_API int tg_part_emit_slots(const tg_ns_out *out, int64_t n_batches, int64_t n_seeds, int64_t request_cap, int32_t world,
                              int32_t fanout, int32_t hop, int32_t n_hops, void *workspace, const void *slots,
                              int32_t vertex_bits, int32_t position_bits, const int64_t *e_lo_of, void *stream);
TG_API int tg_part_unpack(int64_t v_lo, int64_t n_major, const void *requests, const int64_t *m_dev, int64_t m_cap,
                          int32_t world, const int64_t *seg_off, const uint64_t *seg_call0, int64_t *vertices, int64_t *ids,
                          int64_t *call_ids, void *stream);
TG_API int tg_part_pack(const tg_hop_out *hop, const int64_t *states_out, const int64_t *m_dev, int64_t m_cap, int64_t e_lo,
                        int32_t world, const int64_t *seg_off, uint32_t *cnt, int64_t *reply, int32_t reply_format,
                        int64_t *reply_counts, void *stream);
TG_API int tg_part_emit(const tg_ns_out *out, int64_t n_batches, int64_t n_seeds, int64_t request_cap, int64_t hop_cap,
                        int32_t world, int32_t fanout, int32_t hop, int32_t n_hops, void *workspace, const uint32_t *cnt,
                        const int64_t *cnt_prefix, const int64_t *reply, int32_t reply_format, void *stream);

/* random_walk (src/algo/random_walk.rs:10-75; binding python.rs:584-608).
 * walks: [n, walk_length + 1] device int64, -1 padded after a dead end. */
TG_API int tg_random_walk(const tg_graph *csr, const int64_t *start, int64_t n, int64_t walk_length, float p, float q,
                   const tg_rng *rng, int64_t *walks, void *stream);

/* The EDGE SET of a CSR: SparseGraph::has_edge (src/data/graph.rs:80-83, a binary search of the row: ~log2(deg) dependent
 * random line requests) as one hash probe.  node2vec with p != q asks has_edge once per proposal (random_walk.rs:57-63);
 * with the set a 1 M-walker call on RMAT-24 takes a quarter of the time, with the same walks.  Optional: built once per
 * graph by the caller (8 bytes x the next power of two >= 2 x n_edges; vertex ids must be < 2^32 - 1), handed to
 * tg_random_walk_es; edge_set = NULL is tg_random_walk. */
TG_API int tg_edge_set_bytes(const tg_graph *csr, int64_t *bytes);
TG_API int tg_edge_set_build(const tg_graph *csr, void *edge_set, int64_t bytes, void *stream);
TG_API int tg_random_walk_es(const tg_graph *csr, const void *edge_set, int64_t edge_set_bytes, const int64_t *start, int64_t n,
                             int64_t walk_length, float p, float q, const tg_rng *rng, int64_t *walks, void *stream);

/* ---- Node2Vec skip-gram batches: walks, context windows and negatives of G mini-batches in one launch -------------------
 * What the reference's examples/random_walk.py composes per mini-batch (random_walk, PyG's strided slices + cat,
 * randint), fused: a walker's row never leaves LDS as a [n, L] tensor, only its windows are written.
 * A launch samples n_batches = G mini-batches of batch_size = B seeds (seeds: device int64 [G, B], ids < csr->n_major).
 * T = walk_length steps give rows of L = T + 1 columns (as tg_random_walk), C = context_size (1 <= C <= L) gives
 * nw = L - C + 1 windows, R = walks_per_node >= 1, K = num_negative_samples >= 0; p, q and the optional edge set are
 * tg_random_walk_es's.  Mini-batch g draws with call id rng->call_id + g.
 *  positives  W = R * B walkers per mini-batch; walker w = r * B + i starts at seeds[g][i] (PyG's batch.repeat(R)).
 *             walk_g[w][0..L) equals, value for value, tg_random_walk(start = seeds[g] repeated R times, n = W, T, p, q,
 *             edge set, seed, call id + g): the draw of step l, attempt a is (call key of TAG_RW, id = w, d0 = l, d1 = a).
 *             pos_rw[g] is [nw * W, C]: row j * W + w, column c holds walk_g[w][j + c] -- PyG's
 *             cat([rw[:, j:j + C] for j in range(nw)], 0).  A walker that meets a dead end keeps the reference's -1
 *             padding, and so do its windows: a consumer masks with (pos_rw >= 0).all(1).
 *  negatives  U = R * K * B walkers per mini-batch; x_u[0] = seeds[g][u mod B], and for m >= 1
 *             x_u[m] = floor(a * n_nodes / 2^64), a = the low 64 bits of the draw (call key of (seed, call id + g,
 *             TAG_RW_NEG = 12), id = u, d0 = m, d1 = 0).  neg_rw[g] is [nw * U, C]: row j * U + u, column c holds
 *             x_u[j + c].  K = 0: an empty [0, C] slab, neg_rw may be NULL.
 * The slabs of a launch are batch-major and contiguous: pos_rw [G, nw * W, C], neg_rw [G, nw * U, C] (device int64),
 * every word of them is written, nothing is counted and nothing is read back; the call does not synchronise.
 * `form`: 0 auto; 1, 2 the LDS form -- one lane per walker (walkers of a launch flat, t = g * W + w), a wavefront stages
 * its 64 walkers' whole rows in LDS (1: as uint32 with 0xffffffff for -1, needs id_bound = max(csr->n_major, n_nodes) <
 * 2^32 - 1; 2: as int64) at an odd pitch and then streams every window out, 64 * C * 8 contiguous bytes per window inside
 * a mini-batch; the negatives go through the same routine.  A workgroup is one wavefront with 64 * (L | 1) * word + 512
 * bytes of LDS, taken while that is <= 40 KiB, so that a CU always keeps a wavefront per SIMD resident: L <= 157 for
 * form 1, L <= 79 for form 2.  3 the flat form, any L: a walk kernel writes [G * W, L] int64 into `workspace`
 * (tg_rw_skipgram_workspace_bytes), a second kernel streams the windows out of it, a third makes the negatives
 * element-wise.  Auto takes 1, else 2, else 3, whichever fits first.  All forms write identical outputs.
 * Bad arguments (a null buffer, C < 1, C > L, R < 1, K < 0, T < 1, n_nodes < 1 with K > 0, p or q <= 0, a forced form
 * that does not fit, a short workspace) are refused with TG_ERR_INVALID before anything is launched; G = 0 or B = 0
 * returns TG_OK and launches nothing. */
typedef struct {
    int64_t walk_length;          /* T */
    int64_t context_size;         /* C */
    int64_t walks_per_node;       /* R */
    int64_t num_negative_samples; /* K */
    int64_t n_nodes;              /* range of the negative draws */
    float p, q;
} tg_rw_skipgram_config;

typedef struct {
    int64_t *pos_rw; /* [G, nw * W, C] */
    int64_t *neg_rw; /* [G, nw * U, C], or NULL when K = 0 */
} tg_rw_skipgram_out;

/* rows of pos_rw and neg_rw per mini-batch: nw * R * B and nw * R * K * B */
TG_API int tg_rw_skipgram_capacity(const tg_rw_skipgram_config *cfg, int64_t batch_size, int64_t *pos_rows,
                                   int64_t *neg_rows);
/* Which form an auto call takes for ids in [0, id_bound): *form = 1, 2 or 3; *lds_bytes = the LDS a workgroup of the
 * narrowest LDS form the ids allow asks for.  lds_limit_bytes > 0 replaces the 40 KiB limit.  No device is touched. */
TG_API int tg_rw_skipgram_form(const tg_rw_skipgram_config *cfg, int64_t id_bound, int64_t lds_limit_bytes, int32_t *form,
                               int64_t *lds_bytes);
/* the workspace a call of this form needs (form 0: the form auto takes): 0 for the LDS forms, G * W * L * 8 for flat */
TG_API int tg_rw_skipgram_workspace_bytes(const tg_rw_skipgram_config *cfg, int64_t n_batches, int64_t batch_size,
                                          int64_t id_bound, int32_t form, int64_t *bytes);
TG_API int tg_rw_skipgram(const tg_graph *csr, const void *edge_set, int64_t edge_set_bytes, const int64_t *seeds,
                          int64_t n_batches, int64_t batch_size, const tg_rw_skipgram_config *cfg, const tg_rng *rng,
                          const tg_rw_skipgram_out *out, void *workspace, int64_t workspace_bytes, int32_t form,
                          void *stream);

/* ---- MetaPath2Vec skip-gram batches: tg_rw_skipgram along a metapath of a typed graph ---------------------------------------
 * What PyG's MetaPath2Vec composes per mini-batch (a sample per step over the step's relation, the offset of the column's
 * node type into ONE embedding table, dummy_idx for ended walks, strided slices + cat, randint per column type), as one
 * launch for G mini-batches.  The metapath has M = n_steps relations; step l of a walk goes over metapath[l mod M], so a
 * walk longer than M repeats the path, which must then close (step_dst[M - 1] == step_src[0]).  G, B, T, C, R, K, L, nw, W,
 * U, the slabs (tg_rw_skipgram_out: pos_rw [G, nw * W, C], neg_rw [G, nw * U, C], batch-major, every word written, nothing
 * read back, no synchronisation), the window rule (pos_rw[g] row j * W + w, column c = walk_g[w][j + c]; neg_rw[g] row
 * j * U + u, column c = x_u[j + c]) and walker w = r * B + i starting at seeds[g][i] are tg_rw_skipgram's.  seeds: device
 * int64 [G, B], LOCAL ids of type step_src[0].  context_size = L yields the raw walks.
 *  column types  column 0 has type step_src[0], column l + 1 has type step_dst[l mod M].
 *  positives     step l stands at local id cur of type step_src[l mod M] and reads row [b, e) = ptrs[cur], ptrs[cur + 1] of
 *                graphs[l mod M].  e <= b: the walk is over, this column and all later ones are pad_value.  Otherwise the
 *                draw is (call key of (seed, call id + g, TAG_RW), id = w, d0 = l, d1 = 0) and, a = its low 64 bits, the
 *                next local id is indices[b + floor(a * (e - b) / 2^64)]: tg_random_walk's step with p = q = 1 on the
 *                step's own CSR.
 *  negatives     x_u[0] = seeds[g][u mod B]; for m >= 1 x_u[m] = floor(a * type_count[type of column m] / 2^64), a = the
 *                low 64 bits of the draw (call key of (seed, call id + g, TAG_RW_NEG = 12), id = u, d0 = m, d1 = 0).
 *  output word   local id + type_start[type of its column], added in 64 bits: global ids may pass 2^32 while local ids do
 *                not.  type_start = NULL: local ids.
 * The two tags are tg_rw_skipgram's on purpose: with M = 1, one node type, type_start = NULL and pad_value = -1 both slabs
 * equal tg_rw_skipgram(p = q = 1, n_nodes = type_count[0]) bit for bit.
 * `form` as tg_rw_skipgram: 1, 2 stage a wavefront's 64 rows in LDS as LOCAL ids (1: uint32 with 0xffffffff for an ended
 * walk, needs max(type_count) < 2^32 - 1; 2: int64) and add the start / put in pad_value when a word is emitted, from a
 * per-column table of L int64 in LDS; a workgroup is one wavefront with TG_MP_SKIPGRAM_LDS_BYTES(L, word) bytes of LDS,
 * taken while that is <= 40 KiB: L <= 153 for form 1, L <= 77 for form 2.  3 the flat form, any L: finished words go
 * through `workspace` [G * W, L] int64.  Auto takes 1, else 2, else 3, whichever fits first.  All forms write identical words.
 * Refused with TG_ERR_INVALID before anything is launched, with the step named: a null config, graphs, step arrays,
 * type_count or rng; M outside [1, TG_MP_MAX_STEPS]; a type index outside [0, n_types); step_dst[m] != step_src[m + 1] (a
 * broken chain); walk_length > M on an open path; graphs[m].n_major != type_count[step_src[m]]; a type_count < 1;
 * tg_rw_skipgram's own checks (C, R, K, T, a forced form that does not fit, a short workspace, null buffers, sizes whose
 * products overflow).  G = 0 or B = 0 returns TG_OK and launches nothing.  seeds < type_count[step_src[0]] and
 * indices < type_count[step_dst[m]] are the caller's contract. */
#define TG_MP_MAX_STEPS 16
/* LDS of one workgroup of the LDS forms: 64 rows at the odd pitch L | 1, the 64 per-walker offsets, the L column starts */
#define TG_MP_SKIPGRAM_LDS_BYTES(L, word_bytes) (64 * ((L) | 1) * (int64_t)(word_bytes) + 512 + 8 * (int64_t)(L))
typedef struct {
    int32_t n_types, n_steps;      /* n_steps = M = len(metapath), 1 <= M <= TG_MP_MAX_STEPS */
    const tg_graph *graphs;        /* host [M]: CSR of metapath[m] (rows = source type, indices = ids of the dest type);
                                      the same relation may appear at several steps; ptrs32 / indices32 optional */
    const int32_t *step_src;       /* host [M] node-type index */
    const int32_t *step_dst;       /* host [M] */
    const int64_t *type_count;     /* host [n_types] nodes per type */
    const int64_t *type_start;     /* host [n_types] added to every id of that type on output (PyG: start of the type in
                                      the one embedding table); NULL = all zero = local ids */
    int64_t walk_length, context_size, walks_per_node, num_negative_samples;   /* T, C, R, K as tg_rw_skipgram */
    int64_t pad_value;             /* written for every column after a walk ended: -1, or PyG's dummy_idx */
} tg_mp_skipgram_config;

/* rows of pos_rw and neg_rw per mini-batch: nw * R * B and nw * R * K * B */
TG_API int tg_mp_skipgram_capacity(const tg_mp_skipgram_config *cfg, int64_t batch_size, int64_t *pos_rows,
                                   int64_t *neg_rows);
/* Which form an auto call takes: *form = 1, 2 or 3; *lds_bytes = TG_MP_SKIPGRAM_LDS_BYTES of the narrowest LDS form that
 * max(type_count) allows.  lds_limit_bytes > 0 replaces the 40 KiB limit.  No device is touched. */
TG_API int tg_mp_skipgram_form(const tg_mp_skipgram_config *cfg, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes);
/* the workspace a call of this form needs (form 0: the form auto takes): 0 for the LDS forms, G * W * L * 8 for flat */
TG_API int tg_mp_skipgram_workspace_bytes(const tg_mp_skipgram_config *cfg, int64_t n_batches, int64_t batch_size,
                                          int32_t form, int64_t *bytes);
TG_API int tg_mp_skipgram(const tg_mp_skipgram_config *cfg, const int64_t *seeds, int64_t n_batches, int64_t batch_size,
                          const tg_rng *rng, const tg_rw_skipgram_out *out, void *workspace, int64_t workspace_bytes,
                          int32_t form, void *stream);

/* ---- Temporal (CTDNE) skip-gram batches: tg_tempo_random_walk's walks as context windows, with their timestamps -----------
 * What a temporal skip-gram trainer composes per mini-batch (tempo_random_walk, strided slices + cat for the nodes and for
 * the timestamps, randint, slices + cat), fused as tg_rw_skipgram fuses Node2Vec's: a walker's [node | ts] row never leaves
 * LDS as [n, L] tensors, only its windows are written.  A launch samples n_batches = G mini-batches of batch_size = B seeds
 * (seeds, seeds_ts: device int64 [G, B]; ids < csr->n_major; a start time of -1 admits every edge).  csr, node_ts [n_major],
 * edge_ts [n_edges, CSR order], win0, win1 are tg_tempo_random_walk's.  L = walk_length counts COLUMNS of a row, as
 * tg_tempo_random_walk (column 0 is the start; tg_rw_skipgram's T counts steps, L = T + 1); C = context_size (1 <= C <= L)
 * gives nw = L - C + 1 windows, R = walks_per_node >= 1, K = num_negative_samples >= 0.  W = R * B, U = R * K * B.
 * Mini-batch g draws with call id rng->call_id + g.
 *  positives  walker w = r * B + i starts at seeds[g][i] with start time seeds_ts[g][i].  walk_g[w][0..L) and
 *             walk_ts_g[w][0..L) equal, value for value, tg_tempo_random_walk(start = seeds[g] repeated R times, start_ts
 *             likewise, n = W, L, window, seed, call id + g): the draws of step l are addressed (call key of TAG_RW_TEMPO,
 *             id = w * L + l), the chunked one-slot reservoir and the restart draw are that operator's.
 *             pos_rw[g] is [nw * W, C]: row j * W + w, column c holds walk_g[w][j + c]; pos_ts[g] holds walk_ts_g[w][j + c]
 *             at the same place.  A temporal walk never ends (it restarts), so there is no padding; a timestamp may be -1.
 *  negatives  tg_rw_skipgram's rule exactly (TAG_RW_NEG = 12, id = u, d0 = m, floor(a * n_nodes / 2^64); x_u[0] =
 *             seeds[g][u mod B]): neg_rw equals, bit for bit, the neg_rw of tg_rw_skipgram with T = L - 1 for the same
 *             seeds, R, K, n_nodes, seed and call id.  K = 0: an empty slab, neg_rw may be NULL.
 * The slabs are batch-major and contiguous: pos_rw, pos_ts [G, nw * W, C], neg_rw [G, nw * U, C] (device int64); every word
 * of them is written and nothing else, nothing is read back, the call does not synchronise.  pos_ts = NULL: the timestamps
 * are not wanted and not written.
 * One wavefront walks one walker at a time (every step inspects a whole row).  A workgroup is one wavefront that owns
 * walkers_per_workgroup consecutive walkers of the launch (flat t = g * W + w) and takes them in turn; their rows stay in
 * LDS: per walker one 8-byte slab offset and a row of (2 L | 1) int64 (L nodes, L timestamps, odd pitch),
 * TG_TEMPO_SKIPGRAM_LDS_BYTES(L, walkers) in all.  Then it streams the windows out; inside a mini-batch window j of the
 * workgroup's walkers is one run of walkers * C * 8 contiguous bytes per slab, and a run that crosses a mini-batch boundary
 * splits there.  walkers_per_workgroup is 4 while that fits 16 KiB (L <= 255), then 2 (L <= 511), then 1; a single walker
 * may take up to 64 KiB (L <= 4095), beyond that the call returns TG_ERR_UNSUPPORTED, as tg_tempo_random_walk does for a
 * row that does not fit.  The walk bounds the launch, not the stores (tools/bench_temporal_walk_loader.py).  The negatives
 * are a second launch on the same stream.
 * Bad arguments (a null buffer, config or rng, C < 1, C > L, R < 1, K < 0, L < 1, n_nodes < 1 with K > 0, negative sizes or
 * sizes whose products leave tg_rw_skipgram's bounds) are refused with TG_ERR_INVALID before anything is launched; G = 0 or
 * B = 0 returns TG_OK and launches nothing. */
#define TG_TEMPO_SKIPGRAM_LDS_BYTES(L, walkers) ((int64_t)(walkers) * (((2 * (int64_t)(L)) | 1) + 1) * 8)
typedef struct {
    int64_t walk_length;          /* L: COLUMNS of a row, as tg_tempo_random_walk (column 0 is the start; not L + 1) */
    int64_t context_size;         /* C, 1 <= C <= L; nw = L - C + 1 windows */
    int64_t walks_per_node;       /* R >= 1 */
    int64_t num_negative_samples; /* K >= 0 */
    int64_t n_nodes;              /* range of the negative draws */
    int64_t win0, win1;           /* the walk's half-open window relative to the start time, as tg_tempo_random_walk */
} tg_tempo_skipgram_config;

typedef struct {
    int64_t *pos_rw; /* [G, nw * W, C] nodes */
    int64_t *pos_ts; /* [G, nw * W, C] timestamps of the same words, or NULL: not wanted, not written */
    int64_t *neg_rw; /* [G, nw * U, C], or NULL when K = 0 */
} tg_tempo_skipgram_out;

/* rows of pos_rw (and pos_ts) and of neg_rw per mini-batch: nw * R * B and nw * R * K * B */
TG_API int tg_tempo_skipgram_capacity(const tg_tempo_skipgram_config *cfg, int64_t batch_size, int64_t *pos_rows,
                                      int64_t *neg_rows);
/* What a launch will use: *walkers_per_workgroup and *lds_bytes = TG_TEMPO_SKIPGRAM_LDS_BYTES(L, *walkers_per_workgroup);
 * TG_ERR_UNSUPPORTED when one walker's rows do not fit.  No device is touched. */
TG_API int tg_tempo_skipgram_lds_bytes(const tg_tempo_skipgram_config *cfg, int32_t *walkers_per_workgroup, int64_t *lds_bytes);
TG_API int tg_tempo_skipgram(const tg_graph *csr, const int64_t *node_ts, const int64_t *edge_ts, const int64_t *seeds,
                             const int64_t *seeds_ts, int64_t n_batches, int64_t batch_size,
                             const tg_tempo_skipgram_config *cfg, const tg_rng *rng, const tg_tempo_skipgram_out *out,
                             void *stream);

/* ---- Link-level seed rows: positive edges plus checked negatives of G mini-batches in one launch --------------------------
 * What a link-prediction trainer composes per mini-batch (randint negatives, cat with the positives), with the negatives
 * checked against the graph as the reference's negative sampler checks them (negative_sampling.rs: has_edge(v, w) and
 * v == w are rejected) and addressed, so a row depends on (seed, call id) alone.  The rows feed tg_ns_homo_batched.
 * csc: the graph the sampler walks (column = target), optionally with ptrs32 / indices32.  edge_set: NULL, or the set
 * tg_edge_set_build made over THIS csc (key = column << 32 | row; ids < 2^32 - 1).  edge(s -> d) means: s is among
 * indices[ptrs[d] .. ptrs[d + 1]) -- a binary search of column d, or one probe of the set.
 * src, dst: device int64 [G, E], the positive edges of n_batches = G mini-batches of n_edges = E each.  K = n_neg >= 0
 * negatives per positive, try_count >= 1, n_nodes = csc->n_major.  Mini-batch g draws with call id rng->call_id + g:
 * attempt a of negative u is the draw (call key of (seed, call id + g, TAG_LINK_NEG = 13), id = u, d0 = a, d1 = 0); a
 * candidate is floor(half * n_nodes / 2^64) of a 64-bit half of it (words 0,1 / words 2,3).
 *  TG_LINK_BINARY   P = E + K * E pairs, S = 2 P.  seeds[g] = [src_pos(E) | src_neg(K E) | dst_pos(E) | dst_neg(K E)], so
 *                   seeds[g] viewed as [2, P] is the global edge_label_index.  Attempt a proposes s_a (words 0,1) and d_a
 *                   (words 2,3); accepted when s_a != d_a and not edge(s_a -> d_a).
 *  TG_LINK_TRIPLET  S = E * (2 + K), P = E + K * E.  seeds[g] = [src(E) | dst_pos(E) | dst_neg(E K)], negative u = i * K + k
 *                   belongs to positive i.  Attempt a proposes d_a (words 0,1); accepted when d_a != src[g][i] and not
 *                   edge(src[g][i] -> d_a).
 * The first accepted attempt a < try_count is kept.  When none is, the candidate of attempt try_count - 1 is kept and
 * unverified[g] counts it (the row's shape is fixed: a slot cannot be dropped as the reference drops it).  try_count = 1
 * makes no look-up: attempt 0 is kept as it is (PyG's unchecked negatives) and unverified[g] = 0.
 * seeds: device int64 [G, S], contiguous; every word is written and nothing else.  unverified: device int64 [G] (written
 * for every g) or NULL.  Nothing is read back; the call does not synchronise.  Bad arguments (a null pointer, a negative
 * size, try_count < 1, an unknown mode, n_nodes < 1 or != csc->n_major, an edge set of another size or with ids >= 2^32 - 1)
 * are refused with TG_ERR_INVALID before anything is launched; G = 0 or E = 0 returns TG_OK and launches nothing. */
#define TG_LINK_BINARY 0
#define TG_LINK_TRIPLET 1
/* *seeds_per_batch = S and *pairs = P of a mini-batch of n_edges positives with n_neg negatives each */
TG_API int tg_link_seeds_capacity(int64_t n_edges, int64_t n_neg, int32_t mode, int64_t *seeds_per_batch, int64_t *pairs);
TG_API int tg_link_seeds(const tg_graph *csc, const void *edge_set, int64_t edge_set_bytes, const int64_t *src,
                         const int64_t *dst, int64_t n_batches, int64_t n_edges, int64_t n_neg, int32_t mode,
                         int32_t try_count, const tg_rng *rng, int64_t n_nodes, int64_t *seeds, int64_t *unverified,
                         void *stream);

/* ---- Typed link-level seed rows: tg_link_seeds for ONE relation (A, rel, B) of a typed graph --------------------------------
 * The positives are edges of the relation: src[G, E] are ids of node type A in [0, n_src), dst[G, E] ids of node type B in
 * [0, n_dst).  G, E, K = n_neg, mode, try_count, unverified and the draw law are tg_link_seeds' (same tag, mini-batch g
 * draws with call id rng->call_id + g, attempt a of negative u is the block (id = u, d0 = a, d1 = 0)), with two ranges:
 *  TG_LINK_BINARY   s_a = floor(words01 * n_src / 2^64), d_a = floor(words23 * n_dst / 2^64)
 *  TG_LINK_TRIPLET  d_a = floor(words01 * n_dst / 2^64), s = the positive's source
 * A candidate is accepted when edge(s -> d) is false (s among indices[ptrs[d] .. ptrs[d + 1]) of rel->csc, or one probe of
 * rel->edge_set) and, ONLY if same_type, s != d.  A deliberate difference from the reference: its heterogeneous negative
 * sampler rejects v == w even across node types (negative_sampling.rs:117); here equal ids of two different types are
 * unrelated nodes and stay eligible.  same_type = 1 says both endpoints are one node type (needs n_src == n_dst).
 * Mini-batch g writes TWO rows, the inputs of the two node types for tg_ns_hetero_batched (P, S of tg_link_seeds_capacity):
 *  source row       src_seeds + g * src_pitch, Ws words: binary Ws = P [src_pos(E) | src_neg(K E)]; triplet Ws = E [src(E)]
 *  destination row  dst_seeds + g * dst_pitch, Wd = P words: [dst_pos(E) | dst_neg(K E)] (triplet: negative i * K + k
 *                   belongs to positive i)
 * Pitches are in words and at least the widths.  Every word inside the widths is written and nothing else: not the words
 * between width and pitch, nothing behind the last row.  The two regions must not overlap, except that their rows may
 * interleave inside one common pitch: src_seeds = base, dst_seeds = base + Ws, both pitches = Ws + Wd = S is tg_link_seeds'
 * row, and with same_type = 1 the output then equals tg_link_seeds' bit for bit (one input row when A == B).
 * Refused with TG_ERR_INVALID before anything is launched: a null rel, rng or graph; n_src < 1 or n_dst < 1; n_dst !=
 * csc->n_major; same_type with n_src != n_dst; a pitch below its width; try_count < 1; an unknown mode; negative sizes or
 * products past tg_link_seeds' bounds; an edge set of another size or with n_src or n_dst >= 2^32 - 1; overlapping
 * regions.  G = 0 or E = 0 returns TG_OK and launches nothing.  src < n_src, dst < n_dst and indices < n_src are the
 * caller's contract.  Nothing is read back; the call does not synchronise. */
typedef struct {
    const tg_graph *csc;      /* the labelled relation's CSC: n_major == n_dst columns, every index < n_src;
                                 ptrs32 / indices32 optional */
    const void *edge_set;     /* NULL, or tg_edge_set_build over THIS csc (key = column << 32 | row) */
    int64_t edge_set_bytes;
    int64_t n_src, n_dst;     /* id ranges of the source and the destination node type */
    int32_t same_type;        /* 1: both endpoints are ONE node type (needs n_src == n_dst); then s == d is rejected */
} tg_link_rel;

TG_API int tg_link_seeds_typed(const tg_link_rel *rel, const int64_t *src, const int64_t *dst, int64_t n_batches,
                               int64_t n_edges, int64_t n_neg, int32_t mode, int32_t try_count, const tg_rng *rng,
                               int64_t *src_seeds, int64_t src_pitch, int64_t *dst_seeds, int64_t dst_pitch,
                               int64_t *unverified, void *stream);

/* tempo_random_walk (random_walk.rs:80-158; binding python.rs:611-642).
 * walks, walks_ts: [n, walk_length] device int64. */
TG_API int tg_tempo_random_walk(const tg_graph *csr, const int64_t *node_ts, const int64_t *edge_ts, const int64_t *start,
                         const int64_t *start_ts, int64_t n, int64_t walk_length, int64_t win0, int64_t win1,
                         const tg_rng *rng, int64_t *walks, int64_t *walks_ts, void *stream);

/* biased_tempo_random_walk (random_walk.rs:160-288; binding python.rs:645-687): time-respecting walk whose next
 * vertex is drawn with BiasType weights (random_walk.rs:165-182) by the one-slot weighted reservoir (f32,
 * utils/sampling.rs:28-55); a walker without candidates restarts from its start vertex, at most retry_count times.
 * walks, walks_ts: [n, walk_length] device int64.  status (device int32, zeroed by the caller): bit 1 = the reference
 * would have panicked (empty float range, sampling.rs:49), bit 0 = a row longer than `max_degree` met the linear
 * bias.  `max_degree` (largest CSR row) sizes the sort slab the linear bias needs for rows above 1024 edges:
 * workspace = tg_biased_walk_workspace_bytes(n, max_degree, bias), 0 for the other biases. */
#define TG_BIAS_UNIFORM 0
#define TG_BIAS_LINEAR 1
#define TG_BIAS_EXPONENTIAL 2
TG_API int tg_biased_walk_workspace_bytes(int64_t n, int64_t max_degree, int32_t bias, int64_t *bytes);
TG_API int tg_biased_tempo_random_walk(const tg_graph *csr, const int64_t *node_ts, const int64_t *edge_ts,
                                       const int64_t *start, const int64_t *start_ts, int64_t n, int64_t walk_length,
                                       int32_t bias, int32_t forward, int64_t retry_count, int64_t max_degree,
                                       const tg_rng *rng, int64_t *walks, int64_t *walks_ts, int32_t *status,
                                       void *workspace, int64_t workspace_bytes, void *stream);

/* negative_sample_neighbors_homogenous / _heterogenous (src/algo/negative_sampling.rs:6-131; bindings
 * python.rs:690-783) as one problem description.  Host arrays are indexed by node type (order of the caller's
 * `node_types`) and relation (order of `edge_types`); the reference's HashMap visiting order is replaced by
 * those orders. */
typedef struct {
    int32_t n_types, n_rels;
    int32_t homogeneous; /* 1: the homogeneous operator (no relation draw; n_types = n_rels = 1) */
    int32_t inbound;     /* negative_sampling.rs:112-115 */
    const int32_t *rel_src;       /* host [n_rels] node-type index of the relation's source */
    const int32_t *rel_dst;       /* host [n_rels] */
    const tg_graph *graphs;       /* host [n_rels] CSR views (device pointers inside) */
    const int64_t *node_count;    /* host [n_rels]: graph_size.1 / sizes[rel].1 (negative_sampling.rs:28,105) */
    const int64_t *const *inputs; /* host [n_types] device pointers */
    const int64_t *n_inputs;      /* host [n_types]; < 0: the type has no entry in `inputs` */
    int64_t num_neg, try_count;
} tg_neg_problem;

typedef struct {
    int64_t *const *samples; /* host [n_types] device buffers, capacity max(n_inputs[t],0) + total items */
    int64_t *const *rows;    /* host [n_rels] device buffers, capacity n_inputs[src] * num_neg */
    int64_t *const *cols;    /* host [n_rels] */
    int64_t *n_samples;      /* device [n_types] */
    int64_t *n_edges;        /* device [n_rels] */
    int32_t *panic;          /* device [1]: 1 where the reference would panic (inbound row out of range) */
} tg_neg_out;

TG_API int tg_neg_workspace_bytes(const tg_neg_problem *problem, int64_t *bytes);
TG_API int tg_neg_sample(const tg_neg_problem *problem, const tg_rng *rng, const tg_neg_out *out, void *workspace,
                         void *stream);

/* Batched negative sampling: n_calls independent calls of one problem shape in ONE launch.  The calls share the graphs,
 * n_inputs, num_neg and try_count; problem->inputs[t] points at an [n_calls, n_inputs[t]] row-major slab.  Call b draws
 * with call id rng->call_id + b and equals tg_neg_sample run alone with that call id, word for word.
 *  - form: where a call's state (32-bit candidates, local ids, one hash table over inputs and new nodes) fits the LDS of
 *    a workgroup, ONE workgroup runs ONE whole call and only the CSR look-ups and the output stores touch global memory
 *    (form 1, "fused").  Otherwise (too many items or inputs, node counts or CSR rows of 2^32 and more, more than 16 node
 *    types, a device with less LDS) the same entry point runs tg_neg_sample's kernels call by call on the caller's
 *    stream (form 0): same outputs, tg_neg_sample's speed.  tg_neg_batched_form tells which: lds_limit_bytes > 0 is taken
 *    as the workgroup's LDS limit and no device is touched, <= 0 asks the current device (what tg_neg_sample_batched
 *    does); *lds_bytes = what the fused kernel asks for (0 where 32-bit ids do not do).
 *  - inputs must be valid node ids of their type (>= 0, below the row count of every relation that leaves the type), as for
 *    tg_neg_sample; the fused form keeps ids in 32 bits, so ids outside [0, 2^32) would be merged there (the host
 *    surfaces check the range before they launch).
 *  - outputs: row b of every slab is call b's; only its first counts[b][...] words are written.  counts[b] holds the node
 *    counts of the types, then the edge counts of the relations.  panic[b] = 1 where the reference would panic in call b
 *    (inbound row out of range, negative_sampling.rs:113); that call's rows are then unspecified, every other call is
 *    unaffected.
 *  - capacities (tg_neg_batched_capacity), per call: tg_neg_out's, max(n_inputs[t], 0) + total items for a type,
 *    n_inputs[src] * num_neg for a relation.  Pitches must be at least these.
 *  - workspace: none for the fused form (0 bytes, the pointer may be NULL), tg_neg_workspace_bytes for the other (the
 *    calls run one after the other in it); 8-byte aligned.  1 <= n_calls <= TG_NEG_MAX_CALLS.
 *  - bad arguments (null, n_calls, more than 32 relations, negative counts, a type with inputs and no outgoing
 *    relation, short pitches, short workspace) are refused with TG_ERR_INVALID before anything is launched.  Nothing
 *    synchronises. */
#define TG_NEG_MAX_CALLS 65535
typedef struct {
    int64_t *const *samples;    /* host [n_types] device slabs [n_calls, pitch_nodes[t]] */
    const int64_t *pitch_nodes; /* host [n_types], >= tg_neg_batched_capacity()'s cap_nodes */
    int64_t *const *rows;       /* host [n_rels] device slabs [n_calls, pitch_edges[r]] */
    int64_t *const *cols;
    const int64_t *pitch_edges; /* host [n_rels], >= tg_neg_batched_capacity()'s cap_edges */
    int64_t *counts;            /* device [n_calls, n_types + n_rels] */
    int32_t *panic;             /* device [n_calls] */
} tg_neg_batched_out;

TG_API int tg_neg_batched_capacity(const tg_neg_problem *problem, int64_t *cap_nodes, int64_t *cap_edges);
TG_API int tg_neg_batched_form(const tg_neg_problem *problem, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes);
TG_API int tg_neg_batched_workspace_bytes(const tg_neg_problem *problem, int64_t n_calls, int64_t *bytes);
TG_API int tg_neg_sample_batched(const tg_neg_problem *problem, int64_t n_calls, const tg_rng *rng,
                                 const tg_neg_batched_out *out, void *workspace, int64_t workspace_bytes, void *stream);

/* hgt_sampling (src/algo/hgt_sampling.rs:138-278; binding python.rs:399-482).  Host arrays are indexed by node
 * type (`node_types` order) and relation (`edge_types` order); graphs are CSC, graphs[r].timestamps is the
 * relation's row_timestamps or NULL.  All state lives in the caller's workspace; nothing synchronises. */
typedef struct {
    int32_t n_types, n_rels, n_hops;
    int32_t has_timerange;          /* timerange = [tr_lo, tr_hi) (python.rs:450) */
    const int32_t *rel_src;         /* host [n_rels] */
    const int32_t *rel_dst;         /* host [n_rels] */
    const tg_graph *graphs;         /* host [n_rels] */
    const int64_t *const *inputs;   /* host [n_types] device pointers (NULL when absent) */
    const int64_t *const *input_ts; /* host [n_types] device pointers, or NULL: no input timestamps */
    const int64_t *n_inputs;        /* host [n_types]; < 0: the type has no entry in `inputs` */
    const int64_t *num_samples;     /* host [n_types * n_hops]; < 0: the type has no entry in `num_samples` */
    int64_t tr_lo, tr_hi;
} tg_hgt_problem;

typedef struct {
    int64_t *const *samples;    /* host [n_types] device buffers, capacity max(n_inputs,0) + sum of num_samples */
    int64_t *const *sample_ts;  /* host [n_types], same capacity */
    int64_t *const *rows;       /* host [n_rels] device buffers, capacity 50 * capacity(samples[dst]) */
    int64_t *const *cols;       /* host [n_rels] */
    int64_t *const *edge_index; /* host [n_rels] */
    int64_t *n_samples;         /* device [n_types] */
    int64_t *n_edges;           /* device [n_rels] */
    int32_t *panic;             /* device [1]: 1 where the reference would panic */
} tg_hgt_out;

TG_API int tg_hgt_workspace_bytes(const tg_hgt_problem *problem, int64_t *bytes);
TG_API int tg_hgt_sample(const tg_hgt_problem *problem, const tg_rng *rng, const tg_hgt_out *out, void *workspace,
                         int64_t workspace_bytes, void *stream);

/* Batched hgt_sampling: n_calls independent calls of one problem shape in ONE launch chain (the call is the third grid
 * dimension of every launch, so the chain is as long as a single call's).  The calls share the graphs, n_inputs,
 * num_samples and the time range; problem->inputs[t] / input_ts[t] point at [n_calls, n_inputs[t]] row-major slabs.
 * Call b draws with call id rng->call_id + b and equals tg_hgt_sample run alone with that call id, word for word.
 *  - outputs: row b of every slab is call b's; only its first counts[b][...] words are written.  counts[b] holds the
 *    node counts of the types, then the edge counts of the relations, then call b's panic flag (1 where the reference
 *    would panic; the other calls are unaffected).
 *  - workspace: n_calls regions at a fixed stride, nothing shared: tg_hgt_batched_workspace_bytes(p, n) =
 *    n * tg_hgt_batched_workspace_bytes(p, 1); 8-byte aligned.  1 <= n_calls <= TG_HGT_MAX_CALLS (grid z).
 *  - scan limit: every scan runs in one workgroup per call, so shapes past the single call's one-workgroup limit
 *    (TG_HGT_ONE_WORKGROUP_SCAN chunks of 64 contributions in a layer or of 64 budget entries, or
 *    TG_HGT_ONE_WORKGROUP_SCAN nodes in a type that a relation points into) are refused with TG_ERR_INVALID by all
 *    three functions below; tg_hgt_sample takes such shapes one call at a time. */
#define TG_HGT_MAX_CALLS 65535
#define TG_HGT_ONE_WORKGROUP_SCAN 16384
typedef struct {
    int64_t *const *samples;    /* host [n_types] device slabs [n_calls, cap_nodes[t]] */
    int64_t *const *sample_ts;  /* host [n_types], same shape */
    const int64_t *cap_nodes;   /* host [n_types] row pitches, >= tg_hgt_batched_capacity()'s cap_nodes */
    int64_t *const *rows;       /* host [n_rels] device slabs [n_calls, cap_edges[r]] */
    int64_t *const *cols;       /* host [n_rels] */
    int64_t *const *edge_index; /* host [n_rels] */
    const int64_t *cap_edges;   /* host [n_rels] row pitches, >= tg_hgt_batched_capacity()'s cap_edges */
    int64_t *counts;            /* device [n_calls, n_types + n_rels + 1] */
} tg_hgt_batched_out;

/* per call: cap_nodes[t] = max(n_inputs[t], 0) + the type's num_samples; cap_edges[r] = 50 * max(cap_nodes[dst], 1) */
TG_API int tg_hgt_batched_capacity(const tg_hgt_problem *problem, int64_t *cap_nodes, int64_t *cap_edges);
TG_API int tg_hgt_batched_workspace_bytes(const tg_hgt_problem *problem, int64_t n_calls, int64_t *bytes);
TG_API int tg_hgt_sample_batched(const tg_hgt_problem *problem, int64_t n_calls, const tg_rng *rng,
                                 const tg_hgt_batched_out *out, void *workspace, int64_t workspace_bytes, void *stream);

/* budget_sampling (src/algo/budget_sampling.rs:63-265; binding python.rs:486-581), one (layer, node type) at a
 * time: Budget::update + Budget::sample for every frontier node of the type (SURVEY.md 8(f) "next" row).  The host
 * appends the selected candidates in (node, slot) order.  Selected slot (j, s) lives at [j * fanout + s];
 * sel_rel < 0 marks an empty slot. */
typedef struct {
    const tg_graph *graphs;  /* host [n_rels]: CSC of the relations INTO the node type (timestamps optional) */
    const int32_t *rel_ids;  /* host [n_rels]: their index in the caller's relation list */
    int32_t n_rels;
    int32_t node_type;       /* index of the type being expanded (rng tag) */
    int32_t fanout;          /* num_neighbors[type][layer], <= 64 */
    int32_t filter_on, forward, relative;
    int64_t win_lo, win_hi;  /* half-open window */
    const int64_t *nodes;    /* [n_front] frontier nodes of the type */
    const int64_t *nodes_ts; /* [n_front] */
    int64_t n_front;
    int64_t id_base;         /* slot of nodes[0] in the type's sample list (draw id = id_base + j) */
} tg_budget_layer_in;

typedef struct {
    int64_t *sel_v, *sel_ts, *sel_rel, *sel_i; /* each [n_front * fanout] */
} tg_budget_layer_out;

TG_API int tg_budget_layer(const tg_budget_layer_in *in, const tg_rng *rng, const tg_budget_layer_out *out, void *stream);

/* budget_sampling as ONE stream-ordered call without host bookkeeping: sample lists, their lengths and the frontier
 * bounds live on the device (workspace); per (layer, node type) step the per-node selection is followed by a stable
 * multi-way partition that appends every chosen candidate to its source type's list and its relation's edge lists in
 * (node, slot) order (budget_sampling.rs:223-257).  Node types / relations are indexed in the caller's order.
 * Up to 8 node types, 16 relations, num_neighbors <= 64 (tg_budget_layer is the per-step form without these
 * limits on types / relations).  counts [n_types + n_rels] = list lengths.  Quirk kept: edge_index holds the
 * neighbour's index inside its column (budget_sampling.rs:116). */
typedef struct {
    int32_t n_types, n_rels, n_hops;
    int32_t filter_on, forward, relative;
    int64_t win_lo, win_hi;          /* half-open window (python.rs:541-548) */
    const int32_t *rel_src, *rel_dst; /* host [n_rels] */
    const tg_graph *graphs;           /* host [n_rels] CSC, timestamps optional */
    const int64_t *num_neighbors;     /* host [n_types * n_hops] */
    const int64_t *const *inputs;     /* host [n_types] device pointers (NULL where n_inputs[t] == 0) */
    const int64_t *const *input_ts;   /* host [n_types] device pointers or NULL (timestamp -1) */
    const int64_t *n_inputs;          /* host [n_types] */
} tg_budget_problem;

typedef struct {
    int64_t *const *samples;    /* [n_types] device slabs [cap_nodes[t]] */
    int64_t *const *sample_ts;
    const int64_t *cap_nodes;
    int64_t *const *rows;       /* [n_rels] device slabs [cap_edges[r]] */
    int64_t *const *cols;
    int64_t *const *edge_index;
    const int64_t *cap_edges;
    int64_t *counts;            /* device [n_types + n_rels] */
} tg_budget_out;

TG_API int tg_budget_capacity(const tg_budget_problem *problem, int64_t *cap_nodes, int64_t *cap_edges);
TG_API int tg_budget_workspace_bytes(const tg_budget_problem *problem, int64_t *bytes);
TG_API int tg_budget_sample(const tg_budget_problem *problem, const tg_rng *rng, const tg_budget_out *out, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* Batched budget_sampling: n_calls independent calls of one problem shape in ONE launch chain (the call is the third grid
 * dimension of every launch, so the chain is as long as a single call's).  The calls share the graphs, n_inputs,
 * num_neighbors and the temporal filter; problem->inputs[t] / input_ts[t] point at [n_calls, n_inputs[t]] row-major slabs.
 * Call b draws with call id rng->call_id + b and equals tg_budget_sample run alone with that call id, word for word.
 *  - outputs: row b of every slab is call b's; only its first counts[b][...] words are written.  counts[b] holds the
 *    node counts of the types, then the edge counts of the relations (budget sampling never panics on the device).
 *  - capacities: tg_budget_capacity's, per call.
 *  - workspace: n_calls regions at a fixed stride, nothing shared: tg_budget_batched_workspace_bytes(p, n) =
 *    n * tg_budget_batched_workspace_bytes(p, 1) (= n * tg_budget_workspace_bytes(p)); 8-byte aligned.
 *    1 <= n_calls <= TG_BUDGET_MAX_CALLS (grid z).
 *  - limits: tg_budget_sample's (<= 8 node types, <= 16 relations, num_neighbors <= 64).  Shapes past them and bad
 *    arguments are refused with TG_ERR_INVALID before anything is launched. */
#define TG_BUDGET_MAX_CALLS 65535
typedef struct {
    int64_t *const *samples, *const *sample_ts;             /* host [n_types] device slabs [n_calls, pitch_nodes[t]] */
    const int64_t *pitch_nodes;                             /* host [n_types], >= tg_budget_capacity()'s cap_nodes */
    int64_t *const *rows, *const *cols, *const *edge_index; /* host [n_rels] device slabs [n_calls, pitch_edges[r]] */
    const int64_t *pitch_edges;                             /* host [n_rels], >= tg_budget_capacity()'s cap_edges */
    int64_t *counts;                                        /* device [n_calls, n_types + n_rels] */
} tg_budget_batched_out;

TG_API int tg_budget_batched_workspace_bytes(const tg_budget_problem *problem, int64_t n_calls, int64_t *bytes);
TG_API int tg_budget_sample_batched(const tg_budget_problem *problem, int64_t n_calls, const tg_rng *rng,
                                    const tg_budget_batched_out *out, void *workspace, int64_t workspace_bytes,
                                    void *stream);

/* ---- synthetic inputs of the measurement harness ---- */

/* R-MAT edge list: n_edges edges over 2^scale vertices, (a,b,c,d) =
 * (0.57,0.19,0.19,0.05), one Philox word per bit; duplicates and self loops
 * kept.  row, col: [n_edges] device int64. */
TG_API int tg_rmat_edges(int32_t scale, int64_t n_edges, uint64_t seed, int64_t *row, int64_t *col, void *stream);
/* rectangular form for bipartite relations: 2^row_scale x 2^col_scale, row / column bits drawn to their own depths */
TG_API int tg_rmat_edges_rect(int32_t row_scale, int32_t col_scale, int64_t n_edges, uint64_t seed, int64_t *row,
                              int64_t *col, void *stream);

/* Seed batches: out[b*n_seeds + i] = Philox(seed; first_batch + b, i) mod n_nodes. */
TG_API int tg_seed_batches(uint64_t seed, int64_t first_batch, int64_t n_batches, int64_t n_seeds, int64_t n_nodes,
                    int64_t *out, void *stream);

/* to_csc / to_csr (src/data/storage.rs:103-126; bindings python.rs:27-53): COO (row, col) of a size0 x size1 graph
 * -> ptrs [size1 + 1 | size0 + 1], indices [nnz], perm [nnz] (stable sort by the reference's key
 * col*size0+row | row*size1+col).  Negative ids are not checked. */
TG_API int tg_coo_to_csx_workspace_bytes(int64_t nnz, int64_t size0, int64_t size1, int64_t *bytes);
TG_API int tg_coo_to_csx(const int64_t *row, const int64_t *col, int64_t nnz, int64_t size0, int64_t size1, int32_t csc,
                         int64_t *ptrs, int64_t *indices, int64_t *perm, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* Input validation for hosts: sets flag[0] |= 1 (device int32, zeroed by the caller) when any of values[0..n) lies
 * outside [lo, hi).  The samplers index `ptrs` with their inputs and do NOT check them (the reference panics on an
 * out-of-range node id; a device kernel would fault). */
TG_API int tg_check_range(const int64_t *values, int64_t n, int64_t lo, int64_t hi, int32_t *flag, void *stream);
/* The same check without a read-back before the sampler runs: out[i] = values[i] if it lies in [lo, hi) else lo (a valid
 * id, so the sampler cannot fault), flag[0] |= 1 (device int64 word, zeroed by the caller -- e.g. the last word of the
 * array the host reads back anyway when the call ends) if any did not.  The host raises after that one read-back. */
TG_API int tg_sanitize_range(const int64_t *values, int64_t n, int64_t lo, int64_t hi, int64_t *out, int64_t *flag,
                             void *stream);

/* ind2ptr (src/data/storage.rs:67-101) on the device: sorted `ind` [numel] -> out [m+1]. */
TG_API int tg_ind2ptr(const int64_t *ind, int64_t numel, int64_t m, int64_t *out, void *stream);

/* Mini-batch materialisation, the step AFTER the path: dst[i, :] = src[index[i], :] for
 * i < n, rows of `row_bytes` bytes, source rows `src_stride_bytes` apart (>= row_bytes), dst rows packed.  This is the
 * `x[samples]` / `edge_attr[perm[edge_index]]` gather the reference's examples leave to PyG's filter_data
 * (examples/neighbor_sampling.py:24,36,48; examples/neighbor_sampling_typed.py:27).  dtype-agnostic (bytes); uses
 * 16-byte vectors when pointers, stride and row length are 16-byte multiples.  An index outside [0, n_src_rows)
 * writes a zero row and sets status[0] |= 1 (device int32, zeroed by the caller; may be NULL). */
TG_API int tg_gather_rows(const void *src, int64_t n_src_rows, int64_t row_bytes, int64_t src_stride_bytes,
                          const int64_t *index, int64_t n, void *dst, int32_t *status, void *stream);

/* Per-batch slabs of tg_ns_homo_batched -> flat batch-major arrays: batch b's samples to flat_samples[node_off[b] ..],
 * its rows / cols / edge pointers to flat_*[edge_off[b] ..] (offsets: device arrays, exclusive prefixes of the batch
 * counts).  What a loader hands on to tg_gather_rows (tch_geometric/loader.py). */
TG_API int tg_ns_homo_compact(const tg_ns_out *out, int64_t n_batches, const int64_t *node_off, const int64_t *edge_off,
                              int64_t *flat_samples, int64_t *flat_rows, int64_t *flat_cols, int64_t *flat_edge_index,
                              void *stream);

/* ---- per-batch node dedup and relabel of the tg_ns_homo_batched slabs ------------------------------------------------
 * The sampler returns a forest: a vertex reached along two paths has two slots in `samples`.  This operator makes, for
 * every batch b independently (n = counts[b][0] nodes, m = counts[b][1] edges), what a PyG-style consumer expects:
 *   nodes[b]        the distinct values of samples[b][:n], ordered by the position of their FIRST occurrence (distinct
 *                   seeds therefore stay first, in order)
 *   inverse[b][p]   index in nodes[b] of samples[b][p], p < n: nodes[inverse] == samples          (may be NULL)
 *   rows[b][e], cols[b][e] = inverse[in.rows[b][e]], inverse[in.cols[b][e]], e < m; edges are not merged
 *   counts[b]       {n_unique, m}: the layout of tg_ns_out.counts
 *   layer_nodes[b][h], h < n_hops: unique nodes among the first in.layer_offsets[b][h][0] positions, the node count known
 *                   when hop h starts (h = 0: the unique seeds)                                    (may be NULL)
 * Pitches are in.cap_nodes (nodes, inverse), in.cap_edges (rows, cols), 2 (counts), n_hops (layer_nodes).  Words past
 * n_unique / n / m are not written; in.edge_index is not touched.  out.rows / out.cols may be in.rows / in.cols.  A
 * tg_ns_out with samples = nodes, rows, cols, counts of this struct goes straight into tg_ns_homo_compact.
 * Every id is in [0, id_bound): id_bound <= 2^31 takes 32-bit hash keys, else 64-bit ones.  `form`: 0 auto, 1 one
 * workgroup runs one batch with its table in LDS (where a table of 2^k >= 4/3 cap_nodes slots fits: cap_nodes <= 12 288
 * with 32-bit keys in 160 KiB), 2 a grid over all batches' positions with the per-batch tables in `workspace` (cleared
 * inside the call).  Outputs depend on neither the form nor the workspace size: a workspace of at least bytes_min and
 * less than bytes runs the batches in rounds of as many tables as fit.  Bad arguments are refused with TG_ERR_INVALID
 * before anything is launched; the call does not synchronise and reads nothing back. */
typedef struct {
    int64_t *nodes;
    int64_t *inverse;     /* or NULL */
    int64_t *rows;
    int64_t *cols;
    int64_t *counts;
    int64_t *layer_nodes; /* or NULL */
} tg_ns_unique_out;
/* Which form an auto call takes: *form = 1 (LDS) or 2 (flat); *lds_bytes = the LDS the LDS form asks for.
 * lds_limit_bytes > 0 is taken as the workgroup's LDS limit and no device is touched; <= 0 asks the current device. */
TG_API int tg_ns_homo_unique_form(int64_t cap_nodes, int64_t id_bound, int64_t lds_limit_bytes, int32_t *form,
                                  int64_t *lds_bytes);
/* *bytes_min = the flat form's workspace of ONE batch, *bytes = what an auto call wants for all n_batches at once:
 * n_batches * bytes_min, or 0 where auto takes the LDS form on the current device. */
TG_API int tg_ns_homo_unique_workspace_bytes(int64_t cap_nodes, int64_t id_bound, int64_t n_batches, int64_t *bytes,
                                             int64_t *bytes_min);
TG_API int tg_ns_homo_unique(const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops, int64_t id_bound,
                             const tg_ns_unique_out *out, void *workspace, int64_t workspace_bytes, int32_t form,
                             void *stream);

/* ---- per-batch, per-GROUP node dedup and relabel: one subgraph per group of seeds (PyG's disjoint=True) ------------------
 * tg_ns_homo_unique with a group dimension.  seed_group (device int32 [n_seeds], shared by all batches; NULL = the
 * identity, and then n_groups must equal n_seeds) puts every seed position in a group of [0, n_groups).  Per batch:
 *   root(p)   = p for p < n_seeds, else root(in.cols[p - n_seeds]): the forest contract rows[e] == n_seeds + e,
 *               cols[e] < n_seeds + e (see rows_prefilled) ends a chase after at most n_hops parents
 *   group(p)  = seed_group[root(p)]
 *   nodes[b]  the ids of the distinct PAIRS (group(p), samples[b][p]), p < n, ordered by the position of their first
 *             occurrence; group[b][u] = the group of nodes[b][u] (pitch in.cap_nodes; PyG's `batch` vector)
 *   inverse, rows, cols, counts, layer_nodes: as tg_ns_homo_unique defines them, over the pair instead of the id.
 * The same node under two groups is two entries; inside one group (two seeds of it included) it is one.  The hash key is
 * group * id_bound + id: 32-bit keys when n_groups * id_bound <= 2^31, else 64-bit ones; n_groups * id_bound >= 2^63 is
 * refused.  Forms, rounds and the workspace rule are tg_ns_homo_unique's (the LDS form also holds a u16 group word per
 * position, so it needs n_groups <= 65 536; the flat form's workspace holds a u32 one).  out.rows / out.cols may be
 * in.rows / in.cols: every group is found before any edge is relabelled.  A batch that breaks the forest contract (a cols
 * word that is no earlier position, a chase longer than n_hops) gets unspecified values, nothing out of bounds, no spin.
 * Bad arguments are refused with TG_ERR_INVALID before anything is launched; no synchronisation, no read-back. */
typedef struct {
    int64_t *nodes;
    int64_t *inverse;     /* or NULL */
    int64_t *rows;
    int64_t *cols;
    int64_t *counts;
    int64_t *layer_nodes; /* or NULL */
    int64_t *group;       /* [n_batches * cap_nodes] */
} tg_ns_unique_grouped_out;
TG_API int tg_ns_homo_unique_grouped_form(int64_t cap_nodes, int64_t id_bound, int64_t n_groups, int64_t lds_limit_bytes,
                                          int32_t *form, int64_t *lds_bytes);
TG_API int tg_ns_homo_unique_grouped_workspace_bytes(int64_t cap_nodes, int64_t id_bound, int64_t n_groups,
                                                     int64_t n_batches, int64_t *bytes, int64_t *bytes_min);
TG_API int tg_ns_homo_unique_grouped(const tg_ns_out *in, int64_t n_batches, int64_t n_seeds, int32_t n_hops,
                                     int64_t id_bound, const int32_t *seed_group, int64_t n_groups,
                                     const tg_ns_unique_grouped_out *out, void *workspace, int64_t workspace_bytes,
                                     int32_t form, void *stream);

/* ---- per-batch, per-type node dedup and relabel of the typed slabs (tg_ns_hetero_batched's layout) ---------------------
 * tg_ns_homo_unique with a type dimension.  Input: per node type t a `samples` slab [n_batches * pitch_nodes[t]], per
 * relation r `rows` / `cols` slabs [n_batches * pitch_edges[r]] -- rows index positions of samples[rel_src[r]], cols
 * positions of samples[rel_dst[r]] -- and counts[b * counts_stride ..] = {len(samples[t]) for t..., len(edges r) for
 * r...}, counts_stride >= n_types + n_rels (tg_ns_hetero_batched: exactly that; layouts whose rows carry tail words pass
 * their own stride).  For every batch b and type t independently (n = counts[b][t], clamped to the pitch):
 *   nodes[t][b]        the distinct values of samples[t][b][:n] in order of FIRST occurrence (distinct seeds stay first)
 *   inverse[t][b][p]   index of samples[t][b][p] in nodes[t][b]       (the array, or single entries of it, may be NULL)
 * and for every relation r (m = counts[b][n_types + r], clamped):
 *   rows[r][b][e] = inverse[rel_src[r]][in.rows[r][b][e]], cols[r][b][e] = inverse[rel_dst[r]][in.cols[r][b][e]], e < m;
 *                      an end that is no position of its list gives -1; edges are not merged
 *   counts[b * counts_stride ..] = {n_unique[t]..., m[r]...}; the words of a row past n_types + n_rels are not written
 *   seed_counts[b * n_types + t]  distinct values among the first min(n_inputs[t], n) positions: the unique seeds
 *                                                                                                      (may be NULL)
 * Words past n_unique / n / m of an output row are not written; the sampler's edge_index slabs are no argument.  out.rows /
 * out.cols may be in.rows / in.cols (in place); out.counts is not in.counts.  Array-of-pointer fields, pitches, rel_src /
 * rel_dst, n_inputs and id_bound are HOST arrays; what the pointers inside point to is device memory.
 * Every id of type t is in [0, id_bound[t]): id_bound[t] <= 2^31 takes 32-bit hash keys for that type, else 64-bit ones.
 * `form`: 0 auto, 1 LDS, 2 flat.  LDS: one workgroup runs one batch, type after type through one table area sized for the
 * type that needs most (2^k >= 4/3 pitch slots of key + u32), with a u16 word per position of EVERY type kept in LDS, so
 * the relabel of every relation reads only LDS and the edge slabs; it needs max_t(slots[t] * (key bytes[t] + 4)) +
 * 2 * sum_t(pitch_nodes[t] rounded up to 8) + 256 bytes and every pitch <= 32 768.  Flat: a grid over (tile of positions,
 * batch, type) with one table, one slot word per position and one count per tile for every type of a batch in `workspace`
 * (cleared inside the call).  Outputs depend on neither the form nor the workspace size: a workspace of at least
 * bytes_min and less than bytes runs the batches in rounds of as many as fit.  Limits: n_types in [1,
 * TG_HET_MAX_TYPES], n_rels in [0, TG_HET_MAX_RELS], pitches in [0, 2^30], rel_src / rel_dst in [0, n_types).  Bad
 * arguments are refused with TG_ERR_INVALID before anything is launched; the call does not synchronise and reads nothing
 * back. */
typedef struct {
    int32_t n_types, n_rels;
    const int32_t *rel_src;            /* [n_rels] type whose list `rows` index */
    const int32_t *rel_dst;            /* [n_rels] type whose list `cols` index */
    const int64_t *const *samples;     /* [n_types] device slabs [n_batches * pitch_nodes[t]] */
    const int64_t *pitch_nodes;        /* [n_types] */
    const int64_t *const *rows;        /* [n_rels] device slabs [n_batches * pitch_edges[r]] */
    const int64_t *const *cols;
    const int64_t *pitch_edges;        /* [n_rels] */
    const int64_t *counts;             /* device [n_batches * counts_stride] */
    int64_t counts_stride;
    const int64_t *n_inputs;           /* [n_types] seeds per batch (as tg_het_problem; <= 0: none); NULL without seed_counts */
    const int64_t *id_bound;           /* [n_types] */
} tg_ns_typed_in;

typedef struct {
    int64_t *const *nodes;             /* [n_types] device slabs, pitch_nodes */
    int64_t *const *inverse;           /* [n_types] or NULL */
    int64_t *const *rows;              /* [n_rels] device slabs, pitch_edges */
    int64_t *const *cols;
    int64_t *counts;                   /* device [n_batches * counts_stride] */
    int64_t *seed_counts;              /* device [n_batches * n_types], or NULL */
} tg_ns_typed_unique_out;
/* Which form an auto call takes: *form = 1 (LDS) or 2 (flat); *lds_bytes = the LDS the LDS form asks for.
 * lds_limit_bytes > 0 is taken as the workgroup's LDS limit and no device is touched; <= 0 asks the current device. */
TG_API int tg_ns_typed_unique_form(int32_t n_types, const int64_t *pitch_nodes, const int64_t *id_bound,
                                   int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes);
/* *bytes_min = the flat form's workspace of ONE batch (every type's table, slot words and tile counts), *bytes = what an
 * auto call wants for all n_batches at once: n_batches * bytes_min, or 0 where auto takes the LDS form on the current
 * device. */
TG_API int tg_ns_typed_unique_workspace_bytes(int32_t n_types, const int64_t *pitch_nodes, const int64_t *id_bound,
                                              int64_t n_batches, int64_t *bytes, int64_t *bytes_min);
TG_API int tg_ns_typed_unique(const tg_ns_typed_in *in, int64_t n_batches, const tg_ns_typed_unique_out *out,
                              void *workspace, int64_t workspace_bytes, int32_t form, void *stream);

/* ---- per-batch induced subgraph of a list of distinct nodes (PyG directed=False / subgraph_type="induced") --------------
 * The dedup above fixes the node contract; its edges are still the sampler's forest.  This pair makes, for every batch b
 * independently (nodes = in.nodes[b][:n], n = counts[b * counts_stride] clamped to the pitch), EVERY edge of the graph
 * between two nodes of the batch:
 *   local(v) = the FIRST position of v in nodes                  (no position: v is not in the batch)
 *   for i in 0 .. n-1, for e in ptrs[nodes[i]] .. ptrs[nodes[i]+1]-1 ascending:
 *       j = local(indices[e]);  if j exists: emit (row = j, col = i, edge_index = e)
 * Output order is (i, e) ascending; parallel edges (separate CSC offsets) are each emitted, self loops too; m_b = the
 * number of triples.  This is the edge loop of PyG's neighbor_sample(..., directed=False).  The contract is a
 * list of distinct ids (tg_ns_unique_out.nodes); a list with repeats is still deterministic -- every position scans its
 * column, local is the first position -- and never faults.  An id outside [0, csc->n_major) is a column of length 0 and
 * raises status bit 1.
 * Two exact passes: tg_ns_induced_count gives m_b, the caller allocates and passes the exclusive prefix, tg_ns_induced_emit
 * writes; no capacity guess, no retry.  Columns are scanned in chunks of 512 consecutive CSC offsets spread over the whole
 * device (a hub column is scanned by many wavefronts at once), each entry probed in the batch's hash table in `workspace`.
 * The workspace is bounded by the graph: distinct nodes have disjoint columns, so a batch has at most pitch_nodes +
 * ceil(csc->n_edges / 512) chunks.  A list with repeats that exceeds the bound raises status bit 0 and gets m_b = 0 (pass
 * 2 writes nothing for it); other batches are unaffected.  The workspace must hold all n_batches at once (bytes =
 * n_batches * bytes_min; a caller with less memory splits the launch).  id_bound (>= csc->n_major) <= 2^31 takes 32-bit
 * hash keys, else 64-bit ones; indices32 / ptrs32 are used when given, with equal results.  Limits: pitch_nodes in
 * [0, 2^30], n_marks in [0, TG_MAX_HOPS], the chunk bound <= 2^31.  Bad arguments (null pointers, negative sizes, a short or
 * misaligned workspace) are refused with TG_ERR_INVALID before anything is launched; the calls do not synchronise,
 * allocate or read back. */
typedef struct {
    const int64_t *nodes;      /* device [n_batches * pitch_nodes]: distinct ids per batch (tg_ns_unique_out.nodes) */
    int64_t pitch_nodes;
    const int64_t *counts;     /* device: n of batch b = counts[b * counts_stride] (tg_ns_unique_out.counts: stride 2) */
    int64_t counts_stride;
    const int64_t *node_marks; /* device [n_batches * n_marks] or NULL: positions (e.g. tg_ns_unique_out.layer_nodes) */
    int32_t n_marks;
} tg_ns_induced_in;

TG_API int tg_ns_induced_workspace_bytes(const tg_graph *csc, int64_t pitch_nodes, int64_t id_bound, int64_t n_batches,
                                         int64_t *bytes, int64_t *bytes_min /* one batch */);
/* pass 1: n_edges[b] = m_b (device [n_batches]); edge_marks[b*n_marks+k] = induced edges with col < clamp(node_marks[b][k], 0, n)
 * (or NULL); leaves tables / prefixes in `workspace` for pass 2.  status: device int32, zeroed by the caller. */
TG_API int tg_ns_induced_count(const tg_graph *csc, const tg_ns_induced_in *in, int64_t n_batches, int64_t id_bound,
                               int64_t *n_edges, int64_t *edge_marks, int32_t *status, void *workspace,
                               int64_t workspace_bytes, void *stream);
/* pass 2, same arguments and the SAME untouched workspace: batch b's triples to rows / cols / edge_index[edge_off[b] ..
 * edge_off[b] + m_b) of three FLAT arrays (edge_off: device [n_batches], the caller's exclusive prefix of n_edges).
 * Nothing outside those ranges is written. */
TG_API int tg_ns_induced_emit(const tg_graph *csc, const tg_ns_induced_in *in, int64_t n_batches, int64_t id_bound,
                              const int64_t *edge_off, int64_t *rows, int64_t *cols, int64_t *edge_index,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ---- induced edges per SUBGRAPH of a disjoint list (ShaDow-GNN's k-hop sampler; subgraph_type="induced" under times) -----
 * The pair above with a group dimension, behind tg_ns_homo_unique_grouped.  Per batch b (n as above):
 *   local(g, v) = the FIRST position p < n with (group[p], nodes[p]) == (g, v)
 *   for i in 0 .. n-1, g = group[i], for e in ptrs[nodes[i]] .. ptrs[nodes[i]+1]-1 ascending:
 *       j = local(g, indices[e]);  if j exists and the edge is admitted: emit (row = j, col = i, edge_index = e)
 * Order is (i, e) ascending, parallel edges and self loops are kept, both ends of every triple share a group.  Admitted:
 * always when group_time is NULL (csc->timestamps is then not looked at); else the backward TG_FILTER_RELATIVE predicate of
 * the filtered hops, window_lo <= group_time[b][g] - csc->timestamps[e] <= window_hi in wrapping int64 arithmetic
 * (csc->timestamps NULL is then refused).  The timestamp is read only behind a table hit; both passes evaluate the same
 * predicate.  The hash key is group * id_bound + id as in tg_ns_homo_unique_grouped: 32-bit while n_groups * id_bound <=
 * 2^31, else 64-bit, >= 2^63 refused; n_groups in [1, 2^31).
 * status: bit 1 as above; a group word outside [0, n_groups) makes its position a column of length 0 that is no `local` of
 * anything and raises bit 2 (value 4).
 * Capacity: columns of a disjoint list are NOT disjoint (a hub reached from many seeds is one entry per seed), so the
 * caller states how many chunks per batch the workspace holds: chunk_cap (<= 0: the ungrouped bound pitch_nodes +
 * ceil(n_edges / 512); at most 2^31).  chunks[b] (device int64 [n_batches], or NULL) always receives the batch's exact
 * chunk count, the sum over positions of ceil(column length / 512).  A batch with chunks[b] > chunk_cap raises status bit 0,
 * gets m_b = 0 and nothing from pass 2; other batches are unaffected; the caller may repeat both passes with chunk_cap =
 * max(chunks) in a workspace of that size.  edge_marks, the two exact passes, the untouched workspace between them, no
 * allocation / synchronisation / read-back and refusals with TG_ERR_INVALID before any launch are the ungrouped pair's. */
typedef struct {
    const int64_t *nodes;       /* device [n_batches * pitch_nodes]: tg_ns_unique_grouped_out.nodes */
    const int64_t *group;       /* device [n_batches * pitch_nodes]: tg_ns_unique_grouped_out.group */
    int64_t pitch_nodes;
    const int64_t *counts;
    int64_t counts_stride;
    const int64_t *node_marks;  /* as tg_ns_induced_in */
    int32_t n_marks;
    int64_t n_groups;
    const int64_t *group_time;  /* device [n_batches * n_groups] or NULL: no time filter */
    int64_t window_lo, window_hi;
    int64_t chunk_cap;          /* chunks per batch the workspace holds; <= 0: pitch_nodes + ceil(n_edges / 512) */
} tg_ns_induced_grouped_in;

TG_API int tg_ns_induced_grouped_workspace_bytes(const tg_graph *csc, int64_t pitch_nodes, int64_t id_bound, int64_t n_groups,
                                                 int64_t chunk_cap, int64_t n_batches, int64_t *bytes,
                                                 int64_t *bytes_min /* one batch */);
TG_API int tg_ns_induced_grouped_count(const tg_graph *csc, const tg_ns_induced_grouped_in *in, int64_t n_batches,
                                       int64_t id_bound, int64_t *n_edges, int64_t *edge_marks, int64_t *chunks,
                                       int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);
TG_API int tg_ns_induced_grouped_emit(const tg_graph *csc, const tg_ns_induced_grouped_in *in, int64_t n_batches,
                                      int64_t id_bound, const int64_t *edge_off, int64_t *rows, int64_t *cols,
                                      int64_t *edge_index, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Cluster-GCN mini-batches: the induced subgraph of a UNION OF CLUSTERS (PyG's ClusterLoader, DGL's ClusterGCNSampler) --
 * The nodes of csc are numbered so that cluster c of a fixed partition is the id range [partptr[c], partptr[c+1])
 * (partptr ascends from 0 to csc->n_major: ranges of distinct clusters are disjoint).  For every batch b independently,
 * with its cluster list c_0 .. c_{q-1} (q = n_clusters[b] clamped to [0, pitch_parts]; pitch_parts each without
 * n_clusters):
 *   size_k = partptr[c_k+1] - partptr[c_k];  base_k = size_0 + .. + size_{k-1};  n_b = base_q
 *   position i in [base_k, base_k + size_k) is vertex v_i = partptr[c_k] + (i - base_k)
 *   local(u) = base_k + (u - partptr[c_k]) for the FIRST k whose range holds u       (no such k: u is not in the batch)
 *   for i in 0 .. n_b-1, for e in ptrs[v_i] .. ptrs[v_i+1]-1 ascending:
 *       j = local(indices[e]);  if j exists: emit (row = j, col = i, edge_index = e)
 * Output order is (i, e) ascending; parallel edges and self loops are emitted; m_b = the number of triples.  That is word
 * for word tg_ns_induced_* over the list nodes[b] = (v_0 .. v_{n_b-1}), between-cluster edges included, and also where a
 * cluster is named twice: every position scans its column, local is the first position.  What the partition saves: no
 * hash table (the batch's distinct ranges, sorted, sit in LDS; a neighbour costs one search there), no idle lanes (a
 * cluster's CSC entries are ONE offset range, scanned in chunks of 512 consecutive offsets that cross column boundaries;
 * a hub column is still split over many chunks), no node list read (it is implied, and written once by pass 2).
 * Two exact passes, as the induced pair: tg_cluster_count gives n_b and m_b, the caller computes the two exclusive
 * prefixes, tg_cluster_emit writes; the workspace stays untouched between them; neither call allocates, synchronises or
 * reads back.  The workspace holds all n_batches at once (bytes = n_batches * bytes_min), bounded by the graph: distinct
 * clusters have disjoint offset ranges, so a batch has at most pitch_parts + ceil(csc->n_edges / 512) chunks.
 * status (device int32, zeroed by the caller):
 *   bit 1 (value 2): a cluster id outside [0, n_parts); the entry contributes no nodes.
 *   bit 2 (value 4): a partptr pair that is inverted or leaves [0, csc->n_major]; the entry is treated as empty and never
 *                    indexes ptrs out of range.  (A partptr that does not ascend elsewhere can make ranges overlap: the
 *                    output is then still deterministic and in bounds, local(u) taken from the range with the greatest
 *                    start <= u.)
 *   bit 0 (value 1): a batch with more chunks than the bound (only possible with repeated clusters) or with n_b >= 2^31:
 *                    it gets n_b = m_b = 0 and nothing from pass 2; other batches are unaffected.
 * Limits: csc->n_major <= 2^31 (else TG_ERR_UNSUPPORTED); pitch_parts in [0, TG_CLUSTER_MAX_PARTS_PER_BATCH]; the chunk
 * bound <= 2^31; indices32 / ptrs32 are used when given, with equal results.  Null buffers, negative sizes, a pitch above
 * the limit and a short or misaligned (8 bytes) workspace are refused with TG_ERR_INVALID before anything is launched;
 * n_batches = 0 launches nothing; more batches than one grid's y extent run in rounds. */
#define TG_CLUSTER_MAX_PARTS_PER_BATCH 1024
typedef struct {
    const int64_t *partptr;     /* device [n_parts + 1]: cluster c = ids [partptr[c], partptr[c+1]) of csc */
    int64_t n_parts;
    const int64_t *clusters;    /* device [n_batches * pitch_parts]: batch b's cluster ids, in the caller's order */
    int64_t pitch_parts;        /* 0 .. TG_CLUSTER_MAX_PARTS_PER_BATCH */
    const int64_t *n_clusters;  /* device [n_batches] or NULL (= pitch_parts each); clamped to [0, pitch_parts] */
    const int64_t *node_ids;    /* device [csc->n_major] or NULL: `nodes` receives node_ids[v] instead of v */
} tg_cluster_in;

TG_API int tg_cluster_workspace_bytes(const tg_graph *csc, int64_t n_parts, int64_t pitch_parts, int64_t n_batches,
                                      int64_t *bytes, int64_t *bytes_min /* one batch */);
/* pass 1: n_nodes[b] = n_b, n_edges[b] = m_b (device [n_batches] each); leaves the plan and the chunk prefixes in
 * `workspace` for pass 2. */
TG_API int tg_cluster_count(const tg_graph *csc, const tg_cluster_in *in, int64_t n_batches, int64_t *n_nodes,
                            int64_t *n_edges, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);
/* pass 2, same arguments and the SAME untouched workspace: v_i (node_ids[v_i] when given) to nodes[node_off[b] + i] (nodes
 * may be NULL: nothing is written for it), batch b's triples to rows / cols / edge_index[edge_off[b] .. edge_off[b] + m_b)
 * of three FLAT arrays (node_off, edge_off: device [n_batches], the caller's exclusive prefixes of n_nodes and n_edges).
 * Nothing outside those ranges is written. */
TG_API int tg_cluster_emit(const tg_graph *csc, const tg_cluster_in *in, int64_t n_batches, const int64_t *node_off,
                           const int64_t *edge_off, int64_t *nodes, int64_t *rows, int64_t *cols, int64_t *edge_index,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* ---- full-neighbour hop: EVERY in-edge of a frontier (PyG's num_neighbors=[-1], DGL's MultiLayerFullNeighborSampler) -------
 * The layer of layer-wise inference: no sampling, no fan-out limit, a ragged exact output.  For every batch b independently,
 * with its frontier v_0 .. v_{n-1} = nodes[node_ptr[b] .. node_ptr[b+1]) (n clamped to [0, max_nodes]):
 *   col(i) = the CSC column [ptrs[v_i], ptrs[v_i+1]); an id outside [0, csc->n_major) is a column of length 0 and raises
 *            status bit 1 (value 2)
 *   for i in 0 .. n-1, for e in col(i) ascending: triple k = (src_k = indices[e], col = i, edge_index = e)
 *   m_b = the number of triples, the sum of the column lengths; parallel edges and self loops are each emitted
 *   out_nodes = v_0 .. v_{n-1}, followed by every src that equals no earlier entry of out_nodes, in order of first
 *               occurrence in triple order;  n_out_b = len(out_nodes)
 *   row_k = the FIRST position of src_k in out_nodes
 * A frontier with repeats stays deterministic and in bounds: every position emits its column, rows point to the first
 * position.  Sources are expected inside [0, id_bound).
 * Two exact passes.  tg_ns_full_count writes n_nodes[b] = n_out_b, n_edges[b] = m_b and chunks[b] (may be NULL) = the sum
 * over positions of ceil(column length / 512), and leaves its tables and prefixes in `workspace`; the caller computes the
 * exclusive prefixes node_off / edge_off; tg_ns_full_emit, with the same arguments and the SAME untouched workspace, writes
 * out_nodes to nodes_out[node_off[b] ..) (nodes_out may be NULL: nothing is written for it) and the triples to rows / cols /
 * edge_index[edge_off[b] .. edge_off[b] + m_b) of three flat arrays.  Nothing outside those ranges is written.  Pass 2
 * leaves the new positions in the workspace's table: a second tg_ns_full_emit needs a second tg_ns_full_count.  Neither call
 * allocates, synchronises or reads back.
 * Capacity, decided per batch before any table work: a batch with n + min(m_b, id_bound) > node_cap, with chunks[b] >
 * the chunk bound (chunk_cap; <= 0: max_nodes + ceil(csc->n_edges / 512), what a frontier of distinct nodes needs at most)
 * or with m_b >= 2^31 is refused: status bit 0 (value 1), n_nodes[b] = 0, n_edges[b] and chunks[b] still exact, so the caller
 * can repeat with a workspace of that size; pass 2 writes nothing for it; other batches are unaffected.
 * Columns are scanned in chunks of 512 consecutive CSC offsets spread over the whole device (a hub column is many chunks);
 * every entry is inserted into the batch's hash table with the index of its triple, so the first occurrence is decided
 * across chunks.  Hash keys are 32-bit while id_bound (>= csc->n_major) <= 2^31, else 64-bit; indices32 / ptrs32 are used
 * when given, with equal results.  Limits: max_nodes in [0, 2^30], node_cap in [max_nodes, 2^30], the chunk bound <= 2^31.
 * Null buffers, negative sizes, id_bound < csc->n_major and a short or misaligned (8 bytes) workspace are refused with
 * TG_ERR_INVALID before anything is launched; n_batches = 0 launches nothing; more batches than one grid's y extent run in
 * rounds.  The workspace holds all n_batches at once (bytes = n_batches * bytes_min). */
typedef struct {
    const int64_t *nodes;     /* device, flat: batch b's frontier is nodes[node_ptr[b] .. node_ptr[b+1]) */
    const int64_t *node_ptr;  /* device [n_batches + 1], ascending from any base */
    int64_t max_nodes;        /* the caller's bound on node_ptr[b+1]-node_ptr[b]; a longer list is clamped to it */
    int64_t node_cap;         /* distinct nodes (frontier + new sources) per batch the workspace's table holds */
    int64_t chunk_cap;        /* chunks per batch the workspace holds; <= 0: max_nodes + ceil(n_edges / 512) */
} tg_ns_full_in;

/* only the sizes of `in` (max_nodes, node_cap, chunk_cap) are read */
TG_API int tg_ns_full_workspace_bytes(const tg_graph *csc, const tg_ns_full_in *in, int64_t id_bound, int64_t n_batches,
                                      int64_t *bytes, int64_t *bytes_min /* one batch */);
/* pass 1: n_nodes, n_edges, chunks: device int64 [n_batches] (chunks may be NULL); status: device int32, zeroed by the caller */
TG_API int tg_ns_full_count(const tg_graph *csc, const tg_ns_full_in *in, int64_t n_batches, int64_t id_bound,
                            int64_t *n_nodes, int64_t *n_edges, int64_t *chunks, int32_t *status, void *workspace,
                            int64_t workspace_bytes, void *stream);
/* pass 2: node_off, edge_off: device [n_batches], the caller's exclusive prefixes of n_nodes and n_edges */
TG_API int tg_ns_full_emit(const tg_graph *csc, const tg_ns_full_in *in, int64_t n_batches, int64_t id_bound,
                           const int64_t *node_off, const int64_t *edge_off, int64_t *nodes_out, int64_t *rows, int64_t *cols,
                           int64_t *edge_index, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- GraphSAINT's random-walk sampler: a SUBGRAPH per mini-batch (PyG's GraphSAINTRandomWalkSampler) ---------------------
 * tg_saint_rw_nodes: one launch takes G = n_batches mini-batches of B = batch_size roots (roots: device [G, B]); every
 * root walks T = walk_length >= 1 uniform steps over csr.  Per mini-batch g: walker i starts at roots[g][i] and its
 * vertices x_i[0..T] are, value for value, row i of tg_random_walk(start = roots[g], n = B, T, p = q = 1, seed, call id =
 * rng->call_id + g); a walker that meets a vertex without out-edges stops there (tg_random_walk's -1 padding is no visit).
 * The visit x_i[l] has position p = l * B + i (step-major: the distinct roots lead); nodes[g] = the distinct visited
 * vertices ordered by the position of their first occurrence, counts[g * counts_stride] = their number n_unique; words
 * past n_unique are not written.  pitch_nodes >= P = B * (T + 1).  nodes / pitch_nodes / counts / counts_stride go
 * straight into tg_ns_induced_in.  A root outside [0, csr->n_major) contributes nothing, raises bit 1 (value 2) of the
 * caller-zeroed device word `status` and never indexes ptrs.
 * form: 0 auto, 1 LDS (one workgroup walks and dedups one mini-batch in LDS: a table of 2^k >= 4P/3 slots of 8 bytes plus
 * 2 bytes per position, P <= 12 288 in 160 KiB, where a CU holds one such workgroup; no workspace), 2 flat (any P; visit
 * lists and tables in `workspace`: bytes = n_batches * bytes_min runs all mini-batches at once, anything from bytes_min up
 * runs them in rounds).  Both forms write identical words.  tg_saint_rw_form / _workspace_bytes: lds_limit_bytes > 0
 * replaces the device's limit (no device is touched); a forced form asks no device either.
 * Limits: csr->n_major <= 2^31 (else TG_ERR_UNSUPPORTED), P <= 2^30; indices32 / ptrs32 are used when given, with equal
 * results.  Null buffers, T < 1, B < 0, a short pitch, counts_stride < 1, a forced form 1 that does not fit, a short or
 * misaligned (8 bytes) workspace are refused with TG_ERR_INVALID before any launch; G = 0 or B = 0 launches nothing.  The
 * call does not synchronise, allocate or read back. */
typedef struct {
    int64_t *nodes;        /* device [n_batches * pitch_nodes] */
    int64_t pitch_nodes;
    int64_t *counts;       /* device: n_unique of mini-batch g at counts[g * counts_stride] */
    int64_t counts_stride;
} tg_saint_rw_out;

TG_API int tg_saint_rw_capacity(int64_t batch_size, int64_t walk_length, int64_t *positions);
TG_API int tg_saint_rw_form(int64_t batch_size, int64_t walk_length, int64_t lds_limit_bytes, int32_t *form,
                            int64_t *lds_bytes);
TG_API int tg_saint_rw_workspace_bytes(int64_t n_batches, int64_t batch_size, int64_t walk_length, int32_t form,
                                       int64_t *bytes, int64_t *bytes_min /* one mini-batch */);
TG_API int tg_saint_rw_nodes(const tg_graph *csr, const int64_t *roots, int64_t n_batches, int64_t batch_size,
                             int64_t walk_length, const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status,
                             void *workspace, int64_t workspace_bytes, int32_t form, void *stream);

/* GraphSAINT's coverage counters: node_count[v] += 1 for every listed node of every mini-batch (nodes / pitch_nodes /
 * counts / counts_stride as above, n clamped to the pitch), edge_count[e] += 1 for every entry of the flat edge_ids (the
 * edge_index words of tg_ns_induced_emit: CSC offsets).  Both tables are device int64, updated with atomic adds: the
 * caller zeroes them once and may call repeatedly.  An id outside its table is skipped and raises status bit 1 (value 2). */
TG_API int tg_saint_coverage_add(const int64_t *nodes, int64_t pitch_nodes, const int64_t *counts, int64_t counts_stride,
                                 int64_t n_batches, const int64_t *edge_ids, int64_t n_edge_ids, int64_t *node_count,
                                 int64_t n_nodes, int64_t *edge_count, int64_t n_edges, int32_t *status, void *stream);
/* The two normalisation vectors (float32) of n_samples pre-sampled mini-batches:
 *   edge_norm[e], e in column c of csc (c = the edge's target): r = (float)node_count[c] / (float)edge_count[e];
 *                 NaN (0/0) -> 0.1f, otherwise min(max(r, 0), 1e4f) (x/0 = inf -> 1e4f)
 *   node_norm[v] = ((float)n_samples / d) / (float)n_major, d = (float)node_count[v], 0.1f where the count is 0
 * The edge pass runs over chunks of consecutive CSC offsets, so a hub column is shared by many wavefronts. */
TG_API int tg_saint_norm(const tg_graph *csc, const int64_t *node_count, const int64_t *edge_count, int64_t n_samples,
                         float *node_norm, float *edge_norm, void *stream);

/* ---- GraphSAINT's node and edge samplers (PyG's GraphSAINTNodeSampler / GraphSAINTEdgeSampler) --------------------------
 * Both write tg_saint_rw_out under tg_saint_rw_nodes' rules: G = n_batches mini-batches of B = batch_size slots, every
 * visit has a position p < P, nodes[g] = the distinct visited ids ordered by the position of their first occurrence,
 * counts[g * counts_stride] = their number n_unique, words past n_unique are not written, pitch_nodes >= P.
 *   draws     slot i of mini-batch g takes ONE Philox block: w = draw(call key of (rng->seed, rng->call_id + g, tag), id = i,
 *             d0 = 0, d1 = 0), lo = w0 | w1 << 32, hi = w2 | w3 << 32 (as tg_link_seeds splits them); every bounded pick is
 *             floor(x * n / 2^64).  tag = TG_TAG_SAINT_NODE / TG_TAG_SAINT_EDGE.
 * tg_saint_node_nodes: slot i picks the entry e = floor(lo * graph->n_edges / 2^64); its node indices[e] sits at position
 *             i; P = B.  Given the CSC this picks a source with probability out-degree / E (PyG's law), given the CSR a
 *             target with probability in-degree / E.  A value outside [0, id_bound) contributes nothing and raises bit 1
 *             (value 2) of the caller-zeroed device word `status`.  graph->ptrs is not read.
 * tg_saint_edge_nodes: slot i picks t = floor(lo * (n_cols + n_rows) / 2^64).
 *               t < n_cols:  c = cols[t], k = floor(hi * deg_csc(c) / 2^64), source = csc.indices[csc.ptrs[c] + k], target = c
 *               otherwise:   r = rows[t - n_cols], k = floor(hi * deg_csr(r) / 2^64), source = r,
 *                            target = csr.indices[csr.ptrs[r] + k]
 *             The source sits at position i, the target at position B + i (PyG's cat([source, target])); P = 2 B.
 *   law       when cols / rows are exactly the non-empty columns of the CSC / rows of the CSR of one graph, the entry
 *             (u -> v) is drawn with probability (1 / deg_in(v) + 1 / deg_out(u)) / (n_cols + n_rows): the paper's law
 *             p_e ~ 1/deg(u) + 1/deg(v) as a mixture of "a uniform non-empty column, then a uniform entry of it" and the
 *             same over rows -- no prefix sum or alias table over E.  Parallel entries count separately.  Draws are
 *             INDEPENDENT, with replacement; PyG takes a Gumbel top-k (without replacement) over all E entries for every
 *             mini-batch.  csr == NULL with n_rows == 0 is legal and gives the one-sided (column) law.
 *   slots     a listed major outside its graph contributes nothing, never indexes ptrs and raises status bit 1 (value 2);
 *             a listed major without entries contributes nothing and raises bit 2 (value 4); a drawn endpoint (either
 *             one) >= id_bound raises bit 1 and the slot contributes NEITHER end.
 * form: 0 auto, 1 LDS (one workgroup draws and dedups one mini-batch in LDS; nsu's table of 2^k >= 4P/3 slots of 8 bytes
 * plus 2 bytes per position, sized by P so that small mini-batches share a CU; P <= 12 288; no workspace), 2 flat (any
 * P <= 2^30; visit words and tables in `workspace`: bytes = n_batches * bytes_min runs all mini-batches at once, anything
 * from bytes_min up runs them in rounds).  Both forms write identical words.  tg_saint_ne_form / _workspace_bytes speak in
 * positions P (B, or 2 B for the edge sampler): lds_limit_bytes > 0 replaces the device's limit (no device is touched); a
 * forced form asks no device either.
 * Limits: ids below 2^31 (id_bound > 2^31: TG_ERR_UNSUPPORTED), P <= 2^30; ptrs32 / indices32 are used when given, with
 * equal words.  Refused with TG_ERR_INVALID before any launch: null graph / in / rng / out / nodes / counts / status, null
 * indices of a graph with entries, null ptrs of csc / csr, a list without its graph or null with entries, negative sizes,
 * id_bound < 1, B < 0, n_edges == 0 (node) or n_cols + n_rows == 0 (edge) with B > 0, a short pitch, counts_stride < 1,
 * an unknown form, a forced form 1 that does not fit, a short or misaligned (8 bytes) workspace.  G = 0 or B = 0 launches
 * nothing.  The calls do not synchronise, allocate or read back. */
#define TG_TAG_SAINT_NODE 16u
#define TG_TAG_SAINT_EDGE 17u
typedef struct {
    const tg_graph *csc;   /* columns = targets: deg_csc(c) = in-degree                   */
    const int64_t *cols;   /* device [n_cols]: the columns to draw from                   */
    int64_t n_cols;
    const tg_graph *csr;   /* rows = sources: deg_csr(r) = out-degree; NULL with n_rows 0 */
    const int64_t *rows;   /* device [n_rows]                                             */
    int64_t n_rows;
} tg_saint_edge_in;

TG_API int tg_saint_ne_form(int64_t positions, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes);
TG_API int tg_saint_ne_workspace_bytes(int64_t n_batches, int64_t positions, int32_t form, int64_t *bytes,
                                       int64_t *bytes_min /* one mini-batch */);
TG_API int tg_saint_node_nodes(const tg_graph *graph, int64_t id_bound, int64_t n_batches, int64_t batch_size,
                               const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status, void *workspace,
                               int64_t workspace_bytes, int32_t form, void *stream);
TG_API int tg_saint_edge_nodes(const tg_saint_edge_in *in, int64_t id_bound, int64_t n_batches, int64_t batch_size,
                               const tg_rng *rng, const tg_saint_rw_out *out, int32_t *status, void *workspace,
                               int64_t workspace_bytes, int32_t form, void *stream);

/* ---- PinSAGE's importance sampler: random-walk neighbours (DGL's RandomWalkNeighborSampler / PinSAGESampler) ---------------
 * tg_pinsage_hop: a flat hop over a frontier, shaped like tg_ns_hop_recent.  The neighbours of a frontier vertex are the
 * vertices that R = n_walks short random walks from it visit most often; the visit counts are the weights.
 *   walks     frontier slot i has draw id u = in->ids[i] (or in->id_base + i) and call id c = in->call_ids[i] (or
 *             rng->call_id).  It starts R walks at in->vertices[i]; walk r is walker w = u * R + r (uint64 arithmetic).
 *             Walker w takes up to T = walk_length uniform steps over walk_graph's rows: tg_random_walk's step with
 *             p = q = 1 under tg_random_walk's call key of (rng->seed, c), so that WITHOUT termination its vertices are,
 *             value for value, row w of tg_random_walk under call id c.  Pass the CSC to walk against edge direction, the
 *             CSR to walk along it.
 *   termination (DGL's restart_prob): the first step is always taken; before step l, 1 <= l < T, the walk ends if
 *             u32_to_f32_01(draw(ck', w, l, 0).w[0]) < termination, ck' the call key of the same (seed, c) under the tag
 *             in->rng_tag, 0 meaning TG_TAG_PINSAGE, and u32_to_f32_01(x) = float32 with the bits 0x3F800000 | x >> 9,
 *             minus 1.  A vertex without out-edges ends the walk too.
 *   visits    of slot i: the vertices after each step taken, x[1..] of all R walks; the start counts only where a walk
 *             steps back onto it.
 *   selection the distinct visited vertices ranked by visit count descending, then vertex id ascending; the first
 *             min(in->fanout, distinct) are kept.  Fan-outs 1..64.
 *   outputs   laid out as tg_ns_hop_recent's: cnt [m], offsets [m + 1] with offsets[m] the total, neighbors and parents
 *             compact and grouped by frontier slot in rank order; `visits` runs parallel to neighbors and holds each one's
 *             count as int64.  Words past offsets[m] are not written.  out->edge_ptrs must be NULL: a sampled neighbour is
 *             not an edge of the graph.
 *   slots     a vertex < 0 is an empty slot with cnt 0; a vertex >= n_major has cnt 0, raises bit 1 (value 2) of the
 *             caller-zeroed device word `status` and never indexes ptrs.  in->sampler is ignored.
 * Refused before any launch, without touching a device: with TG_ERR_INVALID a null graph, in, cfg, rng, out, and while
 * m > 0 null vertices, cnt, offsets, neighbors, parents, visits or status; a non-NULL edge_ptrs; R < 1 or T < 1; a fan-out
 * outside 1..64; termination outside [0, 1) or NaN; m < 0; a short or misaligned (8 bytes) workspace
 * (tg_pinsage_hop_workspace_bytes: m * fanout words, where the winners wait for their offsets); with TG_ERR_UNSUPPORTED
 * V = R * T > 4096 and n_major > 2^31.  m = 0 returns TG_OK and launches nothing.  The call does not allocate, synchronise
 * or read back; ptrs32 / indices32 are used when given, with equal results.  The visits live in LDS only: a workgroup
 * walks and selects a tile of consecutive slots (csrc/pinsage.hip); the result does not depend on the tile. */
#define TG_TAG_PINSAGE 15u
typedef struct {
    int32_t n_walks;        /* R >= 1 walks per frontier vertex              */
    int32_t walk_length;    /* T >= 1 steps per walk; V = R * T <= 4096      */
    float   termination;    /* alpha in [0, 1): before every step l >= 1     */
    int32_t _reserved;
} tg_pinsage_config;

TG_API int tg_pinsage_hop_workspace_bytes(int64_t m, int32_t fanout, int64_t *bytes);
TG_API int tg_pinsage_hop(const tg_graph *walk_graph, const tg_hop_in *in, const tg_pinsage_config *cfg,
                          const tg_rng *rng, const tg_hop_out *out, int64_t *visits, int32_t *status,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* Ragged rows of an int64 slab -> one flat array: dst[offsets[r] + i] = src[r * pitch + i] for
 * i < lens[r * lens_stride] (lens, offsets: device arrays).  The per-type / per-relation slabs of
 * tg_ns_hetero_batched are flattened with it (tch_geometric/loader.py). */
TG_API int tg_compact_rows(const int64_t *src, int64_t pitch, const int64_t *lens, int64_t lens_stride, const int64_t *offsets,
                           int64_t n_rows, int64_t *dst, void *stream);

/* Harness calibration (not part of the sampling path): n_threads lanes each issue per_thread
 * independent random 8-byte loads from table[0..n_table); sink: [n_threads]. */
TG_API int tg_probe_random_gather(const int64_t *table, int64_t n_table, int64_t n_threads, int64_t per_thread,
                                  uint64_t seed, int64_t *sink, void *stream);

/* Debug build only (`make dbg`, -DTG_DEBUG_BOUNDS -> lib/libtchgeo_hip_dbg.so): registers a device word; the multi-hop
 * neighbor-sampling kernels then compare every frontier id with n_major before it indexes `ptrs`, raise bit 0 of the word
 * for an offender and sample vertex 0 instead of reading out of bounds.  For experiments that drop or alter a hop's work.
 * The regular build trusts the ids (contract: ids in `indices` are < n_major) and returns TG_ERR_UNSUPPORTED here. */
TG_API int tg_debug_bounds_set_flag(uint32_t *device_word);

/* Harness calibration: the speed of light of neighbor_sampling_homogenous's output contract.  Moves the ALGORITHMIC bytes
 * of a finished launch `src` (per seed 8 B read + 8 B written, per expanded frontier slot 24 B read, per sampled edge 8 B
 * read + 32 B written) as pure streams into the slabs `dst` (same pitch, other memory) -- precomputed contents,
 * no draws, no random access, no ordering.  sink: [n_batches]. */
TG_API int tg_probe_ns_sol(const tg_ns_out *src, const tg_ns_out *dst, const int64_t *seeds, int64_t n_batches,
                           int64_t n_seeds, int32_t n_hops, int64_t *sink, void *stream);

#ifdef __cplusplus
}
#endif
#endif
