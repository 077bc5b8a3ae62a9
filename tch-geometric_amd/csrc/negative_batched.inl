// Batched negative sampling: ONE workgroup runs ONE whole call (included by negative.hip).
//
// tg_neg_sample is built for one huge call: a device hash map in global memory, device-wide scans, 8 or more dependent
// launches.  A mini-batch sized call (1 024 inputs x 5 negatives) is a few microseconds of work for one CU, so here the
// call's whole state lives in the LDS of the workgroup that runs it and only the CSR look-ups and the output stores touch
// global memory.  Call b draws with call_key(seed, call_id + b, tag) and the draw addresses of neg_candidates_kernel, so
// it equals tg_neg_sample run alone with call id call_id + b, word for word.
//
// LDS of a call with M items and at most I inputs of one type (32-bit words; ids, slots and positions are < 2^31):
//   keys [cap]  node id of the slot, NEGB_NONE = empty          cap = 2^k >= 4/3 (I + M): load factor <= 0.75
//   vals [cap]  NEGB_FLAG | input slot (atomicMax: the LAST input slot holding the id, negative_sampling.rs:26), or the
//               MINIMUM item position that produced the node (atomicMin), later the node's local id
//   cand [M]    accepted node of the item, NEGB_NONE = none
//   ids  [M]    local id of the item's node; NEGB_FLAG | table slot while the node's id is not known yet
//   rel  [M]    u8 relation of the item
// One table serves inputs and new nodes of a destination type (an id is one or the other); it is cleared per type.
// The order-preserving parts are exclusive scans in item order over the workgroup: a thread owns a contiguous run of
// items, counts its flags, the counts are scanned (DPP inside a wave, wave totals through LDS).
#pragma once
#include <atomic>

namespace tg {

constexpr int NEGB_MAX_TYPES = 16;      // more node types: call by call
constexpr int NEGB_THREADS = 1024;
constexpr int NEGB_MAX_PER_THREAD = 32; // items a thread owns in a scan: its flags are one 32-bit mask
constexpr int NEGB_STATIC_LDS = 256;    // wave totals, destination types, panic word (upper bound)
constexpr uint32_t NEGB_NONE = 0xFFFFFFFFu;
constexpr uint32_t NEGB_FLAG = 0x80000000u;
constexpr uint32_t NEGB_UNSEEN = 0x7FFFFFFFu;

struct NegbArgs {
    NegRelTable tab;
    int64_t *rows[NEG_MAX_RELS], *cols[NEG_MAX_RELS]; // call 0's rows of the slabs
    int64_t edge_pitch[NEG_MAX_RELS];
    int32_t rel_src[NEG_MAX_RELS];
    int32_t src_rels[NEG_MAX_RELS];         // relations grouped by source type, edge_types order inside a group
    int32_t src_begin[NEGB_MAX_TYPES + 1];  // group of type t = src_rels[src_begin[t] .. src_begin[t + 1])
    const int64_t *inputs[NEGB_MAX_TYPES];  // [n_calls, n_in[t]]
    int64_t *samples[NEGB_MAX_TYPES];
    int64_t node_pitch[NEGB_MAX_TYPES];
    int32_t n_in[NEGB_MAX_TYPES];           // >= 0
    int32_t item_begin[NEGB_MAX_TYPES + 1]; // items of source type t = [item_begin[t], item_begin[t + 1])
    uint32_t dst_mask;                      // bit t: some relation ends in type t
    int32_t n_types, n_rels, hetero, inbound;
    uint32_t num_neg;                       // clamped to 2^31 - 1 (above the item count either way)
    int64_t try_count;
    uint64_t seed, call_id;
    int64_t *counts; // [n_calls, n_types + n_rels]
    int32_t *panic;  // [n_calls]
    int32_t n_calls;
    uint32_t cap_mask, hash_shift; // cap = cap_mask + 1 = 2^(32 - hash_shift)
};

__device__ __forceinline__ uint32_t negb_insert(uint32_t *keys, uint32_t mask, uint32_t shift, uint32_t key) {
    uint32_t s = (key * 0x9E3779B1u) >> shift;
    for (;;) { // ends: the table has more slots than a call has ids
        const uint32_t prev = atomicCAS(&keys[s], NEGB_NONE, key);
        if (prev == NEGB_NONE || prev == key) return s;
        s = (s + 1) & mask;
    }
}

// exclusive prefix of `cnt` over the threads of the workgroup in thread order, *total = the sum.  Every thread calls it.
__device__ __forceinline__ uint32_t negb_scan(uint32_t cnt, uint32_t *s_wave, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const uint32_t incl = wave_inclusive_scan_u32_dpp(cnt);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t carry = 0, sum = 0;
    for (int w = 0; w < n_waves; ++w) {
        const uint32_t v = s_wave[w];
        sum += v;
        if (w < wave) carry += v;
    }
    __syncthreads(); // s_wave is free again
    *total = sum;
    return carry + incl - cnt;
}

__global__ void __launch_bounds__(NEGB_THREADS) neg_batched_kernel(const NegbArgs a, const int M) {
    extern __shared__ __align__(16) unsigned char negb_lds[];
    __shared__ uint32_t s_wave[NEGB_THREADS / 64];
    __shared__ int32_t s_dst[NEG_MAX_RELS];
    __shared__ int32_t s_panic;
    const uint32_t cap = a.cap_mask + 1;
    uint32_t *keys = reinterpret_cast<uint32_t *>(negb_lds), *vals = keys + cap, *cand = vals + cap, *ids = cand + M;
    uint8_t *rel = reinterpret_cast<uint8_t *>(ids + M);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n_out = a.n_types + a.n_rels;
    if (tid < a.n_rels) s_dst[tid] = a.tab.r[tid].dst_type;
    const int per = (M + nt - 1) / nt; // <= NEGB_MAX_PER_THREAD
    const int p0 = min(M, tid * per), p1 = min(M, p0 + per);

    for (int64_t call = blockIdx.x; call < a.n_calls; call += gridDim.x) {
        if (tid == 0) s_panic = 0;
        __syncthreads(); // also: the previous call is done with the item arrays
        // ---- 1. candidates: lane per item, node type major, then (i, jn); the draws of neg_candidates_kernel
        for (int t = 0; t < a.n_types; ++t) {
            const int base = a.item_begin[t], m_t = a.item_begin[t + 1] - base;
            if (m_t == 0) continue;
            const int64_t *inputs = a.inputs[t] + call * a.n_in[t];
            const int sb = a.src_begin[t];
            const uint32_t n_src = (uint32_t)(a.src_begin[t + 1] - sb);
            const CallKey ck = call_key(a.seed, a.call_id + (uint64_t)call,
                                        a.hetero ? (TAG_NEG_HETERO | ((uint32_t)t << 8)) : TAG_NEG_HOMO);
            for (int q = tid; q < m_t; q += nt) {
                const uint32_t i = (uint32_t)q / a.num_neg, jn = (uint32_t)q - i * a.num_neg;
                const int64_t v = inputs[i];
                int r = a.src_rels[sb];
                if (a.hetero) { // negative_sampling.rs:104
                    const Draw d = draw(ck, (uint64_t)i, jn, 0xFFFFFFFFu);
                    r = a.src_rels[sb + (int)bounded64(d.a(), (uint64_t)n_src)];
                }
                const NegRel R = a.tab.r[r];
                uint32_t found = NEGB_NONE;
                for (int64_t tr = 0; tr < a.try_count; ++tr) { // :33 / :110
                    const Draw d = draw(ck, (uint64_t)i, jn, (uint32_t)tr);
                    const int64_t w = (int64_t)bounded64(d.a(), (uint64_t)R.node_count);
                    bool he;
                    if (a.inbound) { // :113: the reference panics when w is not a row
                        if (w >= R.row_count) {
                            s_panic = 1;
                            break;
                        }
                        he = neg_has_edge(R.ptrs, R.indices, w, v);
                    } else {
                        he = neg_has_edge(R.ptrs, R.indices, v, w);
                    }
                    if (!he && v != w) { // :35 / :117
                        found = (uint32_t)w;
                        break;
                    }
                }
                cand[base + q] = found;
                rel[base + q] = (uint8_t)r;
            }
        }
        __syncthreads();
        // ---- 2. local ids per destination type
        for (int dt = 0; dt < a.n_types; ++dt) {
            const int n_in = a.n_in[dt];
            const bool is_dst = ((a.dst_mask >> dt) & 1u) && M > 0;
            int64_t *samples = a.samples[dt] + call * a.node_pitch[dt];
            uint32_t n_new = 0;
            if (!is_dst) { // uniform; only the head of `samples`
                const int64_t *inputs = a.inputs[dt] + call * n_in;
                for (int i = tid; i < n_in; i += nt) samples[i] = inputs[i];
            } else {
                for (uint32_t s = tid; s < cap; s += nt) {
                    keys[s] = NEGB_NONE;
                    vals[s] = NEGB_UNSEEN;
                }
                __syncthreads();
                const int64_t *inputs = a.inputs[dt] + call * n_in;
                for (int i = tid; i < n_in; i += nt) { // value -> LAST slot holding it; the head of `samples`
                    const int64_t v = inputs[i];
                    samples[i] = v;
                    const uint32_t s = negb_insert(keys, a.cap_mask, a.hash_shift, (uint32_t)v);
                    atomicMax(&vals[s], NEGB_FLAG | (uint32_t)i);
                }
                __syncthreads();
                // items: known input -> its slot; otherwise the node keeps the smallest item position that produced it
                for (int p = tid; p < M; p += nt) {
                    const uint32_t w = cand[p];
                    if (w == NEGB_NONE || s_dst[rel[p]] != dt) continue;
                    const uint32_t s = negb_insert(keys, a.cap_mask, a.hash_shift, w);
                    const uint32_t v = vals[s]; // an input's value is final since the barrier
                    if (v & NEGB_FLAG) {
                        ids[p] = v & ~NEGB_FLAG;
                    } else {
                        ids[p] = NEGB_FLAG | s;
                        atomicMin(&vals[s], (uint32_t)p);
                    }
                }
                __syncthreads();
                // first sights (the item holds its node's minimum position), ranked in item order
                uint32_t first = 0;
                for (int p = p0; p < p1; ++p) {
                    const uint32_t w = cand[p];
                    if (w == NEGB_NONE || s_dst[rel[p]] != dt) continue;
                    const uint32_t v = ids[p];
                    if ((v & NEGB_FLAG) && vals[v & ~NEGB_FLAG] == (uint32_t)p) first |= 1u << (p - p0);
                }
                uint32_t rank = negb_scan((uint32_t)__popc(first), s_wave, &n_new); // barriers: every position is read
                while (first) {
                    const int p = p0 + __ffs(first) - 1;
                    first &= first - 1;
                    const uint32_t id = (uint32_t)n_in + rank++;
                    vals[ids[p] & ~NEGB_FLAG] = id;
                    samples[id] = (int64_t)cand[p]; // :37-38
                }
                __syncthreads();
                for (int p = tid; p < M; p += nt) {
                    const uint32_t w = cand[p];
                    if (w == NEGB_NONE || s_dst[rel[p]] != dt) continue;
                    const uint32_t v = ids[p];
                    if (v & NEGB_FLAG) ids[p] = vals[v & ~NEGB_FLAG];
                }
                __syncthreads(); // the next type clears the table
            }
            if (tid == 0) a.counts[call * n_out + dt] = (int64_t)n_in + (int64_t)n_new;
        }
        // ---- 3. edges per relation, in item order
        for (int r = 0; r < a.n_rels; ++r) {
            const int t = a.rel_src[r];
            const int b = a.item_begin[t], e = a.item_begin[t + 1];
            uint32_t n_edges = 0;
            if (e > b) { // uniform
                const int per_r = (e - b + nt - 1) / nt;
                const int q0 = min(e, b + tid * per_r), q1 = min(e, q0 + per_r);
                uint32_t acc = 0;
                for (int p = q0; p < q1; ++p)
                    if (cand[p] != NEGB_NONE && rel[p] == r) acc |= 1u << (p - q0);
                uint32_t rank = negb_scan((uint32_t)__popc(acc), s_wave, &n_edges);
                int64_t *rows = a.rows[r] + call * a.edge_pitch[r], *cols = a.cols[r] + call * a.edge_pitch[r];
                while (acc) {
                    const int p = q0 + __ffs(acc) - 1;
                    acc &= acc - 1;
                    rows[rank] = (int64_t)((uint32_t)(p - b) / a.num_neg); // :40 / :122 i
                    cols[rank] = (int64_t)ids[p];                          //            j
                    ++rank;
                }
            }
            if (tid == 0) a.counts[call * n_out + a.n_types + r] = (int64_t)n_edges;
        }
        if (tid == 0) a.panic[call] = s_panic;
    }
}

// ---- host side: what a problem needs, which form it takes ---------------------------------------------------------------
struct NegbPlan {
    int64_t m, max_in;            // items of a call, the longest input list
    int64_t cap_edges[NEG_MAX_RELS];
    int fits32;                   // ids, item counts and type count allow the fused kernel
    int64_t table_cap, lds_bytes; // of the fused kernel (0 where fits32 is 0)
    int threads;
};

inline bool negb_mul(int64_t a, int64_t b, int64_t *out) { return !__builtin_mul_overflow(a, b, out); }

// argument checks shared by every batched entry point; fills the plan and the per-type node capacities
static int negb_plan(const tg_neg_problem *pb, const char *who, NegbPlan &pl, std::vector<int64_t> &cap_nodes) {
    TG_REQUIRE(pb, "%s: null problem", who);
    TG_REQUIRE(pb->n_types >= 1, "%s: n_types = %d, at least 1 expected", who, pb->n_types);
    TG_REQUIRE(pb->n_rels >= 1 && pb->n_rels <= NEG_MAX_RELS, "%s: n_rels = %d relations outside [1, %d]", who, pb->n_rels,
               NEG_MAX_RELS);
    TG_REQUIRE(pb->num_neg >= 0, "%s: num_neg = %lld is negative", who, (long long)pb->num_neg);
    TG_REQUIRE(pb->try_count >= 0, "%s: try_count = %lld is negative", who, (long long)pb->try_count);
    TG_REQUIRE(pb->rel_src && pb->rel_dst && pb->graphs && pb->node_count && pb->n_inputs, "%s: null problem array", who);
    TG_REQUIRE(!pb->homogeneous || (pb->n_types == 1 && pb->n_rels == 1), "%s: homogeneous with n_types = %d, n_rels = %d", who,
               pb->n_types, pb->n_rels);
    for (int r = 0; r < pb->n_rels; ++r) {
        TG_REQUIRE(pb->rel_src[r] >= 0 && pb->rel_src[r] < pb->n_types && pb->rel_dst[r] >= 0 && pb->rel_dst[r] < pb->n_types,
                   "%s: rel_src / rel_dst of relation %d outside [0, n_types)", who, r);
        TG_REQUIRE(pb->node_count[r] >= 1, "%s: node_count of relation %d is an empty node range", who, r);
    }
    pl.m = 0, pl.max_in = 0;
    for (int t = 0; t < pb->n_types; ++t) {
        const int64_t n = pb->n_inputs[t] > 0 ? pb->n_inputs[t] : 0;
        int64_t items = 0;
        TG_REQUIRE(negb_mul(n, pb->num_neg, &items) && !__builtin_add_overflow(pl.m, items, &pl.m) && pl.m < ((int64_t)1 << 60),
                   "%s: n_inputs x num_neg overflows", who);
        if (n > pl.max_in) pl.max_in = n;
        if (items == 0) continue;
        bool has_rel = false;
        for (int r = 0; r < pb->n_rels; ++r) has_rel |= pb->rel_src[r] == t;
        TG_REQUIRE(has_rel, "%s: n_inputs: node type %d has inputs but no outgoing relation (the reference panics)", who, t);
    }
    cap_nodes.assign((size_t)pb->n_types, 0);
    for (int t = 0; t < pb->n_types; ++t) cap_nodes[t] = (pb->n_inputs[t] > 0 ? pb->n_inputs[t] : 0) + pl.m;
    for (int r = 0; r < pb->n_rels; ++r) {
        const int64_t n = pb->n_inputs[pb->rel_src[r]];
        pl.cap_edges[r] = (n > 0 ? n : 0) * pb->num_neg;
    }
    // the fused kernel: 32-bit ids, positions below 2^31, a bounded type count, a thread's run of items in one mask
    pl.fits32 = pb->n_types <= NEGB_MAX_TYPES && pl.m + pl.max_in < ((int64_t)1 << 30) &&
                pl.m <= (int64_t)NEGB_THREADS * NEGB_MAX_PER_THREAD;
    for (int r = 0; r < pb->n_rels && pl.fits32; ++r)
        pl.fits32 = pb->node_count[r] < ((int64_t)1 << 32) && pb->graphs[r].n_major < ((int64_t)1 << 32);
    pl.table_cap = 0, pl.lds_bytes = 0, pl.threads = NEGB_THREADS;
    if (pl.fits32) {
        pl.table_cap = pow2_at_least((4 * (pl.m + pl.max_in) + 2) / 3);
        pl.lds_bytes = 8 * pl.table_cap + 8 * pl.m + ((pl.m + 15) & ~(int64_t)15) + NEGB_STATIC_LDS;
        const int64_t widest = pl.m > pl.max_in ? pl.m : pl.max_in;
        pl.threads = widest >= NEGB_THREADS ? NEGB_THREADS : (int)(widest < 64 ? 64 : (widest + 63) & ~(int64_t)63);
    }
    return TG_OK;
}

// LDS a workgroup may ask for on the current device (0: no device)
static int64_t negb_device_lds_limit() {
    static std::atomic<int64_t> cached[64]; // zero-initialised; a race only repeats the query
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 64 && cached[dev] > 0) return cached[dev];
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (dev >= 0 && dev < 64) cached[dev] = v;
    return v;
}
static inline bool negb_fused(const NegbPlan &pl, int64_t lds_limit) { return pl.fits32 && pl.lds_bytes <= lds_limit; }

} // namespace tg

extern "C" int tg_neg_batched_capacity(const tg_neg_problem *pb, int64_t *cap_nodes, int64_t *cap_edges) {
    using namespace tg;
    const char *who = "tg_neg_batched_capacity";
    TG_REQUIRE(cap_nodes && cap_edges, "%s: null output", who);
    NegbPlan pl;
    std::vector<int64_t> cn;
    if (const int rc = negb_plan(pb, who, pl, cn)) return rc;
    for (int t = 0; t < pb->n_types; ++t) cap_nodes[t] = cn[t];
    for (int r = 0; r < pb->n_rels; ++r) cap_edges[r] = pl.cap_edges[r];
    return TG_OK;
}

extern "C" int tg_neg_batched_form(const tg_neg_problem *pb, int64_t lds_limit_bytes, int32_t *form, int64_t *lds_bytes) {
    using namespace tg;
    const char *who = "tg_neg_batched_form";
    TG_REQUIRE(form && lds_bytes, "%s: null output", who);
    NegbPlan pl;
    std::vector<int64_t> cn;
    if (const int rc = negb_plan(pb, who, pl, cn)) return rc;
    const int64_t limit = lds_limit_bytes > 0 ? lds_limit_bytes : negb_device_lds_limit();
    *form = negb_fused(pl, limit) ? 1 : 0;
    *lds_bytes = pl.lds_bytes;
    return TG_OK;
}

extern "C" int tg_neg_batched_workspace_bytes(const tg_neg_problem *pb, int64_t n_calls, int64_t *bytes) {
    using namespace tg;
    const char *who = "tg_neg_batched_workspace_bytes";
    TG_REQUIRE(bytes, "%s: null output", who);
    TG_REQUIRE(n_calls >= 1 && n_calls <= TG_NEG_MAX_CALLS, "%s: n_calls = %lld outside [1, %d]", who, (long long)n_calls,
               TG_NEG_MAX_CALLS);
    NegbPlan pl;
    std::vector<int64_t> cn;
    if (const int rc = negb_plan(pb, who, pl, cn)) return rc;
    if (negb_fused(pl, negb_device_lds_limit())) {
        *bytes = 0;
        return TG_OK;
    }
    return tg_neg_workspace_bytes(pb, bytes); // the calls run one after the other in the first region
}

extern "C" int tg_neg_sample_batched(const tg_neg_problem *pb, int64_t n_calls, const tg_rng *rng, const tg_neg_batched_out *out,
                                     void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_neg_sample_batched";
    TG_REQUIRE(rng && out, "%s: null argument", who);
    TG_REQUIRE(n_calls >= 1 && n_calls <= TG_NEG_MAX_CALLS, "%s: n_calls = %lld outside [1, %d]", who, (long long)n_calls,
               TG_NEG_MAX_CALLS);
    NegbPlan pl;
    std::vector<int64_t> cn;
    if (const int rc = negb_plan(pb, who, pl, cn)) return rc;
    const int T = pb->n_types, R = pb->n_rels;
    TG_REQUIRE(out->samples && out->pitch_nodes && out->rows && out->cols && out->pitch_edges, "%s: null output array", who);
    for (int t = 0; t < T; ++t)
        TG_REQUIRE(out->pitch_nodes[t] >= cn[t], "%s: samples slabs of type %d too small (pitch_nodes %lld < %lld)", who, t,
                   (long long)out->pitch_nodes[t], (long long)cn[t]);
    for (int r = 0; r < R; ++r)
        TG_REQUIRE(out->pitch_edges[r] >= pl.cap_edges[r], "%s: edge slabs of relation %d too small (pitch_edges %lld < %lld)", who,
                   r, (long long)out->pitch_edges[r], (long long)pl.cap_edges[r]);
    const bool fused = negb_fused(pl, negb_device_lds_limit());
    int64_t need = 0;
    if (!fused)
        if (const int rc = tg_neg_workspace_bytes(pb, &need)) return rc;
    TG_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "%s: workspace too small (%lld < %lld)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    // device pointers
    TG_REQUIRE(out->counts && out->panic, "%s: null counts / panic", who);
    TG_REQUIRE(((uintptr_t)out->counts & 7u) == 0 && ((uintptr_t)workspace & 7u) == 0,
               "%s: workspace and counts must be 8-byte aligned", who);
    TG_REQUIRE(pb->inputs, "%s: null inputs array", who);
    for (int t = 0; t < T; ++t) {
        TG_REQUIRE(pb->n_inputs[t] <= 0 || pb->inputs[t], "%s: null inputs slab of type %d", who, t);
        TG_REQUIRE(cn[t] == 0 || out->samples[t], "%s: null samples slab of type %d", who, t);
    }
    for (int r = 0; r < R; ++r) {
        TG_REQUIRE(pb->graphs[r].ptrs, "%s: relation %d has no CSR", who, r);
        TG_REQUIRE(pl.cap_edges[r] == 0 || (out->rows[r] && out->cols[r]), "%s: null edge slab of relation %d", who, r);
    }
    hipStream_t stream = (hipStream_t)stream_;

    if (!fused) { // the existing kernels, call by call, each into its own rows
        std::vector<const int64_t *> ins((size_t)T);
        std::vector<int64_t *> s((size_t)T), rw((size_t)R), cl((size_t)R);
        tg_neg_problem one = *pb;
        one.inputs = ins.data();
        for (int64_t b = 0; b < n_calls; ++b) {
            for (int t = 0; t < T; ++t) {
                ins[t] = pb->n_inputs[t] > 0 ? pb->inputs[t] + b * pb->n_inputs[t] : nullptr;
                s[t] = out->samples[t] ? out->samples[t] + b * out->pitch_nodes[t] : nullptr;
            }
            for (int r = 0; r < R; ++r) {
                rw[r] = out->rows[r] ? out->rows[r] + b * out->pitch_edges[r] : nullptr;
                cl[r] = out->cols[r] ? out->cols[r] + b * out->pitch_edges[r] : nullptr;
            }
            tg_neg_out o{};
            o.samples = s.data(), o.rows = rw.data(), o.cols = cl.data();
            o.n_samples = out->counts + b * (T + R), o.n_edges = o.n_samples + T, o.panic = out->panic + b;
            const tg_rng one_rng{rng->seed, rng->call_id + (uint64_t)b};
            if (const int rc = tg_neg_sample(&one, &one_rng, &o, workspace, stream_)) return rc;
        }
        return TG_OK;
    }

    NegbArgs a{};
    int n_src = 0;
    for (int t = 0; t < T; ++t) {
        a.src_begin[t] = n_src;
        for (int r = 0; r < R; ++r)
            if (pb->rel_src[r] == t) a.src_rels[n_src++] = r; // negative_sampling.rs:65-71
        const int64_t n = pb->n_inputs[t] > 0 ? pb->n_inputs[t] : 0;
        a.inputs[t] = n > 0 ? pb->inputs[t] : nullptr;
        a.samples[t] = out->samples[t];
        a.node_pitch[t] = out->pitch_nodes[t];
        a.n_in[t] = (int32_t)n;
        a.item_begin[t + 1] = a.item_begin[t] + (int32_t)(n * pb->num_neg);
    }
    a.src_begin[T] = n_src;
    for (int r = 0; r < R; ++r) {
        a.tab.r[r] = NegRel{pb->graphs[r].ptrs, pb->graphs[r].indices, pb->node_count[r], pb->graphs[r].n_major, pb->rel_dst[r], 0};
        a.rows[r] = out->rows[r], a.cols[r] = out->cols[r], a.edge_pitch[r] = out->pitch_edges[r];
        a.rel_src[r] = pb->rel_src[r];
        a.dst_mask |= 1u << pb->rel_dst[r];
    }
    a.n_types = T, a.n_rels = R, a.hetero = pb->homogeneous ? 0 : 1, a.inbound = pb->inbound;
    a.num_neg = (uint32_t)(pb->num_neg < 0x7FFFFFFF ? (pb->num_neg > 0 ? pb->num_neg : 1) : 0x7FFFFFFF);
    a.try_count = pb->try_count;
    a.seed = rng->seed, a.call_id = rng->call_id;
    a.counts = out->counts, a.panic = out->panic, a.n_calls = (int32_t)n_calls;
    a.cap_mask = (uint32_t)(pl.table_cap - 1);
    a.hash_shift = 32u - (uint32_t)__builtin_ctzll((unsigned long long)pl.table_cap);
    const int64_t dyn = pl.lds_bytes - NEGB_STATIC_LDS;
    if (dyn > 64 * 1024) { // above the default limit of a launch: raise it once per device (the plan keeps it below the device's)
        static std::atomic<int64_t> raised[64]; // zero-initialised; a race only sets the attribute twice
        int dev = 0;
        TG_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || raised[dev] < dyn) {
            TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(neg_batched_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)dyn));
            if (dev >= 0 && dev < 64) raised[dev] = dyn;
        }
    }
    const unsigned grid = (unsigned)(n_calls < 16384 ? n_calls : 16384);
    hipLaunchKernelGGL(neg_batched_kernel, dim3(grid), dim3(pl.threads), (size_t)dyn, stream, a, (int)pl.m);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
