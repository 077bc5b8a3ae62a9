// The device code and the plan that seal.hip (tg_seal_nodes) and seal_capped.hip (tg_seal_nodes_capped) share: the table, the
// flat dealing, the claiming hop, the restricted rounds, the sort, the output and the cleanup of one slot.
// seal_slots is the body of both kernels; what differs between them is a HOPS policy:
//   capped            compile-time: false leaves every hop the claiming hop below and the policy unused
//   begin(i)          a slot that passed the range checks starts
//   cap(hop)          > 0: the hop is run by run_hop, which claims into the table what it keeps and ends behind a barrier
//   refused(i), done(i)   the slot's words beyond tg_seal_out
#pragma once
#include <algorithm>

#include "rw_walk.h"

#include "../../include/tchgeo_seal.h"

namespace tg {

constexpr uint32_t SEAL_EMPTY = 0xFFFFFFFFu; // ids are < 2^31; also "no place" and "no distance"
constexpr int SEAL_THREADS = 256;
constexpr int SEAL_WAVES = SEAL_THREADS / 64;
constexpr int SEAL_LOG_T_SMALL = 10, SEAL_LOG_T_LARGE = 12; // the LDS form's tables

struct SealParams {
    CsrView g;
    int64_t n_major;
    const int64_t *src, *dst;
    int64_t m, z_max;
    int32_t num_hops, node_cap, log_t;
    int64_t *count, *nodes, *z, *du, *dv, *rounds;
    int32_t *status;
    unsigned char *ws; // workspace form: a table per workgroup
    int64_t ws_group_bytes;
};

struct SealTable {
    uint32_t *key, *du, *dv, *queue, *marks, *list;
    uint32_t mask;
    int shift;
    __device__ __forceinline__ uint32_t home(uint32_t id) const { return (id * 0x9E3779B1u) >> shift; }
};

// the tile of the flat dealing: rows with entries, compacted
struct SealDeal {
    uint64_t row[SEAL_THREADS]; // where the row begins,
    uint64_t pre[SEAL_THREADS]; // the entries of the tile before it,
    uint32_t aux[SEAL_THREADS]; // what every entry of it carries
    uint64_t wave_d[SEAL_WAVES];
    uint32_t wave_n[SEAL_WAVES];
};

// a workgroup's static LDS: the deal queue and the slot's counters
struct SealShared {
    SealDeal q;
    uint32_t claimed, over, queued;
};

__host__ __device__ inline int64_t seal_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// a word that atomics write (key, marks).  In the workspace they are performed in L2, so the load has to pass the CU's L1
// as well: agent scope; in LDS any scope does
template <bool LDS> __device__ __forceinline__ uint32_t seal_load(const uint32_t *w) {
    return LDS ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a vertex met for the first time claims a place and a list position
template <bool LDS>
__device__ __forceinline__ void seal_claim(const SealTable &t, uint32_t id, uint32_t cap, uint32_t *n_claimed, uint32_t *over) {
    if (__hip_atomic_load(over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // the slot is refused already
    uint32_t h = t.home(id);
    // at most cap + 256 places are ever claimed (a claim past cap stops every later one) and T >= cap + 512
    for (uint32_t step = 0; step <= t.mask; ++step, h = (h + 1) & t.mask) {
        uint32_t cur = seal_load<LDS>(&t.key[h]);
        if (cur == SEAL_EMPTY) {
            cur = atomicCAS(&t.key[h], SEAL_EMPTY, id);
            if (cur == SEAL_EMPTY) {
                const uint32_t at = atomicAdd(n_claimed, 1u);
                if (at < cap) t.list[at] = h;
                else __hip_atomic_store(over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                return;
            }
        }
        if (cur == id) return;
    }
}

// the place of a vertex of N, SEAL_EMPTY for any other: the restricted searches claim nothing
template <bool LDS> __device__ __forceinline__ uint32_t seal_find(const SealTable &t, uint32_t id) {
    uint32_t h = t.home(id);
    for (uint32_t step = 0; step <= t.mask; ++step, h = (h + 1) & t.mask) {
        const uint32_t cur = seal_load<LDS>(&t.key[h]);
        if (cur == id) return h;
        if (cur == SEAL_EMPTY) break;
    }
    return SEAL_EMPTY;
}

// One tile: `vertex` (where `has`) of every thread, its entries dealt out flat; visit(target, aux of the row).  Every
// thread of the workgroup calls it; it ends behind a barrier, so every visit of the tile is made when it returns.
template <class Visit>
__device__ __forceinline__ void seal_deal(const CsrView &g, SealDeal &q, bool has, int64_t vertex, uint32_t aux, Visit visit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t b = 0;
    uint64_t d = 0;
    if (has) {
        b = g.ptr(vertex);
        const int64_t e = g.ptr(vertex + 1);
        if (e > b) d = (uint64_t)(e - b);
    }
    const bool act = d > 0;
    const uint64_t ballot = __ballot(act);
    const uint64_t incl = wave_inclusive_scan<uint64_t>(d);
    if (lane == 63) q.wave_d[wave] = incl;
    if (lane == 0) q.wave_n[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t n_before = 0, n_rows = 0;
    uint64_t d_before = 0, n_ent = 0;
#pragma unroll
    for (int w = 0; w < SEAL_WAVES; ++w) {
        const uint32_t nw = q.wave_n[w];
        const uint64_t dw = q.wave_d[w];
        if (w < wave) n_before += nw, d_before += dw;
        n_rows += nw, n_ent += dw;
    }
    if (act) {
        const uint32_t j = n_before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        q.row[j] = (uint64_t)b;
        q.pre[j] = d_before + incl - d;
        q.aux[j] = aux;
    }
    __syncthreads();
    uint32_t row = 0;
    for (uint64_t e = (uint64_t)tid; e < n_ent; e += SEAL_THREADS) {
        if (row + 1 < n_rows && e >= q.pre[row + 1]) { // not the row of the entry before: the last row with pre <= e
            uint32_t lo = row + 1, hi = n_rows - 1;     // (every queued row has entries)
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (q.pre[mid] <= e) lo = mid;
                else hi = mid - 1;
            }
            row = lo;
        }
        visit((uint32_t)g.idx((int64_t)(q.row[row] + (e - q.pre[row]))), q.aux[row]);
    }
    __syncthreads(); // the queue is free again and every visit is made
}

// tg_seal_nodes' hops: every hop claims all it meets
struct SealEveryHop {
    static constexpr bool capped = false;
    __device__ __forceinline__ void begin(int64_t) {}
    __device__ __forceinline__ uint32_t cap(int) const { return 0; }
    template <bool LDS>
    __device__ __forceinline__ void run_hop(const SealParams &, SealShared &, const SealTable &, uint32_t, uint32_t, int) {}
    __device__ __forceinline__ void refused(int64_t) const {}
    __device__ __forceinline__ void done(int64_t) const {}
};

// the slots of one workgroup, each from its first hop to its rows of output; `dyn` is the workgroup's dynamic LDS
template <bool LDS, class Hops>
__device__ __forceinline__ void seal_slots(const SealParams &P, SealShared &s, unsigned char *dyn, Hops &hops) {
    SealDeal &q = s.q;
    const int tid = threadIdx.x;
    const uint32_t T = 1u << P.log_t, cap = (uint32_t)P.node_cap;
    unsigned char *base = LDS ? dyn : P.ws + (int64_t)blockIdx.x * P.ws_group_bytes;
    SealTable t;
    t.key = reinterpret_cast<uint32_t *>(base);
    t.du = t.key + T;
    t.dv = t.du + T;
    t.queue = t.dv + T;
    t.marks = t.queue + T;
    t.list = t.marks + (T >> 4);
    t.mask = T - 1;
    t.shift = 32 - P.log_t;
    uint64_t *srt = reinterpret_cast<uint64_t *>(t.queue); // the sort's words lie over the queue once the rounds are over

    for (uint32_t j = tid; j < T; j += SEAL_THREADS) t.key[j] = t.du[j] = t.dv[j] = SEAL_EMPTY;
    for (uint32_t j = tid; j < (T >> 4); j += SEAL_THREADS) t.marks[j] = 0;

    for (int64_t i = blockIdx.x; i < P.m; i += gridDim.x) { // block-uniform: every thread meets every barrier
        const int64_t u = P.src[i], v = P.dst[i];
        const bool outside = (uint64_t)u >= (uint64_t)P.n_major || (uint64_t)v >= (uint64_t)P.n_major;
        if (outside || u == v) { // never indexes ptrs
            if (tid == 0) {
                P.count[i] = 0;
                atomicOr(P.status, outside ? TG_SEAL_STATUS_RANGE : TG_SEAL_STATUS_SAME);
                hops.refused(i);
            }
            continue;
        }
        const uint32_t ku = (uint32_t)u, kv = (uint32_t)v;
        __syncthreads(); // the table is clean, the slot before has read its counters
        if (tid == 0) {
            const uint32_t hu = t.home(ku);
            uint32_t hv = t.home(kv);
            if (hv == hu) hv = (hv + 1) & t.mask;
            t.key[hu] = ku, t.key[hv] = kv;
            t.du[hu] = 0, t.dv[hv] = 0;
            t.list[0] = hu, t.list[1] = hv;
            t.queue[0] = (hu << 2) | 1u, t.queue[1] = (hv << 2) | 2u;
            s.claimed = s.queued = 2;
            s.over = 0;
        }
        hops.begin(i);
        __syncthreads();

        // ---- N: h hops from {u, v}; hop t's frontier is what hop t - 1 appended to the list
        uint32_t f0 = 0, f1 = 2, over = 0;
        for (int hop = 0; hop < P.num_hops; ++hop) {
            if (Hops::capped && hops.cap(hop) > 0) {
                hops.template run_hop<LDS>(P, s, t, f0, f1, hop);
            } else {
                for (uint32_t tile = f0; tile < f1; tile += SEAL_THREADS) {
                    const uint32_t at = tile + tid;
                    const bool has = at < f1;
                    const int64_t x = has ? (int64_t)seal_load<LDS>(&t.key[t.list[at]]) : 0;
                    seal_deal(P.g, q, has, x, 0u,
                              [&](uint32_t y, uint32_t) { seal_claim<LDS>(t, y, cap, &s.claimed, &s.over); });
                }
            }
            over = s.over; // behind the hop's last barrier: every claim of the hop is made
            if (over) break;
            f0 = f1;
            f1 = s.claimed; // <= cap; the next claim is two barriers away
            if (f0 == f1) break;
        }
        if (over) { // refused: count and status only; places past the list may be claimed, so the whole table is reset
            if (tid == 0) {
                P.count[i] = 0;
                atomicOr(P.status, TG_SEAL_STATUS_CAP);
                hops.refused(i);
            }
            for (uint32_t j = tid; j < T; j += SEAL_THREADS) t.key[j] = t.du[j] = t.dv[j] = SEAL_EMPTY;
            continue;
        }
        const uint32_t n = s.claimed;

        // ---- du and dv: synchronous rounds over N that only look up
        uint32_t q0 = 0, q1 = 2, rounds = 0;
        for (;;) {
            for (uint32_t tile = q0; tile < q1; tile += SEAL_THREADS) {
                const uint32_t at = tile + tid;
                const bool has = at < q1;
                const uint32_t ent = has ? t.queue[at] : 0u;
                const int64_t x = has ? (int64_t)seal_load<LDS>(&t.key[ent >> 2]) : 0;
                seal_deal(P.g, q, has, x, ent & 3u, [&](uint32_t y, uint32_t waves) {
                    if (y == kv) waves &= ~1u; // u's wave never enters v,
                    if (y == ku) waves &= ~2u; // v's never u
                    if (!waves) return;
                    const uint32_t p = seal_find<LDS>(t, y);
                    if (p == SEAL_EMPTY) return; // outside N
                    if ((waves & 1u) && t.du[p] != SEAL_EMPTY) waves &= ~1u;
                    if ((waves & 2u) && t.dv[p] != SEAL_EMPTY) waves &= ~2u;
                    if (!waves) return;
                    const uint32_t sh = 2u * (p & 15u);
                    const uint32_t old = atomicOr(&t.marks[p >> 4], waves << sh);
                    if (((old >> sh) & 3u) == 0) t.queue[atomicAdd(&s.queued, 1u)] = p; // the place's first mark of the round
                });
            }
            const uint32_t q2 = s.queued; // behind the deal's barrier
            if (q2 == q1) break;
            ++rounds;
            for (uint32_t at = q1 + tid; at < q2; at += SEAL_THREADS) { // the round's marks become distances
                const uint32_t p = t.queue[at], sh = 2u * (p & 15u);
                const uint32_t waves = (seal_load<LDS>(&t.marks[p >> 4]) >> sh) & 3u;
                if (waves & 1u) t.du[p] = rounds;
                if (waves & 2u) t.dv[p] = rounds;
                atomicAnd(&t.marks[p >> 4], ~(3u << sh));
                t.queue[at] = (p << 2) | waves;
            }
            __syncthreads();
            q0 = q1;
            q1 = q2;
        }

        // ---- the others by id ascending; the queue is dead
        const uint32_t others = n - 2;
        uint32_t P2 = 1;
        while (P2 < others) P2 <<= 1; // others <= cap <= T / 2: the words fit
        for (uint32_t j = tid; j < P2; j += SEAL_THREADS) {
            uint64_t w = ~0ull;
            if (j < others) {
                const uint32_t p = t.list[j + 2];
                w = ((uint64_t)seal_load<LDS>(&t.key[p]) << 32) | (uint64_t)p;
            }
            srt[j] = w;
        }
        for (uint32_t size = 2; size <= P2; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (uint32_t x = tid; x < (P2 >> 1); x += SEAL_THREADS) {
                    const uint32_t lo = 2 * x - (x & (stride - 1)), hi = lo + stride;
                    const uint64_t a = srt[lo], c = srt[hi];
                    if ((a > c) == ((lo & size) == 0)) {
                        srt[lo] = c;
                        srt[hi] = a;
                    }
                }
            }
        __syncthreads();
        const int64_t row = i * (int64_t)P.node_cap;
        for (uint32_t j = tid; j < n; j += SEAL_THREADS) {
            const uint32_t p = j < 2 ? t.list[j] : (uint32_t)srt[j - 2];
            const int64_t id = j == 0 ? u : j == 1 ? v : (int64_t)(srt[j - 2] >> 32);
            const uint32_t a = t.du[p], b = t.dv[p];
            int64_t z = 1;
            if (j >= 2) {
                z = 0;
                if (a != SEAL_EMPTY && b != SEAL_EMPTY) {
                    const int64_t d = (int64_t)a + (int64_t)b, half = d >> 1;
                    z = 1 + (int64_t)min(a, b) + half * (half + (d & 1) - 1);
                }
            }
            if (P.z_max > 0 && z > P.z_max) z = P.z_max;
            P.nodes[row + j] = id;
            P.z[row + j] = z;
            if (P.du) P.du[row + j] = a == SEAL_EMPTY ? -1 : (int64_t)a;
            if (P.dv) P.dv[row + j] = b == SEAL_EMPTY ? -1 : (int64_t)b;
        }
        if (tid == 0) {
            P.count[i] = n;
            if (P.rounds) P.rounds[i] = rounds;
            hops.done(i);
        }
        __syncthreads(); // the output has read the table
        for (uint32_t at = tid; at < n; at += SEAL_THREADS) {
            const uint32_t p = t.list[at];
            t.key[p] = t.du[p] = t.dv[p] = SEAL_EMPTY;
        }
    }
}

// the table of a cap, the form a call takes and the bytes of one workgroup's part of the workspace
struct SealPlan {
    int32_t form, log_t;
    int64_t group_bytes, groups, lds_bytes;
};

static int seal_plan(int64_t m, int32_t node_cap, int32_t form, SealPlan *pl, const char *who) {
    TG_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "%s: m = %lld outside [0, 2^31)", who, (long long)m);
    TG_REQUIRE(node_cap >= 2 && node_cap <= TG_SEAL_MAX_CAP, "%s: node_cap = %d outside [2, 2^20]", who, node_cap);
    TG_REQUIRE(form >= TG_SEAL_FORM_AUTO && form <= TG_SEAL_FORM_WORKSPACE, "%s: unknown form %d", who, form);
    TG_REQUIRE(form != TG_SEAL_FORM_LDS || node_cap <= TG_SEAL_LDS_CAP, "%s: node_cap = %d exceeds the LDS form's %d", who,
               node_cap, TG_SEAL_LDS_CAP);
    pl->form = form != TG_SEAL_FORM_AUTO ? form : (node_cap <= TG_SEAL_LDS_CAP ? TG_SEAL_FORM_LDS : TG_SEAL_FORM_WORKSPACE);
    if (pl->form == TG_SEAL_FORM_LDS) {
        pl->log_t = node_cap <= TG_SEAL_LDS_CAP_SMALL ? SEAL_LOG_T_SMALL : SEAL_LOG_T_LARGE;
        pl->lds_bytes = ((int64_t)18 << pl->log_t) + ((int64_t)1 << (pl->log_t - 2)); // four arrays, marks, a list of T / 2
        pl->group_bytes = 0;
        pl->groups = 0;
    } else {
        pl->log_t = 10;
        while (((int64_t)1 << pl->log_t) < 2 * (int64_t)node_cap) ++pl->log_t;
        pl->lds_bytes = 0;
        pl->group_bytes = ((int64_t)16 << pl->log_t) + ((int64_t)1 << (pl->log_t - 2)) + seal_r256(4 * (int64_t)node_cap);
        pl->groups = std::min<int64_t>(m, TG_SEAL_WS_GROUPS);
    }
    return TG_OK;
}

// what tg_seal_nodes refuses behind its plan, and its kernel's arguments
static int seal_params(const tg_graph *g, const tg_seal_in *in, const tg_seal_out *out, int64_t m, const SealPlan &pl,
                       int32_t *status, void *workspace, int64_t workspace_bytes, SealParams *p, bool *launch, const char *who) {
    *launch = false;
    TG_REQUIRE(in->num_hops >= 1 && in->num_hops <= TG_SEAL_MAX_HOPS, "%s: num_hops = %d outside [1, %d]", who, in->num_hops,
               TG_SEAL_MAX_HOPS);
    TG_REQUIRE(in->z_max >= 0, "%s: z_max = %lld is negative", who, (long long)in->z_max);
    TG_REQUIRE(g->n_major >= 0 && g->n_edges >= 0, "%s: negative graph size", who);
    if (g->n_major > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: %lld vertices do not fit the table's 32-bit keys", who, (long long)g->n_major);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    if (m == 0) return TG_OK; // nothing to launch
    TG_REQUIRE(g->ptrs && (g->indices || g->n_edges == 0), "%s: null graph arrays", who);
    TG_REQUIRE(in->src && in->dst && out->count && out->nodes && out->z && status,
               "%s: null src / dst / count / nodes / z / status", who);
    const int64_t need = pl.groups * pl.group_bytes;
    TG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: the workspace has %lld bytes, the call needs %lld", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(need == 0 || ((uintptr_t)workspace & 7u) == 0, "%s: the workspace must be 8-byte aligned", who);

    p->g = CsrView{g->ptrs, g->indices, g->ptrs32, g->indices32, nullptr, 0};
    p->n_major = g->n_major;
    p->src = in->src, p->dst = in->dst, p->m = m, p->z_max = in->z_max;
    p->num_hops = in->num_hops, p->node_cap = in->node_cap, p->log_t = pl.log_t;
    p->count = out->count, p->nodes = out->nodes, p->z = out->z, p->du = out->du, p->dv = out->dv, p->rounds = out->rounds;
    p->status = status;
    p->ws = static_cast<unsigned char *>(workspace), p->ws_group_bytes = pl.group_bytes;
    *launch = true;
    return TG_OK;
}

} // namespace tg
