// Approximate personalised PageRank by forward push, top-k per seed (tg_ppr_topk; the rule and its two proofs in
// include/tchgeo_ppr.h).  Integer end to end: mass in units of 2^-31, every add commutes.
//   One workgroup of 256 threads owns one slot from its first round to its row of output; the rounds are its barriers.
//   table    open addressing over T places (a power of two >= max(1024, 2 * node_cap)): key / p / r / incoming-r as four
//            u32 arrays, and the LIST of claimed places in claim order (node_cap words).  A claim is a compare-and-swap on
//            the key; the claimer takes the next list position from a counter, and that counter passing node_cap is the
//            overflow.  One kernel template over where the table lives: LDS (ds atomics; T = 1024 or 4096) or the caller's
//            workspace (global atomics; words they write are read at agent scope, past the CU's L1; any T up to 2^21).
//   round    the list as it stood when the round began, 256 places at a time: a thread decides its vertex (reads r, takes
//            a into p and a + q d out of r: only the owner touches p and r in a round), a ballot scan compacts the active
//            ones into an LDS queue of {row begin, q, exclusive prefix of the degrees} (DPP scan, four wave totals), and the
//            tile's entries are dealt out FLAT: thread t takes entries t, t + 256, ... of the concatenated rows, finds its
//            row by a search of the prefix (the row of the entry before is tried first: a hub row is found once),
//            and adds q to incoming-r of the target.  Consecutive lanes read consecutive `indices` words.  The sum of the
//            active degrees of a round is at most sum q d <= sum r <= 2^31, so the prefix is a u32.  Behind the last
//            tile incoming-r is folded into r over the list: that is what makes the round synchronous.
//   select   key (U - p) << 31 | id orders by p descending, then id ascending.  k <= 64: every wavefront keeps the running
//            top-64 of ns_topk.h over its share of the list, 64 places at a time, wavefront 0 merges the four.  Larger k:
//            the keys are compacted over the dead r / incoming-r arrays and sorted there by a bitonic network.
//   cleanup  only the listed places (and the sorted words) are reset, so a slot costs what it touched, not T.
// LDS: 18 T bytes of table and list + 4 KiB of queue + 1.6 KiB of merge and counters: 23.6 KiB at T = 1024 -- six workgroups
// fit a CU's 160 KiB -- and 77.6 KiB at T = 4096 -- two fit.  The workspace form keeps only the 5.6 KiB.
#include <algorithm>

#include "ns_topk.h"
#include "rw_walk.h"

#include "../../include/tchgeo_ppr.h"

namespace tg {

constexpr uint32_t PPR_EMPTY = 0xFFFFFFFFu; // ids are < 2^31
constexpr uint32_t PPR_U = 0x80000000u;
constexpr int PPR_THREADS = 256;
constexpr int PPR_WAVES = PPR_THREADS / 64;
constexpr int PPR_LOG_T_SMALL = 10, PPR_LOG_T_LARGE = 12; // the LDS form's tables
constexpr int32_t PPR_STATUS_CAP = 1, PPR_STATUS_RANGE = 2;

struct PprParams {
    CsrView g;
    int64_t n_major;
    const int64_t *seeds;
    int64_t m;
    uint32_t alpha_q, eps_q;
    int32_t max_rounds, k, node_cap, log_t;
    int64_t *count, *nodes, *score;
    float *weight;
    int64_t *touched, *rounds, *activations, *residual, *mass;
    int32_t *status;
    unsigned char *ws; // workspace form: a table per workgroup
    int64_t ws_group_bytes;
};

struct PprTable {
    uint32_t *key, *p, *r, *inc, *list;
    uint32_t mask;
    int shift;
    __device__ __forceinline__ uint32_t home(uint32_t id) const { return (id * 0x9E3779B1u) >> shift; }
};

__host__ __device__ inline int64_t ppr_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// a word that atomics write (key, incoming-r).  In the workspace they are performed in L2, so the load has to pass the
// CU's L1 as well: agent scope; in LDS any scope does
template <bool LDS> __device__ __forceinline__ uint32_t ppr_load(const uint32_t *w) {
    return LDS ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// q more residual for `id` in the round's incoming array; a vertex met for the first time claims a place and a list position
template <bool LDS>
__device__ __forceinline__ void ppr_deposit(const PprTable &t, uint32_t id, uint32_t q, uint32_t cap, uint32_t *n_touched,
                                            uint32_t *over) {
    if (__hip_atomic_load(over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // the slot is refused already
    uint32_t h = t.home(id);
    // at most cap + 256 places are ever claimed (a claim past cap stops every later deposit) and T >= cap + 512
    for (uint32_t step = 0; step <= t.mask; ++step, h = (h + 1) & t.mask) {
        uint32_t cur = ppr_load<LDS>(&t.key[h]);
        if (cur == PPR_EMPTY) {
            cur = atomicCAS(&t.key[h], PPR_EMPTY, id);
            if (cur == PPR_EMPTY) {
                const uint32_t at = atomicAdd(n_touched, 1u);
                if (at < cap) t.list[at] = h;
                else __hip_atomic_store(over, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                cur = id;
            }
        }
        if (cur == id) {
            atomicAdd(&t.inc[h], q);
            return;
        }
    }
}

template <bool LDS> __global__ void __launch_bounds__(PPR_THREADS) ppr_topk_kernel(const PprParams P) {
    extern __shared__ __align__(16) unsigned char ppr_lds[];
    __shared__ uint64_t q_row[PPR_THREADS];     // the queue: where the active vertex's row begins,
    __shared__ uint32_t q_q[PPR_THREADS];       // what every entry of it carries,
    __shared__ uint32_t q_pre[PPR_THREADS];     // the entries of the queue before it
    __shared__ uint64_t s_merge[(PPR_WAVES - 1) * 64];
    __shared__ uint32_t s_wave_n[PPR_WAVES], s_wave_d[PPR_WAVES];
    __shared__ uint32_t s_touched, s_over, s_active, s_sum_p, s_sum_r, s_cand;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t T = 1u << P.log_t, cap = (uint32_t)P.node_cap;
    unsigned char *base = LDS ? ppr_lds : P.ws + (int64_t)blockIdx.x * P.ws_group_bytes;
    PprTable t;
    t.key = reinterpret_cast<uint32_t *>(base);
    t.p = t.key + T;
    t.r = t.p + T;
    t.inc = t.r + T;
    t.list = t.inc + T;
    t.mask = T - 1;
    t.shift = 32 - P.log_t;
    uint64_t *srt = reinterpret_cast<uint64_t *>(t.r); // the sort's words lie over r and incoming-r once those are dead
    const uint64_t keep_q = 0x100000000ull - (uint64_t)P.alpha_q; // (1 - alpha) * 2^32
    const int64_t k = P.k;

    for (uint32_t j = tid; j < T; j += PPR_THREADS) {
        t.key[j] = PPR_EMPTY;
        t.p[j] = t.r[j] = t.inc[j] = 0;
    }

    for (int64_t i = blockIdx.x; i < P.m; i += gridDim.x) { // block-uniform: every thread meets every barrier
        const int64_t seed = P.seeds[i];
        if ((uint64_t)seed >= (uint64_t)P.n_major) { // never indexes ptrs
            if (tid == 0) {
                P.count[i] = 0;
                atomicOr(P.status, PPR_STATUS_RANGE);
            }
            continue;
        }
        __syncthreads(); // the table is clean, the slot before has read its counters
        if (tid == 0) {
            const uint32_t h = t.home((uint32_t)seed);
            t.key[h] = (uint32_t)seed;
            t.r[h] = PPR_U;
            t.list[0] = h;
            s_touched = 1;
            s_over = s_active = s_sum_p = s_sum_r = s_cand = 0;
        }
        __syncthreads();

        uint32_t rounds = 0, over = 0;
        uint64_t acts = 0;
        for (int round = 0; round < P.max_rounds; ++round) {
            const uint32_t n0 = s_touched; // <= cap: a round that passes it is the slot's last
            uint32_t mine = 0;
            for (uint32_t tile = 0; tile < n0; tile += PPR_THREADS) {
                const uint32_t at = tile + tid;
                bool act = false;
                uint32_t d32 = 0, q = 0;
                int64_t b = 0;
                if (at < n0) {
                    const uint32_t h = t.list[at], rv = t.r[h];
                    if (rv) {
                        const int64_t v = (int64_t)ppr_load<LDS>(&t.key[h]);
                        b = P.g.ptr(v);
                        const int64_t d = P.g.ptr(v + 1) - b;
                        if (d <= 0) { // a sink keeps everything it is sent
                            t.p[h] += rv;
                            t.r[h] = 0;
                            ++mine;
                        } else {
                            const uint64_t share = ((uint64_t)rv * keep_q) >> 32; // < 2^31
                            if ((uint64_t)d <= share && (uint64_t)rv >= (uint64_t)P.eps_q * (uint64_t)d) { // q >= 1; d < 2^31
                                d32 = (uint32_t)d;
                                q = (uint32_t)share / d32;
                                const uint32_t sent = q * d32; // <= share
                                const uint32_t a = (uint32_t)(((uint64_t)P.alpha_q * (uint64_t)sent) / keep_q);
                                t.p[h] += a;
                                t.r[h] = rv - a - sent;
                                act = true;
                                ++mine;
                            }
                        }
                    }
                }
                const uint64_t ballot = __ballot(act);
                const uint32_t incl = wave_inclusive_scan_u32_dpp(d32);
                if (lane == 63) s_wave_d[wave] = incl;
                if (lane == 0) s_wave_n[wave] = (uint32_t)__popcll(ballot);
                __syncthreads();
                uint32_t n_before = 0, d_before = 0, n_act = 0, n_ent = 0;
#pragma unroll
                for (int w = 0; w < PPR_WAVES; ++w) {
                    const uint32_t nw = s_wave_n[w], dw = s_wave_d[w];
                    if (w < wave) n_before += nw, d_before += dw;
                    n_act += nw, n_ent += dw;
                }
                if (act) {
                    const uint32_t j = n_before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
                    q_row[j] = (uint64_t)b;
                    q_q[j] = q;
                    q_pre[j] = d_before + incl - d32;
                }
                __syncthreads();
                uint32_t row = 0;
                for (uint32_t e = tid; e < n_ent; e += PPR_THREADS) { // the tile's entries, flat
                    if (row + 1 < n_act && e >= q_pre[row + 1]) {     // not the row of the entry before: the last row with
                        uint32_t lo = row + 1, hi = n_act - 1;        // q_pre <= e (every queued row has entries)
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi + 1) >> 1;
                            if (q_pre[mid] <= e) lo = mid;
                            else hi = mid - 1;
                        }
                        row = lo;
                    }
                    const int64_t target = P.g.idx((int64_t)q_row[row] + (int64_t)(e - q_pre[row]));
                    ppr_deposit<LDS>(t, (uint32_t)target, q_q[row], cap, &s_touched, &s_over);
                }
                __syncthreads(); // the queue is free again
            }
            if (mine) atomicAdd(&s_active, mine);
            __syncthreads(); // every deposit of the round is made
            const uint32_t n_active = s_active;
            over = s_over;
            if (over) break; // block-uniform
            const uint32_t n1 = s_touched;
            for (uint32_t at = tid; at < n1; at += PPR_THREADS) { // the round's receipts become residual
                const uint32_t h = t.list[at], x = ppr_load<LDS>(&t.inc[h]);
                if (x) {
                    t.r[h] += x;
                    t.inc[h] = 0;
                }
            }
            __syncthreads();
            if (tid == 0) s_active = 0; // behind every reader; the next add is two barriers away
            if (n_active == 0) break;
            ++rounds;
            acts += n_active;
        }

        if (over) { // refused: count and status only; places past the list may be claimed, so the whole table is reset
            if (tid == 0) {
                P.count[i] = 0;
                atomicOr(P.status, PPR_STATUS_CAP);
            }
            for (uint32_t j = tid; j < T; j += PPR_THREADS) {
                t.key[j] = PPR_EMPTY;
                t.p[j] = t.r[j] = t.inc[j] = 0;
            }
            continue;
        }

        const uint32_t n1 = s_touched;
        uint32_t sp = 0, sr = 0;
        for (uint32_t at = tid; at < n1; at += PPR_THREADS) {
            const uint32_t h = t.list[at];
            sp += t.p[h];
            sr += t.r[h];
        }
        sp = wave_sum(sp);
        sr = wave_sum(sr);
        if (lane == 0) {
            atomicAdd(&s_sum_p, sp);
            atomicAdd(&s_sum_r, sr);
        }
        __syncthreads(); // r and incoming-r are dead from here on
        if (tid == 0) {
            const uint32_t ps = t.p[t.list[0]];
            P.nodes[i * k] = seed;
            P.score[i * k] = (int64_t)ps;
            if (P.weight) P.weight[i * k] = (float)ps * 4.656612873077393e-10f; // 2^-31
            if (P.touched) P.touched[i] = n1;
            if (P.rounds) P.rounds[i] = rounds;
            if (P.activations) P.activations[i] = (int64_t)acts;
            if (P.residual) P.residual[i] = s_sum_r;
            if (P.mass) P.mass[i] = s_sum_p;
        }
        const int need = (int)min((int64_t)n1 - 1, k - 1); // rows behind the seed at most
        uint32_t sorted = 0;
        if (need <= 0) {
            if (tid == 0) P.count[i] = 1;
        } else if (k <= 64) {
            RcEntry kept{RC_NO_KEY, RC_NO_POS};
            for (uint32_t b0 = (uint32_t)wave * 64u; b0 < n1; b0 += PPR_THREADS) { // wave-uniform
                const uint32_t at = b0 + lane;
                RcEntry c{RC_NO_KEY, RC_NO_POS};
                if (at > 0 && at < n1) { // place 0 of the list is the seed
                    const uint32_t h = t.list[at], pv = t.p[h];
                    if (pv) c = RcEntry{(int64_t)(((uint64_t)(PPR_U - pv) << 31) | (uint64_t)ppr_load<LDS>(&t.key[h])), 0u};
                }
                const RcEntry kth = rc_shfl(kept, need - 1); // empty while fewer than `need` are kept
                const bool cand = c.pos != RC_NO_POS && rc_before(c, kth);
                if (__ballot(cand) == 0) continue;
                if (!cand) c = RcEntry{RC_NO_KEY, RC_NO_POS};
                c = rc_sort64(c, lane);
                kept = rc_merge_reversed(kept, rc_shfl(c, 63 - lane), lane);
            }
            if (wave > 0) s_merge[(wave - 1) * 64 + lane] = (uint64_t)kept.key;
            __syncthreads();
            if (wave == 0) {
                for (int w = 0; w < PPR_WAVES - 1; ++w) {
                    RcEntry o;
                    o.key = (int64_t)s_merge[w * 64 + 63 - lane];
                    o.pos = o.key == RC_NO_KEY ? RC_NO_POS : 0u;
                    kept = rc_merge_reversed(kept, o, lane);
                }
                const int n_kept = __popcll(__ballot(kept.pos != RC_NO_POS));
                const int cnt = min(n_kept, need);
                if (lane < cnt) {
                    const uint32_t pv = PPR_U - (uint32_t)((uint64_t)kept.key >> 31);
                    const int64_t o = i * k + 1 + lane;
                    P.nodes[o] = (int64_t)((uint64_t)kept.key & 0x7FFFFFFFull);
                    P.score[o] = (int64_t)pv;
                    if (P.weight) P.weight[o] = (float)pv * 4.656612873077393e-10f;
                }
                if (lane == 0) P.count[i] = 1 + cnt;
            }
        } else {
            for (uint32_t b0 = 0; b0 < n1; b0 += PPR_THREADS) { // every thread: the loop holds wave-wide calls
                const uint32_t at = b0 + tid;
                uint64_t key = 0;
                bool cand = false;
                if (at > 0 && at < n1) {
                    const uint32_t h = t.list[at], pv = t.p[h];
                    cand = pv != 0;
                    key = ((uint64_t)(PPR_U - pv) << 31) | (uint64_t)ppr_load<LDS>(&t.key[h]);
                }
                const uint64_t ballot = __ballot(cand);
                uint32_t first = 0;
                if (lane == 0 && ballot) first = atomicAdd(&s_cand, (uint32_t)__popcll(ballot));
                first = __shfl(first, 0, 64);
                if (cand) srt[first + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = key;
            }
            __syncthreads();
            const uint32_t n = s_cand;
            uint32_t P2 = 64;
            while (P2 < n) P2 <<= 1; // n <= cap <= T / 2: the words fit
            for (uint32_t j = n + tid; j < P2; j += PPR_THREADS) srt[j] = ~0ull;
            for (uint32_t size = 2; size <= P2; size <<= 1)
                for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                    __syncthreads();
                    for (uint32_t x = tid; x < (P2 >> 1); x += PPR_THREADS) {
                        const uint32_t lo = 2 * x - (x & (stride - 1)), hi = lo + stride;
                        const uint64_t a = srt[lo], c = srt[hi];
                        if ((a > c) == ((lo & size) == 0)) {
                            srt[lo] = c;
                            srt[hi] = a;
                        }
                    }
                }
            __syncthreads();
            const uint32_t cnt = min(n, (uint32_t)need);
            for (uint32_t j = tid; j < cnt; j += PPR_THREADS) {
                const uint64_t key = srt[j];
                const uint32_t pv = PPR_U - (uint32_t)(key >> 31);
                const int64_t o = i * k + 1 + j;
                P.nodes[o] = (int64_t)(key & 0x7FFFFFFFull);
                P.score[o] = (int64_t)pv;
                if (P.weight) P.weight[o] = (float)pv * 4.656612873077393e-10f;
            }
            if (tid == 0) P.count[i] = 1 + cnt;
            sorted = P2;
        }
        __syncthreads(); // the selection has read the table
        for (uint32_t j = tid; j < sorted; j += PPR_THREADS) srt[j] = 0;
        for (uint32_t at = tid; at < n1; at += PPR_THREADS) {
            const uint32_t h = t.list[at];
            t.key[h] = PPR_EMPTY;
            t.p[h] = t.r[h] = t.inc[h] = 0;
        }
    }
}

// the table of a cap, the form a call takes and the bytes of one workgroup's part of the workspace
struct PprPlan {
    int32_t form, log_t;
    int64_t group_bytes, groups, lds_bytes;
};

static int ppr_plan(int64_t m, int32_t k, int32_t node_cap, int32_t form, PprPlan *pl, const char *who) {
    TG_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "%s: m = %lld outside [0, 2^31)", who, (long long)m);
    TG_REQUIRE(node_cap >= 1 && node_cap <= TG_PPR_MAX_CAP, "%s: node_cap = %d outside [1, 2^20]", who, node_cap);
    TG_REQUIRE(k >= 1 && k <= node_cap, "%s: k = %d outside [1, node_cap = %d]", who, k, node_cap);
    TG_REQUIRE(form >= TG_PPR_FORM_AUTO && form <= TG_PPR_FORM_WORKSPACE, "%s: unknown form %d", who, form);
    TG_REQUIRE(form != TG_PPR_FORM_LDS || node_cap <= TG_PPR_LDS_CAP, "%s: node_cap = %d exceeds the LDS form's %d", who,
               node_cap, TG_PPR_LDS_CAP);
    pl->form = form != TG_PPR_FORM_AUTO ? form : (node_cap <= TG_PPR_LDS_CAP ? TG_PPR_FORM_LDS : TG_PPR_FORM_WORKSPACE);
    if (pl->form == TG_PPR_FORM_LDS) {
        pl->log_t = node_cap <= TG_PPR_LDS_CAP_SMALL ? PPR_LOG_T_SMALL : PPR_LOG_T_LARGE;
        pl->lds_bytes = ((int64_t)18 << pl->log_t); // four arrays and a list of T / 2 words
        pl->group_bytes = 0;
        pl->groups = 0;
    } else {
        pl->log_t = 10;
        while (((int64_t)1 << pl->log_t) < 2 * (int64_t)node_cap) ++pl->log_t;
        pl->lds_bytes = 0;
        pl->group_bytes = ((int64_t)16 << pl->log_t) + ppr_r256(4 * (int64_t)node_cap);
        pl->groups = std::min<int64_t>(m, TG_PPR_WS_GROUPS);
    }
    return TG_OK;
}

} // namespace tg

extern "C" int tg_ppr_workspace_bytes(int64_t m, int32_t k, int32_t node_cap, int32_t form, int64_t *bytes,
                                      int32_t *form_taken) {
    TG_REQUIRE(bytes, "tg_ppr_workspace_bytes: null bytes");
    tg::PprPlan pl;
    const int rc = tg::ppr_plan(m, k, node_cap, form, &pl, "tg_ppr_workspace_bytes");
    if (rc != TG_OK) return rc;
    *bytes = pl.groups * pl.group_bytes;
    if (form_taken) *form_taken = pl.form;
    return TG_OK;
}

extern "C" int tg_ppr_topk(const tg_graph *g, const tg_ppr_in *in, const tg_ppr_out *out, int64_t m, int32_t form,
                           int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_ppr_topk";
    TG_REQUIRE(g && in && out, "%s: null graph / in / out", who);
    PprPlan pl;
    const int rc = ppr_plan(m, in->k, in->node_cap, form, &pl, who);
    if (rc != TG_OK) return rc;
    TG_REQUIRE(in->alpha_q >= 1u, "%s: alpha_q = 0 outside [1, 2^32 - 1]", who);
    TG_REQUIRE(in->eps_q >= 1u && in->eps_q <= 0x80000000u, "%s: eps_q = %u outside [1, 2^31]", who, in->eps_q);
    TG_REQUIRE(in->max_rounds >= 1 && in->max_rounds <= TG_PPR_MAX_ROUNDS, "%s: max_rounds = %d outside [1, %d]", who,
               in->max_rounds, TG_PPR_MAX_ROUNDS);
    TG_REQUIRE(g->n_major >= 0 && g->n_edges >= 0, "%s: negative graph size", who);
    if (g->n_major > ((int64_t)1 << 31))
        return fail(TG_ERR_UNSUPPORTED, "%s: %lld vertices do not fit the table's 32-bit keys", who, (long long)g->n_major);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    if (m == 0) return TG_OK; // nothing to launch
    TG_REQUIRE(g->ptrs && (g->indices || g->n_edges == 0), "%s: null graph arrays", who);
    TG_REQUIRE(in->seeds && out->count && out->nodes && out->score && status, "%s: null seeds / count / nodes / score / status",
               who);
    const int64_t need = pl.groups * pl.group_bytes;
    TG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: the workspace has %lld bytes, the call needs %lld", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(need == 0 || ((uintptr_t)workspace & 7u) == 0, "%s: the workspace must be 8-byte aligned", who);

    PprParams p;
    p.g = CsrView{g->ptrs, g->indices, g->ptrs32, g->indices32, nullptr, 0};
    p.n_major = g->n_major;
    p.seeds = in->seeds, p.m = m;
    p.alpha_q = in->alpha_q, p.eps_q = in->eps_q;
    p.max_rounds = in->max_rounds, p.k = in->k, p.node_cap = in->node_cap, p.log_t = pl.log_t;
    p.count = out->count, p.nodes = out->nodes, p.score = out->score, p.weight = out->weight;
    p.touched = out->touched, p.rounds = out->rounds, p.activations = out->activations, p.residual = out->residual;
    p.mass = out->mass;
    p.status = status;
    p.ws = static_cast<unsigned char *>(workspace), p.ws_group_bytes = pl.group_bytes;
    hipStream_t stream = (hipStream_t)stream_;
    if (pl.form == TG_PPR_FORM_LDS) {
        // as many workgroups as stay resident on 256 CUs walk the slots: six per CU with the small table, two with the large
        const int64_t grid = std::min<int64_t>(m, pl.log_t == PPR_LOG_T_SMALL ? 256 * 6 : 256 * 2);
        if (pl.lds_bytes > 64 * 1024)
            TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ppr_topk_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
        hipLaunchKernelGGL(ppr_topk_kernel<true>, dim3((unsigned)grid), dim3(PPR_THREADS), (size_t)pl.lds_bytes, stream, p);
    } else {
        hipLaunchKernelGGL(ppr_topk_kernel<false>, dim3((unsigned)pl.groups), dim3(PPR_THREADS), 0, stream, p);
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}
