// SEAL enclosing subgraphs with a cap per hop (tg_seal_nodes_capped; the rule in include/tchgeo_seal_capped.h).
//   The slot loop, the table, the dealing, the rounds, the sort and the output are seal.h's; this file is the CAPPED HOP:
//   hop t keeps, of the vertices it meets for the first time, the k_t with the smallest (Philox key, id).
//   pool     the hop's candidates live in LDS in both forms, behind the table of the LDS form: TAB, open addressing over Tp
//            places of ids (Tp = TG_SEAL_POOL_PLACES(k_t)), and the candidate LIST of C = Tp / 2 {id, key} in claim order
//            with its counter.  10 Tp bytes: 10 / 20 / 40 KiB.  The main table is only read while the hop runs.
//   visit    an entry y computes key_t(y) in registers (one Philox4x32-10) and ends there when (key, y) is above the
//            threshold TAU, which starts at "everything"; else it ends when y is in the main table (seal_find); else it
//            claims a TAB place by compare-and-swap and takes a list position from the counter.
//   overflow a position >= C sets FULL and claims stop at once: at most C + 256 <= 3 Tp / 4 places are ever claimed, so TAB
//            never fills and every probe ends.  Behind the tile's barrier a full pool is COMPACTED -- the list is sorted by
//            (key, id) with a bitonic network in place, TAU becomes the k_t-th, TAB is rebuilt from the k_t survivors -- and
//            the same tile is dealt again: a survivor finds itself, a dropped vertex is above TAU, a missed one is visited.
//            Every compaction lowers TAU, so the replays end.  A replay starts at the tile's first entry: no restart offset.
//   end      a list above k_t is sorted once more (the cut bit); the survivors claim main-table places with seal_claim, so
//            node_cap's overflow is today's; TAB is cleared whole (4 to 16 stores per thread), the counter and TAU are reset:
//            a finished or refused slot leaves the pool clean.
//   A hop with k_t = 0 is seal.h's claiming hop.
#include "seal.h"

#include "../../include/tchgeo_seal_capped.h"

namespace tg {

constexpr uint32_t TAG_SEAL_HOP = TG_TAG_SEAL_HOP;

struct SealCapParams {
    uint64_t seed;
    const int64_t *call_ids;
    int64_t call_id0;
    int64_t *cut;
    int32_t log_tp_max; // the pool the launch was sized for
    int32_t pool_at;    // where the pool begins in the dynamic LDS
    uint16_t k[TG_SEAL_MAX_HOPS];
};

struct SealPoolShared {
    uint64_t tau_key;
    uint32_t tau_id, n, full;
};

__host__ __device__ inline int seal_log_tp(uint32_t k) { return k <= 256 ? 10 : k <= 512 ? 11 : 12; }

struct SealCappedHops {
    static constexpr bool capped = true;
    const SealCapParams &C;
    SealPoolShared &ps;
    uint64_t *key; // the list's keys,
    uint32_t *id;  // its ids,
    uint32_t *tab; // the places
    CallKey ck;
    uint64_t cut;

    __device__ __forceinline__ SealCappedHops(const SealCapParams &C_, SealPoolShared &ps_, unsigned char *dyn) : C(C_), ps(ps_) {
        const uint32_t c_max = 1u << (C.log_tp_max - 1);
        key = reinterpret_cast<uint64_t *>(dyn + C.pool_at);
        id = reinterpret_cast<uint32_t *>(key + c_max);
        tab = id + c_max;
        for (uint32_t j = threadIdx.x; j < 2 * c_max; j += SEAL_THREADS) tab[j] = SEAL_EMPTY;
        if (threadIdx.x == 0) reset();
    } // the slot loop's first barrier stands between this and the first hop

    __device__ __forceinline__ void reset() { ps.tau_key = ~0ull, ps.tau_id = SEAL_EMPTY, ps.n = 0, ps.full = 0; }
    __device__ __forceinline__ uint32_t cap(int hop) const { return C.k[hop]; }
    __device__ __forceinline__ void begin(int64_t i) {
        ck = call_key(C.seed, (uint64_t)(C.call_ids ? C.call_ids[i] : C.call_id0 + i), TAG_SEAL_HOP);
        cut = 0;
    }
    __device__ __forceinline__ void refused(int64_t i) const {
        if (C.cut) C.cut[i] = 0;
    }
    __device__ __forceinline__ void done(int64_t i) const {
        if (C.cut) C.cut[i] = (int64_t)cut;
    }

    // The list's first n <= C words by (key, id) ascending.  Entered and left behind a barrier by every thread.
    __device__ __forceinline__ void sort(uint32_t n) {
        uint32_t P2 = 1;
        while (P2 < n) P2 <<= 1; // <= C: both are powers of two
        for (uint32_t j = n + threadIdx.x; j < P2; j += SEAL_THREADS) key[j] = ~0ull, id[j] = SEAL_EMPTY;
        for (uint32_t size = 2; size <= P2; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (uint32_t x = threadIdx.x; x < (P2 >> 1); x += SEAL_THREADS) {
                    const uint32_t lo = 2 * x - (x & (stride - 1)), hi = lo + stride;
                    const uint64_t a = key[lo], c = key[hi];
                    const uint32_t ia = id[lo], ic = id[hi];
                    if ((a > c || (a == c && ia > ic)) == ((lo & size) == 0)) {
                        key[lo] = c, key[hi] = a;
                        id[lo] = ic, id[hi] = ia;
                    }
                }
            }
        __syncthreads();
    }

    // A full pool shrinks to its k smallest: TAU is the k-th, TAB holds the survivors alone
    __device__ __forceinline__ void compact(uint32_t k, uint32_t mask, int shift) {
        sort((mask + 1u) >> 1); // full: every one of the list's C words is written
        for (uint32_t j = threadIdx.x; j <= mask; j += SEAL_THREADS) tab[j] = SEAL_EMPTY;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < k; j += SEAL_THREADS) { // k distinct ids into more than 4 k empty places
            const uint32_t y = id[j];
            uint32_t h = (y * 0x9E3779B1u) >> shift;
            for (uint32_t step = 0; step <= mask; ++step, h = (h + 1) & mask)
                if (atomicCAS(&tab[h], SEAL_EMPTY, y) == SEAL_EMPTY) break;
        }
        if (threadIdx.x == 0) ps.tau_key = key[k - 1], ps.tau_id = id[k - 1], ps.n = k, ps.full = 0;
        __syncthreads();
    }

    template <bool LDS>
    __device__ __forceinline__ void run_hop(const SealParams &P, SealShared &s, const SealTable &t, uint32_t f0, uint32_t f1,
                                            int hop) {
        const int tid = threadIdx.x;
        const uint32_t k = C.k[hop], d0 = (uint32_t)hop + 1u;
        const int log_tp = seal_log_tp(k), shift = 32 - log_tp;
        const uint32_t mask = (1u << log_tp) - 1u, cap_p = 1u << (log_tp - 1);
        for (uint32_t tile = f0; tile < f1; tile += SEAL_THREADS) {
            const uint32_t at = tile + tid;
            const bool has = at < f1;
            const int64_t x = has ? (int64_t)seal_load<LDS>(&t.key[t.list[at]]) : 0;
            for (;;) {
                const uint64_t tau_key = ps.tau_key; // behind a barrier; nothing moves TAU while a tile is dealt
                const uint32_t tau_id = ps.tau_id;
                seal_deal(P.g, s.q, has, x, 0u, [&](uint32_t y, uint32_t) {
                    const uint64_t ky = draw(ck, (uint64_t)y, d0, 0u).a();
                    if (ky > tau_key || (ky == tau_key && y > tau_id)) return;
                    if (__hip_atomic_load(&ps.full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; // dealt again
                    if (seal_find<LDS>(t, y) != SEAL_EMPTY) return;                                           // in N_{t-1}
                    uint32_t h = (y * 0x9E3779B1u) >> shift;
                    // at most C + 256 places are ever claimed (a claim past C stops every later one) and Tp >= C + 512
                    for (uint32_t step = 0; step <= mask; ++step, h = (h + 1) & mask) {
                        uint32_t cur = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (cur == SEAL_EMPTY) {
                            cur = atomicCAS(&tab[h], SEAL_EMPTY, y);
                            if (cur == SEAL_EMPTY) {
                                const uint32_t pos = atomicAdd(&ps.n, 1u);
                                if (pos < cap_p) key[pos] = ky, id[pos] = y;
                                else __hip_atomic_store(&ps.full, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                return;
                            }
                        }
                        if (cur == y) return;
                    }
                });
                if (!ps.full) break; // behind the deal's barrier, and compact() writes it behind another
                compact(k, mask, shift);
                cut |= 1ull << hop;
            }
        }
        uint32_t n = ps.n; // <= C: the last tile left the pool not full
        if (n > k) {
            sort(n);
            cut |= 1ull << hop;
            n = k;
        }
        for (uint32_t j = tid; j < n; j += SEAL_THREADS)
            seal_claim<LDS>(t, id[j], (uint32_t)P.node_cap, &s.claimed, &s.over);
        for (uint32_t j = tid; j <= mask; j += SEAL_THREADS) tab[j] = SEAL_EMPTY;
        __syncthreads(); // every thread has read the counter and the list
        if (tid == 0) reset();
        __syncthreads();
    }
};

template <bool LDS>
__global__ void __launch_bounds__(SEAL_THREADS) seal_nodes_capped_kernel(const SealParams P, const SealCapParams C) {
    extern __shared__ __align__(16) unsigned char seal_lds[];
    __shared__ SealShared s;
    __shared__ SealPoolShared ps;
    SealCappedHops hops(C, ps, seal_lds);
    seal_slots<LDS>(P, s, seal_lds, hops);
}

static int seal_max_cap_ok(int32_t max_cap, const char *who) {
    TG_REQUIRE(max_cap >= 0 && max_cap <= TG_SEAL_HOP_CAP_MAX, "%s: a hop's cap of %d outside [0, %d]", who, max_cap,
               TG_SEAL_HOP_CAP_MAX);
    return TG_OK;
}

} // namespace tg

extern "C" int tg_seal_capped_workspace_bytes(int64_t m, int32_t node_cap, int32_t max_cap, int32_t form, int64_t *bytes,
                                              int32_t *form_taken) {
    const char *who = "tg_seal_capped_workspace_bytes";
    TG_REQUIRE(bytes, "%s: null bytes", who);
    tg::SealPlan pl;
    int rc = tg::seal_plan(m, node_cap, form, &pl, who);
    if (rc != TG_OK) return rc;
    rc = tg::seal_max_cap_ok(max_cap, who);
    if (rc != TG_OK) return rc;
    *bytes = pl.groups * pl.group_bytes;
    if (form_taken) *form_taken = pl.form;
    return TG_OK;
}

extern "C" int tg_seal_nodes_capped(const tg_graph *g, const tg_seal_in *in, const tg_seal_caps *caps, const tg_seal_out *out,
                                    int64_t m, int32_t form, int32_t *status, void *workspace, int64_t workspace_bytes,
                                    void *stream_) {
    using namespace tg;
    const char *who = "tg_seal_nodes_capped";
    TG_REQUIRE(g && in && out, "%s: null graph / in / out", who);
    TG_REQUIRE(caps && caps->max_per_hop, "%s: null caps / max_per_hop", who);
    SealPlan pl;
    int rc = seal_plan(m, in->node_cap, form, &pl, who);
    if (rc != TG_OK) return rc;
    SealParams p;
    bool launch;
    TG_REQUIRE(in->num_hops >= 1 && in->num_hops <= TG_SEAL_MAX_HOPS, "%s: num_hops = %d outside [1, %d]", who, in->num_hops,
               TG_SEAL_MAX_HOPS);
    SealCapParams c;
    int32_t max_cap = 0;
    for (int t = 0; t < TG_SEAL_MAX_HOPS; ++t) {
        const int32_t k = t < in->num_hops ? caps->max_per_hop[t] : 0;
        rc = seal_max_cap_ok(k, who);
        if (rc != TG_OK) return rc;
        c.k[t] = (uint16_t)k;
        max_cap = std::max(max_cap, k);
    }
    rc = seal_params(g, in, out, m, pl, status, workspace, workspace_bytes, &p, &launch, who);
    if (rc != TG_OK || !launch) return rc;
    c.seed = caps->seed, c.call_ids = caps->call_ids, c.call_id0 = caps->call_id0, c.cut = caps->cut;
    c.log_tp_max = seal_log_tp((uint32_t)max_cap);
    c.pool_at = (int32_t)pl.lds_bytes; // a multiple of 16
    const int64_t lds_bytes = pl.lds_bytes + ((int64_t)10 << c.log_tp_max);
    hipStream_t stream = (hipStream_t)stream_;
    const void *fn = pl.form == TG_SEAL_FORM_LDS ? reinterpret_cast<const void *>(&seal_nodes_capped_kernel<true>)
                                                 : reinterpret_cast<const void *>(&seal_nodes_capped_kernel<false>);
    if (lds_bytes > 64 * 1024) TG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    if (pl.form == TG_SEAL_FORM_LDS) {
        // as many workgroups as a CU's 160 KiB keep resident (six at most, tg_seal_nodes' figure) on 256 CUs walk the slots;
        // a workgroup's static LDS (SealShared + SealPoolShared, 5 216 B) counts as 5 632: LDS is granted in blocks of 512 B
        const int64_t per_cu = std::min<int64_t>(6, (160 * 1024) / (lds_bytes + 5632));
        const int64_t grid = std::min<int64_t>(m, 256 * per_cu);
        hipLaunchKernelGGL(seal_nodes_capped_kernel<true>, dim3((unsigned)grid), dim3(SEAL_THREADS), (size_t)lds_bytes, stream, p,
                           c);
    } else {
        hipLaunchKernelGGL(seal_nodes_capped_kernel<false>, dim3((unsigned)pl.groups), dim3(SEAL_THREADS), (size_t)lds_bytes,
                           stream, p, c);
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}
