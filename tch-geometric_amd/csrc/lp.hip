// A balanced label-propagation partitioner (tg_lp_sizes / tg_lp_propose / tg_lp_commit; the rule in include/tchgeo_lp.h;
// DESIGN.md 4.26).  Propose is one pass over every entry of the graph with a random gather of the neighbour's label per
// entry; the work per row is a histogram of at most min(row length, P) labels and its arg-max.
//   tile     64 consecutive entries of a row, one per lane, loaded coalesced; the lane gathers label[w].  An entry that
//            counts nowhere (a self loop, an id outside [0, n), a label outside [0, P)) becomes the sentinel label 2^32 - 1.
//   sort     the 64 labels are bitonic-sorted through __shfl_xor (21 compare-exchanges, no LDS).  A lane whose label differs
//            from the lane below is a run head; one ballot holds the heads and a run's length is the distance to the next
//            head.  So a tile hands over at most one (label, count) pair per distinct label, and no two of its pairs collide.
//   WAVE     one wavefront owns a row; a persistent grid of 256-thread workgroups whose four waves never meet a barrier.
//            A row of one tile finishes in registers: the maximum of (count, smaller label) and cnt[l0] are wave reductions.
//            A row of up to TG_LP_WAVE_MAX entries gathers the labels of ALL its (at most eight) tiles before the first is
//            used, then folds each tile's runs into an open-addressed (label, count) table in LDS that the wavefront owns:
//            1024 slots for at most 512 distinct labels.  Every slot a row claims goes on a touched list, so the arg-max and
//            the clean-up cost the row's distinct labels, not the table.  A longer row (the form forced) goes tile by tile,
//            and if it can hold more than 512 distinct labels it takes one pass per 512 consecutive label values.
//            Under AUTO a row longer than wave_max is appended to a list (one atomic per such row).
//   GROUP    one workgroup owns a row.  While min(row length, P) <= TG_LP_LDS_LABELS the table is 4096 slots of LDS, claimed
//            with an LDS compare-and-swap and counted with LDS atomic adds; otherwise it is a dense array of P uint32
//            counters in the workspace, one per resident workgroup, counted with device atomics, with the touched labels
//            listed behind it.  The call clears the dense arrays once; a row cleans up behind itself through its list.
//   cut      a wavefront (a workgroup in the group kernel) sums valid - cnt[l0] over its rows and adds it to cut_entries with
//            one 64-bit atomic when its loop ends.
// Commit: free[] is snapshotted and the vertex ids written out; rocprim's stable radix sort orders (skey, v) -- the ids
// ascend going in, so equal keys keep the smaller v first, and the all-ones words of the vertices that stay sort behind
// every mover; a head-flag pass writes each target's first place; the last kernel takes a place's rank as its index minus
// that, admits while rank < free[target], writes `label` and updates `size` and `moved` with integer atomics.
// LDS: wave kernel 4 x (4 + 4 + 2) KiB = 40 KiB per workgroup, four workgroups per CU; group kernel 16 + 16 + 8 KiB = 40 KiB.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "rw_walk.h"

#include "../../include/tchgeo_lp.h"

namespace tg {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr uint32_t LP_SENT = 0xFFFFFFFFu;           // the label of an entry that counts nowhere; also an empty slot
constexpr int LP_WAVE_TILES = TG_LP_WAVE_MAX / 64;  // tiles gathered ahead
constexpr int LP_WAVE_SLOTS = 2 * TG_LP_WAVE_MAX;   // load <= 1/2
constexpr int LP_GROUP_SLOTS = 2 * TG_LP_LDS_LABELS;
constexpr uint64_t LP_STAY = ~0ull;
static_assert((LP_WAVE_SLOTS & (LP_WAVE_SLOTS - 1)) == 0 && (LP_GROUP_SLOTS & (LP_GROUP_SLOTS - 1)) == 0, "slot masks");
static_assert(TG_LP_WAVE_MAX % 64 == 0, "whole tiles");

struct LpParams {
    CsrView g;
    int64_t n;
    const int32_t *label;
    uint32_t n_parts;
    uint64_t seed, round;
    int64_t wave_max;           // the wave kernel lists longer rows (INT64_MAX: none)
    uint64_t *skey;
    unsigned long long *cut;
    uint32_t *counter, *list;   // AUTO: the listed rows; null otherwise
    uint32_t *dense;            // the group kernel's dense tables: per workgroup P counters, then P touched labels
    int64_t dense_pitch;        // words between two workgroups' tables
};

__host__ __device__ inline int64_t lp_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

template <int SLOTS> __device__ __forceinline__ uint32_t lp_slot(uint32_t label) {
    return (label * 0x9E3779B1u) >> (32 - __builtin_ctz(SLOTS));
}

// (count, label) as one word whose maximum is the larger count, then the smaller label; 0 = nothing
__device__ __forceinline__ uint64_t lp_pack(uint32_t cnt, uint32_t label) { return ((uint64_t)cnt << 32) | (uint64_t)(LP_SENT - label); }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t u = __shfl_xor(v, off, 64);
        v = u > v ? u : v;
    }
    return v;
}

// the label entry e of v's row counts under, or the sentinel
__device__ __forceinline__ uint32_t lp_entry_label(const LpParams &P, int64_t e, int64_t r1, int64_t v) {
    if (e >= r1) return LP_SENT;
    const int64_t w = P.g.idx(e);
    if ((uint64_t)w >= (uint64_t)P.n || w == v) return LP_SENT;
    const uint32_t l = (uint32_t)P.label[w];
    return l < P.n_parts ? l : LP_SENT;
}

// Sorts one label per lane ascending over the wave (the 32-bit analogue of rc_sort64) -> the lane's sorted label; *run = the
// length of the run that starts at this lane, 0 where none does or where the run is the sentinel's.
__device__ __forceinline__ uint32_t lp_sort_runs(uint32_t x, uint32_t *run) {
    const int lane = lane_id();
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint32_t y = (uint32_t)__shfl_xor((int)x, j, 64);
            const bool keep_min = ((lane & k) == 0) == ((lane & j) == 0);
            x = keep_min ? (x < y ? x : y) : (x > y ? x : y);
        }
    }
    const uint32_t below = (uint32_t)__shfl_up((int)x, 1, 64);
    const bool head = lane == 0 || x != below;
    const uint64_t heads = __ballot(head);
    const uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    *run = head && x != LP_SENT ? (uint32_t)(next - lane) : 0u;
    return x;
}

// what a row's scan leaves: the best foreign (count, label), cnt[l0] and the number of counted entries
struct LpRow {
    uint64_t best;
    uint32_t own, valid;
};

__device__ __forceinline__ void lp_write(const LpParams &P, CallKey ck, int64_t v, const LpRow &r, uint64_t &cut) {
    // one lane calls this with the wave's (the workgroup's) reduced values
    const uint32_t cnt = (uint32_t)(r.best >> 32);
    uint64_t word = LP_STAY;
    if (cnt > r.own) {
        const uint64_t best = (uint64_t)(LP_SENT - (uint32_t)r.best);
        const uint32_t gain = cnt - r.own;
        word = (best << 44) | ((uint64_t)(4095u - (gain < 4095u ? gain : 4095u)) << 32) | (uint64_t)draw(ck, (uint64_t)v, 0u, 0u).w[0];
    }
    P.skey[v] = word;
    cut += (uint64_t)(r.valid - r.own);
}

// ---- the wave kernel's table ------------------------------------------------------------------------------------------------
struct LpWaveTable {
    uint32_t *key, *cnt, *touched;
    uint32_t n_touched; // wave-uniform
};

// a tile's runs with lo <= label < hi into the table; every lane of the wave calls it
__device__ __forceinline__ void lp_wave_fold(LpWaveTable &T, uint32_t x, uint32_t run, uint32_t lo, uint32_t hi) {
    const int lane = lane_id();
    bool fresh = false;
    uint32_t s = 0;
    if (run != 0 && x >= lo && x < hi) {
        s = lp_slot<LP_WAVE_SLOTS>(x);
        for (;;) { // at most 512 distinct labels ever sit in 1024 slots: the probe ends
            const uint32_t prev = atomicCAS(&T.key[s], LP_SENT, x);
            if (prev == LP_SENT) fresh = true;
            if (prev == LP_SENT || prev == x) break;
            s = (s + 1) & (LP_WAVE_SLOTS - 1);
        }
        T.cnt[s] += run; // the heads of one tile carry distinct labels: distinct slots
    }
    const uint64_t fb = __ballot(fresh); // outside the divergent part: it sees every fresh lane
    if (fresh) T.touched[T.n_touched + (uint32_t)__popcll(fb & ((1ull << lane) - 1ull))] = s;
    T.n_touched += (uint32_t)__popcll(fb);
    wave_lds_handoff();
}

// the arg-max over the touched slots, which are emptied on the way
__device__ __forceinline__ void lp_wave_drain(LpWaveTable &T, uint32_t l0, uint64_t &best, uint32_t &own) {
    for (uint32_t j = lane_id(); j < T.n_touched; j += 64) {
        const uint32_t s = T.touched[j], l = T.key[s], c = T.cnt[s];
        T.key[s] = LP_SENT;
        T.cnt[s] = 0;
        if (l == l0) own += c;
        else {
            const uint64_t p = lp_pack(c, l);
            best = p > best ? p : best;
        }
    }
    T.n_touched = 0;
    wave_lds_handoff();
}

__global__ void lp_clear_kernel(uint32_t *counter, uint32_t *dense, int64_t dense_words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (i == 0 && counter) *counter = 0;
    for (int64_t j = i; j < dense_words; j += step) dense[j] = 0;
}

__global__ void __launch_bounds__(LP_THREADS) lp_wave_kernel(const LpParams P) {
    __shared__ uint32_t s_key[LP_WAVES][LP_WAVE_SLOTS];
    __shared__ uint32_t s_cnt[LP_WAVES][LP_WAVE_SLOTS];
    __shared__ uint32_t s_touched[LP_WAVES][TG_LP_WAVE_MAX];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    LpWaveTable T{s_key[wave], s_cnt[wave], s_touched[wave], 0u};
    for (int j = lane; j < LP_WAVE_SLOTS; j += 64) T.key[j] = LP_SENT, T.cnt[j] = 0;
    wave_lds_handoff();
    const CallKey ck = call_key(P.seed, P.round, TG_TAG_LP);
    const int64_t n_waves = (int64_t)gridDim.x * LP_WAVES;
    uint64_t cut = 0; // lane 0's is the wave's
    for (int64_t v = (int64_t)blockIdx.x * LP_WAVES + wave; v < P.n; v += n_waves) { // wave-uniform throughout
        const int64_t r0 = P.g.ptr(v), r1 = max(r0, P.g.ptr(v + 1)), len = r1 - r0;
        if (len > P.wave_max) { // the group kernel's
            if (lane == 0) P.list[atomicAdd(P.counter, 1u)] = (uint32_t)v;
            continue;
        }
        const uint32_t l0 = (uint32_t)P.label[v];
        LpRow r{0ull, 0u, 0u};
        if (len == 0 || l0 >= P.n_parts) {
            if (lane == 0) P.skey[v] = LP_STAY;
            continue;
        }
        if (len <= 64) { // in registers
            uint32_t run;
            const uint32_t x = lp_sort_runs(lp_entry_label(P, r0 + lane, r1, v), &run);
            r.valid = (uint32_t)__popcll(__ballot(x != LP_SENT));
            r.own = wave_sum<uint32_t>(x == l0 ? run : 0u);
            r.best = wave_max_u64(run != 0 && x != l0 ? lp_pack(run, x) : 0ull);
        } else if (len <= TG_LP_WAVE_MAX) { // every tile's gathers are issued before the first label is used
            uint32_t lab[LP_WAVE_TILES];
#pragma unroll
            for (int t = 0; t < LP_WAVE_TILES; ++t) lab[t] = lp_entry_label(P, r0 + t * 64 + lane, r1, v);
            const int tiles = (int)((len + 63) >> 6);
#pragma unroll
            for (int t = 0; t < LP_WAVE_TILES; ++t)
                if (t < tiles) {
                    uint32_t run;
                    const uint32_t x = lp_sort_runs(lab[t], &run);
                    r.valid += (uint32_t)__popcll(__ballot(x != LP_SENT));
                    lp_wave_fold(T, x, run, 0u, P.n_parts);
                }
            uint64_t best = 0;
            uint32_t own = 0;
            lp_wave_drain(T, l0, best, own);
            r.best = wave_max_u64(best);
            r.own = wave_sum<uint32_t>(own);
        } else { // the form forced on a long row: one pass per TG_LP_WAVE_MAX label values that can occur
            const bool one_pass = min(len, (int64_t)P.n_parts) <= TG_LP_WAVE_MAX;
            uint64_t best = 0;
            uint32_t own = 0;
            for (uint32_t lo = 0; lo < P.n_parts; lo += TG_LP_WAVE_MAX) {
                const uint32_t hi = one_pass ? P.n_parts : min(lo + (uint32_t)TG_LP_WAVE_MAX, P.n_parts);
                for (int64_t t = r0; t < r1; t += 64) {
                    uint32_t run;
                    const uint32_t x = lp_sort_runs(lp_entry_label(P, t + lane, r1, v), &run);
                    if (lo == 0) r.valid += (uint32_t)__popcll(__ballot(x != LP_SENT));
                    lp_wave_fold(T, x, run, lo, hi);
                }
                lp_wave_drain(T, l0, best, own);
                if (one_pass) break;
            }
            r.best = wave_max_u64(best);
            r.own = wave_sum<uint32_t>(own);
        }
        if (lane == 0) lp_write(P, ck, v, r, cut);
    }
    if (lane == 0 && cut != 0) atomicAdd(P.cut, (unsigned long long)cut);
}

__global__ void __launch_bounds__(LP_THREADS) lp_group_kernel(const LpParams P) {
    __shared__ uint32_t s_key[LP_GROUP_SLOTS];
    __shared__ uint32_t s_cnt[LP_GROUP_SLOTS];
    __shared__ uint32_t s_touched[TG_LP_LDS_LABELS];
    __shared__ uint32_t s_n_touched;
    __shared__ uint64_t s_best[LP_WAVES];
    __shared__ uint32_t s_own[LP_WAVES], s_valid[LP_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (int j = tid; j < LP_GROUP_SLOTS; j += LP_THREADS) s_key[j] = LP_SENT, s_cnt[j] = 0;
    if (tid == 0) s_n_touched = 0;
    uint32_t *d_cnt = P.dense ? P.dense + (int64_t)blockIdx.x * P.dense_pitch : nullptr;
    uint32_t *d_touched = d_cnt ? d_cnt + P.n_parts : nullptr;
    const CallKey ck = call_key(P.seed, P.round, TG_TAG_LP);
    // the wave kernel ran before on the stream: its counter is final
    const int64_t n_rows = P.list ? (int64_t)min((uint64_t)*P.counter, (uint64_t)P.n) : P.n;
    uint64_t cut = 0; // thread 0's is the workgroup's
    __syncthreads();
    for (int64_t j = blockIdx.x; j < n_rows; j += gridDim.x) { // block-uniform: every thread meets every barrier
        const int64_t v = P.list ? (int64_t)P.list[j] : j;
        const int64_t r0 = P.g.ptr(v), r1 = max(r0, P.g.ptr(v + 1)), len = r1 - r0;
        const uint32_t l0 = (uint32_t)P.label[v];
        if (len == 0 || l0 >= P.n_parts) {
            if (tid == 0) P.skey[v] = LP_STAY;
            continue;
        }
        const bool dense = min(len, (int64_t)P.n_parts) > TG_LP_LDS_LABELS; // then P > TG_LP_LDS_LABELS: d_cnt is there
        uint32_t valid = 0;
        for (int64_t e = r0 + tid; e < r1; e += LP_THREADS) {
            const uint32_t x = lp_entry_label(P, e, r1, v);
            if (x == LP_SENT) continue;
            ++valid;
            if (dense) {
                if (atomicAdd(&d_cnt[x], 1u) == 0u) d_touched[atomicAdd(&s_n_touched, 1u)] = x;
            } else {
                uint32_t s = lp_slot<LP_GROUP_SLOTS>(x);
                for (;;) { // at most 2048 distinct labels in 4096 slots
                    const uint32_t prev = atomicCAS(&s_key[s], LP_SENT, x);
                    if (prev == LP_SENT) s_touched[atomicAdd(&s_n_touched, 1u)] = s;
                    if (prev == LP_SENT || prev == x) break;
                    s = (s + 1) & (LP_GROUP_SLOTS - 1);
                }
                atomicAdd(&s_cnt[s], 1u);
            }
        }
        __syncthreads();
        const uint32_t n_touched = s_n_touched;
        uint64_t best = 0;
        uint32_t own = 0;
        for (uint32_t k = tid; k < n_touched; k += LP_THREADS) {
            uint32_t l, c;
            if (dense) { // the counts were made by device atomics: read and clear them where those were performed
                l = d_touched[k];
                c = atomicExch(&d_cnt[l], 0u);
            } else {
                const uint32_t s = s_touched[k];
                l = s_key[s], c = s_cnt[s];
                s_key[s] = LP_SENT, s_cnt[s] = 0;
            }
            if (l == l0) own += c;
            else {
                const uint64_t p = lp_pack(c, l);
                best = p > best ? p : best;
            }
        }
        best = wave_max_u64(best);
        own = wave_sum<uint32_t>(own);
        valid = wave_sum<uint32_t>(valid);
        if (lane == 0) s_best[wave] = best, s_own[wave] = own, s_valid[wave] = valid;
        __syncthreads();
        if (tid == 0) {
            LpRow r{0ull, 0u, 0u};
            for (int w = 0; w < LP_WAVES; ++w) {
                r.best = s_best[w] > r.best ? s_best[w] : r.best;
                r.own += s_own[w];
                r.valid += s_valid[w];
            }
            lp_write(P, ck, v, r, cut);
            s_n_touched = 0;
        }
        __syncthreads(); // the totals are read, the table is empty again
    }
    if (tid == 0 && cut != 0) atomicAdd(P.cut, (unsigned long long)cut);
}

// ---- tg_lp_sizes --------------------------------------------------------------------------------------------------------
__global__ void lp_zero_sizes_kernel(int64_t *size, int32_t n_parts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_parts) size[i] = 0;
}

// a histogram in LDS per workgroup while P fits there, device atomics per vertex otherwise
__global__ void __launch_bounds__(LP_THREADS) lp_sizes_kernel(const int32_t *label, int64_t n, uint32_t n_parts,
                                                              unsigned long long *size, int32_t *status) {
    __shared__ uint32_t s_hist[TG_LP_LDS_LABELS];
    const bool lds = n_parts <= TG_LP_LDS_LABELS;
    if (lds) {
        for (uint32_t l = threadIdx.x; l < n_parts; l += LP_THREADS) s_hist[l] = 0;
        __syncthreads();
    }
    bool bad = false;
    for (int64_t v = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x; v < n; v += (int64_t)gridDim.x * LP_THREADS) {
        const uint32_t l = (uint32_t)label[v];
        if (l >= n_parts) bad = true;
        else if (lds) atomicAdd(&s_hist[l], 1u);
        else atomicAdd(&size[l], 1ull);
    }
    if (__ballot(bad) != 0 && lane_id() == 0) atomicOr(status, TG_LP_STATUS_LABEL);
    if (lds) {
        __syncthreads();
        for (uint32_t l = threadIdx.x; l < n_parts; l += LP_THREADS)
            if (s_hist[l] != 0) atomicAdd(&size[l], (unsigned long long)s_hist[l]);
    }
}

// ---- tg_lp_commit -------------------------------------------------------------------------------------------------------
struct LpCommit {
    int32_t *label;
    unsigned long long *size, *moved;
    int64_t n, cap;
    uint32_t n_parts;
    const uint64_t *keys; // sorted
    const uint32_t *verts; // sorted along
    int64_t *free;
    uint32_t *first;
    int32_t *status;
};

__global__ void lp_snapshot_kernel(const int64_t *size, int64_t cap, uint32_t n_parts, int64_t *free, int64_t n, uint32_t *verts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_parts) free[i] = max((int64_t)0, cap - size[i]);
    if (i < n) verts[i] = (uint32_t)i;
}

// the first place of every target among the sorted keys
__global__ void lp_heads_kernel(const LpCommit C) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C.n) return;
    const uint64_t k = C.keys[i];
    if (k == LP_STAY) return;
    const uint64_t t = k >> 44;
    if (t < C.n_parts && (i == 0 || (C.keys[i - 1] >> 44) != t)) C.first[t] = (uint32_t)i;
}

__global__ void __launch_bounds__(LP_THREADS) lp_admit_kernel(const LpCommit C) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool admitted = false, bad = false;
    if (i < C.n) {
        const uint64_t k = C.keys[i];
        if (k != LP_STAY) {
            const uint64_t t = k >> 44;
            if (t >= C.n_parts) bad = true;
            else if (i - (int64_t)C.first[t] < C.free[t]) {
                const uint32_t v = C.verts[i];
                const uint32_t from = (uint32_t)C.label[v];
                if (from < C.n_parts) atomicAdd(&C.size[from], ~0ull); // - 1
                atomicAdd(&C.size[t], 1ull);
                C.label[v] = (int32_t)t;
                admitted = true;
            }
        }
    }
    const uint64_t ab = __ballot(admitted);
    if (lane_id() == 0) {
        if (ab != 0) atomicAdd(C.moved, (unsigned long long)__popcll(ab));
    }
    if (__ballot(bad) != 0 && lane_id() == 0) atomicOr(C.status, TG_LP_STATUS_TARGET);
}

static size_t lp_sort_temp(int64_t n) {
    size_t st = 0;
    (void)rocprim::radix_sort_pairs(nullptr, st, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (size_t)(n > 0 ? n : 1), 0, 64, (hipStream_t)0, false);
    return st;
}

struct LpPlan {
    int64_t list_off, dense_off, dense_pitch, propose_bytes; // propose
    int64_t free_off, first_off, vin_off, vout_off, keys_off, temp_off, temp_bytes, commit_bytes;
    int64_t bytes;
    int32_t wave_max;
};

static int lp_plan(int64_t n, int32_t n_parts, int32_t form, int32_t wave_max, LpPlan *pl, const char *who) {
    TG_REQUIRE(n >= 0, "%s: n = %lld is negative", who, (long long)n);
    if (n >= ((int64_t)1 << 31)) return fail(TG_ERR_UNSUPPORTED, "%s: %lld vertices exceed the 2^31 - 1 this kernel takes", who, (long long)n);
    TG_REQUIRE(n_parts >= 1 && n_parts <= TG_LP_MAX_PARTS, "%s: n_parts = %d outside [1, 2^20]", who, n_parts);
    TG_REQUIRE(form >= TG_LP_FORM_AUTO && form <= TG_LP_FORM_GROUP, "%s: unknown form %d", who, form);
    TG_REQUIRE(wave_max >= 0 && wave_max <= TG_LP_WAVE_MAX, "%s: wave_max = %d outside [0, %d]", who, wave_max, TG_LP_WAVE_MAX);
    const int64_t P = n_parts;
    pl->wave_max = wave_max > 0 ? wave_max : TG_LP_WAVE_MAX;
    pl->list_off = 256;
    pl->dense_off = pl->list_off + (form == TG_LP_FORM_AUTO ? lp_r256(4 * n) : 0);
    pl->dense_pitch = form != TG_LP_FORM_WAVE && P > TG_LP_LDS_LABELS ? lp_r256(8 * P) / 4 : 0;
    pl->propose_bytes = pl->dense_off + TG_LP_DENSE_GROUPS * 4 * pl->dense_pitch;
    pl->free_off = 0;
    pl->first_off = pl->free_off + lp_r256(8 * P);
    pl->vin_off = pl->first_off + lp_r256(4 * P);
    pl->vout_off = pl->vin_off + lp_r256(4 * n);
    pl->keys_off = pl->vout_off + lp_r256(4 * n);
    pl->temp_off = pl->keys_off + lp_r256(8 * n);
    pl->temp_bytes = lp_r256((int64_t)lp_sort_temp(n));
    pl->commit_bytes = pl->temp_off + pl->temp_bytes;
    pl->bytes = std::max(pl->propose_bytes, pl->commit_bytes);
    return TG_OK;
}

static inline unsigned lp_grid(int64_t n) { return (unsigned)((std::max<int64_t>(n, 1) + LP_THREADS - 1) / LP_THREADS); }

} // namespace tg

extern "C" int tg_lp_workspace_bytes(int64_t n, int32_t n_parts, int32_t form, int32_t wave_max, int64_t *bytes,
                                     int32_t *form_taken) {
    TG_REQUIRE(bytes, "tg_lp_workspace_bytes: null bytes");
    tg::LpPlan pl;
    const int rc = tg::lp_plan(n, n_parts, form, wave_max, &pl, "tg_lp_workspace_bytes");
    if (rc != TG_OK) return rc;
    *bytes = pl.bytes;
    if (form_taken) *form_taken = form;
    return TG_OK;
}

extern "C" int tg_lp_sizes(const int32_t *label, int64_t n, int32_t n_parts, int64_t *size, int32_t *status, void *stream_) {
    using namespace tg;
    const char *who = "tg_lp_sizes";
    LpPlan pl;
    const int rc = lp_plan(n, n_parts, TG_LP_FORM_WAVE, 0, &pl, who);
    if (rc != TG_OK) return rc;
    TG_REQUIRE(size && status && (label || n == 0), "%s: null label / size / status", who);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(lp_zero_sizes_kernel, dim3(lp_grid(n_parts)), dim3(LP_THREADS), 0, stream, size, n_parts);
    if (n > 0)
        hipLaunchKernelGGL(lp_sizes_kernel, dim3(std::min(lp_grid(n), 1024u)), dim3(LP_THREADS), 0, stream, label, n,
                           (uint32_t)n_parts, reinterpret_cast<unsigned long long *>(size), status);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_lp_propose(const tg_graph *g, const int32_t *label, int32_t n_parts, uint64_t seed, uint64_t round,
                             int32_t form, int32_t wave_max, uint64_t *skey, uint64_t *cut_entries, int32_t *status,
                             void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_lp_propose";
    TG_REQUIRE(g, "%s: null graph", who);
    TG_REQUIRE(g->n_major >= 0 && g->n_edges >= 0, "%s: negative graph size", who);
    LpPlan pl;
    const int rc = lp_plan(g->n_major, n_parts, form, wave_max, &pl, who);
    if (rc != TG_OK) return rc;
    if (g->n_edges >= ((int64_t)1 << 32))
        return fail(TG_ERR_UNSUPPORTED, "%s: %lld entries exceed the 2^32 - 1 a 32-bit count takes", who, (long long)g->n_edges);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    const int64_t n = g->n_major;
    if (n == 0) return TG_OK; // nothing to launch
    TG_REQUIRE((g->ptrs || g->ptrs32) && (g->indices || g->indices32 || g->n_edges == 0), "%s: null graph arrays", who);
    TG_REQUIRE(label && skey && cut_entries && status, "%s: null label / skey / cut_entries / status", who);
    TG_REQUIRE(workspace && workspace_bytes >= pl.propose_bytes, "%s: the workspace has %lld bytes, the call needs %lld", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)pl.propose_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);

    char *ws = static_cast<char *>(workspace);
    LpParams p;
    p.g = CsrView{g->ptrs, g->indices, g->ptrs32, g->indices32, nullptr, 0};
    p.n = n, p.label = label, p.n_parts = (uint32_t)n_parts, p.seed = seed, p.round = round;
    p.wave_max = INT64_MAX;
    p.skey = skey, p.cut = reinterpret_cast<unsigned long long *>(cut_entries);
    p.counter = p.list = nullptr;
    p.dense = pl.dense_pitch ? reinterpret_cast<uint32_t *>(ws + pl.dense_off) : nullptr;
    p.dense_pitch = pl.dense_pitch;
    hipStream_t stream = (hipStream_t)stream_;
    if (form == TG_LP_FORM_AUTO) {
        p.counter = reinterpret_cast<uint32_t *>(ws);
        p.list = reinterpret_cast<uint32_t *>(ws + pl.list_off);
        p.wave_max = pl.wave_max;
    }
    if (p.counter || p.dense) {
        const int64_t words = TG_LP_DENSE_GROUPS * pl.dense_pitch;
        hipLaunchKernelGGL(lp_clear_kernel, dim3(std::min(lp_grid(words), 4096u)), dim3(LP_THREADS), 0, stream, p.counter, p.dense,
                           words);
    }
    const unsigned wave_grid = (unsigned)std::min<int64_t>((n + LP_WAVES - 1) / LP_WAVES, TG_LP_WAVE_GROUPS);
    const unsigned group_grid = (unsigned)std::min<int64_t>(n, p.dense ? TG_LP_DENSE_GROUPS : TG_LP_GROUP_GROUPS);
    if (form != TG_LP_FORM_GROUP) hipLaunchKernelGGL(lp_wave_kernel, dim3(wave_grid), dim3(LP_THREADS), 0, stream, p);
    if (form != TG_LP_FORM_WAVE) hipLaunchKernelGGL(lp_group_kernel, dim3(group_grid), dim3(LP_THREADS), 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_lp_commit(int32_t *label, int64_t *size, int64_t n, int32_t n_parts, int64_t cap, const uint64_t *skey,
                            int64_t *moved, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_lp_commit";
    LpPlan pl;
    const int rc = lp_plan(n, n_parts, TG_LP_FORM_WAVE, 0, &pl, who);
    if (rc != TG_OK) return rc;
    TG_REQUIRE(cap >= 1, "%s: cap = %lld is below 1", who, (long long)cap);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    if (n == 0) return TG_OK; // nothing to launch
    TG_REQUIRE(label && size && skey && moved && status, "%s: null label / size / skey / moved / status", who);
    TG_REQUIRE(workspace && workspace_bytes >= pl.commit_bytes, "%s: the workspace has %lld bytes, the call needs %lld", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)pl.commit_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);

    char *ws = static_cast<char *>(workspace);
    uint32_t *vin = reinterpret_cast<uint32_t *>(ws + pl.vin_off), *vout = reinterpret_cast<uint32_t *>(ws + pl.vout_off);
    uint64_t *keys = reinterpret_cast<uint64_t *>(ws + pl.keys_off);
    LpCommit c;
    c.label = label, c.size = reinterpret_cast<unsigned long long *>(size), c.moved = reinterpret_cast<unsigned long long *>(moved);
    c.n = n, c.cap = cap, c.n_parts = (uint32_t)n_parts;
    c.keys = keys, c.verts = vout;
    c.free = reinterpret_cast<int64_t *>(ws + pl.free_off), c.first = reinterpret_cast<uint32_t *>(ws + pl.first_off);
    c.status = status;
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned grid = lp_grid(n);
    hipLaunchKernelGGL(lp_snapshot_kernel, dim3(lp_grid(std::max<int64_t>(n, n_parts))), dim3(LP_THREADS), 0, stream, size, cap,
                       (uint32_t)n_parts, c.free, n, vin);
    size_t st = (size_t)pl.temp_bytes;
    TG_HIP(rocprim::radix_sort_pairs(ws + pl.temp_off, st, skey, keys, vin, vout, (size_t)n, 0, 64, stream, false));
    hipLaunchKernelGGL(lp_heads_kernel, dim3(grid), dim3(LP_THREADS), 0, stream, c);
    hipLaunchKernelGGL(lp_admit_kernel, dim3(grid), dim3(LP_THREADS), 0, stream, c);
    TG_LAUNCH_CHECK();
    return TG_OK;
}
