// Subgraph sketches (tg_sketch_init / _propagate / _links; the rule in include/tchgeo_sketch.h): MinHash
// words and HyperLogLog registers of every vertex's closed l-hop ball, propagated by an elementwise min / bytewise max over
// the neighbours' rows, and per link the integer statistics of the 2h rows of its ends.  Integer and order-free throughout.
//   row      W = 64 (NP + RW) words, NP = n_perm / 64 in 1..4, RW = m_reg / 256 in {1, 2, 4}: lane l of a wavefront holds the
//            NP MinHash words from word l NP and the RW register words from word 64 NP + l RW -- one load of NP words and
//            one of RW words per lane, consecutive over the wave, the widest the two sizes allow.  min and max are
//            elementwise, so which lane holds which word matters to nobody as long as the store uses the same places.
//   fold     a tile of 64 neighbour ids is loaded coalesced, one per lane (u32 shadows when the graph has them); an id
//            outside [0, n) is replaced by the destination vertex itself, which changes nothing (min and max are
//            idempotent), and flagged.  The ids are made wave-uniform four at a time (v_readlane), the four rows are
//            loaded, and only then folded: four rows of latency in flight per wave, and a row shorter than four pays its
//            latency once (the missing ones are the vertex's own row again, an L2 hit, no branch).
//   bytes    four registers to a word: the bytewise unsigned max is taken on the even and the odd bytes as 16-bit fields
//            ((a | 0x0100) - b keeps bit 8 where a >= b), correct for every byte value.  No atomics anywhere on rows.
//   WAVE     one wavefront owns a destination row; a persistent grid of 256-thread workgroups whose waves never meet.
//            Under AUTO / SPLIT it lists the rows it leaves to the kernels behind it (one or two atomics per such row).
//   GROUP    one workgroup owns a row (or, for SPLIT, a segment of one): its four waves fold a contiguous quarter each --
//            contiguous rather than interleaved, so that every wave's id tiles stay coalesced; the words are equal -- and
//            waves 1..3 hand their partial rows to wave 0 through LDS once.
//   SPLIT    the group kernel over (row, segment) pairs into partial rows in the workspace, then one wavefront per split
//            row folds its partial rows (the same four-at-a-time fold, the "ids" being partial-row numbers).
//   links    one wavefront owns a link: its 2h rows in registers (at most 6 x 8 words per lane), `match` by a ballot and
//            popcount per word, the register statistics as two DPP wave sums of 32-bit fields per item.
#include <algorithm>

#include "rw_walk.h"

#include "../../include/tchgeo_sketch.h"

namespace tg {

constexpr int SK_THREADS = 256;
constexpr int SK_WAVES = SK_THREADS / 64;
constexpr int SK_INFLIGHT = 4; // neighbour rows loaded before any is folded
constexpr uint32_t SK_NONE = 0xFFFFFFFFu;
constexpr int64_t SK_NO_LIMIT = INT64_MAX;
enum { SK_ROWS_ALL = 0, SK_ROWS_LISTED = 1, SK_SEGMENTS = 2 };

template <int K> struct alignas(K == 3 ? 4 : 4 * K) SkVec {
    uint32_t w[K];
};
template <int NP, int RW> struct SkRow {
    SkVec<NP> m;
    SkVec<RW> r;
};

__host__ __device__ inline int64_t sk_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

template <int NP, int RW, typename T> __device__ __forceinline__ SkRow<NP, RW> sk_load(const T *row, int lane) {
    SkRow<NP, RW> v;
    v.m = *reinterpret_cast<const SkVec<NP> *>(row + lane * NP);
    v.r = *reinterpret_cast<const SkVec<RW> *>(row + 64 * NP + lane * RW);
    return v;
}
template <int NP, int RW, typename T> __device__ __forceinline__ void sk_store(T *row, int lane, const SkRow<NP, RW> &v) {
    *reinterpret_cast<SkVec<NP> *>(row + lane * NP) = v.m;
    *reinterpret_cast<SkVec<RW> *>(row + 64 * NP + lane * RW) = v.r;
}

// the unsigned max of each of the four bytes
__device__ __forceinline__ uint32_t sk_bytemax(uint32_t a, uint32_t b) {
    const uint32_t ae = a & 0x00FF00FFu, be = b & 0x00FF00FFu, ao = (a >> 8) & 0x00FF00FFu, bo = (b >> 8) & 0x00FF00FFu;
    const uint32_t ge = ((((ae | 0x01000100u) - be) >> 8) & 0x00010001u) * 0xFFu; // 0xFF in the fields where a >= b
    const uint32_t go = ((((ao | 0x01000100u) - bo) >> 8) & 0x00010001u) * 0xFFu;
    return ((ae & ge) | (be & ~ge)) | (((ao & go) | (bo & ~go)) << 8);
}

template <int NP, int RW> __device__ __forceinline__ void sk_fold(SkRow<NP, RW> &acc, const SkRow<NP, RW> &v) {
#pragma unroll
    for (int k = 0; k < NP; ++k) acc.m.w[k] = min(acc.m.w[k], v.m.w[k]);
#pragma unroll
    for (int k = 0; k < RW; ++k) acc.r.w[k] = sk_bytemax(acc.r.w[k], v.r.w[k]);
}

// Folds the rows src[id * W ..] of the ids held by lanes 0 .. cnt - 1 (cnt in [1, 64], wave-uniform); the lanes from cnt on
// hold an id whose row changes nothing.  Lane numbers read stay below 64: j <= 60.
template <int NP, int RW>
__device__ __forceinline__ void sk_fold_tile(SkRow<NP, RW> &acc, const uint32_t *__restrict__ src, uint32_t my_id, int cnt) {
    constexpr int64_t W = 64 * (NP + RW);
    const int lane = lane_id();
    for (int j = 0; j < cnt; j += SK_INFLIGHT) {
        SkRow<NP, RW> t[SK_INFLIGHT];
#pragma unroll
        for (int k = 0; k < SK_INFLIGHT; ++k) {
            const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)my_id, j + k);
            t[k] = sk_load<NP, RW>(src + (int64_t)id * W, lane);
        }
#pragma unroll
        for (int k = 0; k < SK_INFLIGHT; ++k) sk_fold(acc, t[k]);
    }
}

struct SkProp {
    CsrView g;
    int64_t n, n_edges;
    const uint32_t *prev;
    uint32_t *next;
    int32_t *status;
    int64_t wave_max, group_max, seg;    // rows longer than wave_max are listed (SK_NO_LIMIT: none)
    uint32_t *counters;                  // [0] group rows, [1] split rows, [2] segments
    uint32_t *group_list;                // [cap_group]
    uint2 *row_list, *seg_list;          // [cap_rows] {row, first segment}, [cap_segs] {row, segment of the row}
    uint32_t *partial;                   // [cap_segs, W]
    int64_t cap_group, cap_rows, cap_segs;
};

// the entries [b, e) of x's row, inside [0, n_edges] whatever the pointers hold
__device__ __forceinline__ void sk_row_range(const SkProp &P, int64_t x, int64_t &b, int64_t &e) {
    b = min(max(P.g.ptr(x), (int64_t)0), P.n_edges);
    e = min(max(P.g.ptr(x + 1), b), P.n_edges);
}

// folds the rows of the entries [b, e) into acc; x is the destination vertex
template <int NP, int RW>
__device__ __forceinline__ void sk_fold_entries(const SkProp &P, SkRow<NP, RW> &acc, int64_t x, int64_t b, int64_t e) {
    const int lane = lane_id();
    bool bad = false;
    for (int64_t t = b; t < e; t += 64) {
        const int cnt = (int)min((int64_t)64, e - t);
        uint32_t id = (uint32_t)x;
        if (lane < cnt) {
            const int64_t y = P.g.idx(t + lane);
            if ((uint64_t)y < (uint64_t)P.n) id = (uint32_t)y;
            else bad = true;
        }
        sk_fold_tile<NP, RW>(acc, P.prev, id, cnt);
    }
    if (__ballot(bad) != 0 && lane == 0) atomicOr(P.status, TG_SKETCH_STATUS_RANGE);
}

__global__ void sk_clear_kernel(uint32_t *counters) { counters[0] = counters[1] = counters[2] = 0; }

template <int NP, int RW> __global__ void __launch_bounds__(SK_THREADS) sk_wave_kernel(const SkProp P) {
    constexpr int64_t W = 64 * (NP + RW);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * SK_WAVES;
    for (int64_t x = (int64_t)blockIdx.x * SK_WAVES + wave; x < P.n; x += n_waves) { // wave-uniform throughout
        int64_t b, e;
        sk_row_range(P, x, b, e);
        const int64_t deg = e - b;
        if (deg > P.wave_max) {
            if (deg <= P.group_max) {
                if (lane == 0) {
                    const uint32_t at = atomicAdd(&P.counters[0], 1u);
                    if (at < P.cap_group) P.group_list[at] = (uint32_t)x;
                    else atomicOr(P.status, TG_SKETCH_STATUS_GRAPH);
                }
            } else {
                const int64_t nseg = (deg + P.seg - 1) / P.seg;
                uint32_t at = 0, first = 0;
                if (lane == 0) {
                    at = atomicAdd(&P.counters[1], 1u);
                    first = atomicAdd(&P.counters[2], (uint32_t)nseg);
                }
                at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
                first = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
                const bool ok = at < P.cap_rows && (int64_t)first + nseg <= P.cap_segs;
                const uint32_t row = ok ? (uint32_t)x : SK_NONE;
                if (lane == 0) {
                    if (at < P.cap_rows) P.row_list[at] = make_uint2(row, first);
                    if (!ok) atomicOr(P.status, TG_SKETCH_STATUS_GRAPH);
                }
                for (int64_t s = lane; s < nseg; s += 64)
                    if ((int64_t)first + s < P.cap_segs) P.seg_list[(int64_t)first + s] = make_uint2(row, (uint32_t)s);
            }
            continue;
        }
        SkRow<NP, RW> acc = sk_load<NP, RW>(P.prev + x * W, lane);
        sk_fold_entries<NP, RW>(P, acc, x, b, e);
        sk_store<NP, RW>(P.next + x * W, lane, acc);
    }
}

// One workgroup per item: a row (every row, or the listed ones) into `next`, or a segment into its partial row.
template <int NP, int RW> __global__ void __launch_bounds__(SK_THREADS) sk_group_kernel(const SkProp P, const int mode) {
    constexpr int64_t W = 64 * (NP + RW);
    __shared__ __attribute__((aligned(16))) uint32_t s_part[SK_WAVES - 1][W];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    // the wave kernel ran before on the stream: its counters are final
    const int64_t n_items = mode == SK_ROWS_ALL      ? P.n
                            : mode == SK_ROWS_LISTED ? min((int64_t)P.counters[0], P.cap_group)
                                                     : min((int64_t)P.counters[2], P.cap_segs);
    for (int64_t j = blockIdx.x; j < n_items; j += gridDim.x) { // block-uniform: every thread meets every barrier
        int64_t x = j, seg = 0;
        if (mode == SK_ROWS_LISTED) x = P.group_list[j];
        if (mode == SK_SEGMENTS) {
            const uint2 item = P.seg_list[j];
            if (item.x == SK_NONE) continue;
            x = item.x, seg = item.y;
        }
        int64_t b, e;
        sk_row_range(P, x, b, e);
        if (mode == SK_SEGMENTS) {
            b = min(b + seg * P.seg, e);
            e = min(b + P.seg, e);
        }
        const int64_t quarter = (e - b + SK_WAVES - 1) / SK_WAVES;
        const int64_t wb = min(b + wave * quarter, e), we = min(wb + quarter, e);
        SkRow<NP, RW> acc = sk_load<NP, RW>(P.prev + x * W, lane);
        sk_fold_entries<NP, RW>(P, acc, x, wb, we);
        if (wave > 0) sk_store<NP, RW>(s_part[wave - 1], lane, acc);
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int w = 0; w < SK_WAVES - 1; ++w) sk_fold(acc, sk_load<NP, RW>(s_part[w], lane));
            sk_store<NP, RW>(mode == SK_SEGMENTS ? P.partial + j * W : P.next + x * W, lane, acc);
        }
        __syncthreads(); // the partial rows are read
    }
}

// One wavefront per split row: its partial rows (each already holds the vertex's own row) into `next`.
template <int NP, int RW> __global__ void __launch_bounds__(SK_THREADS) sk_combine_kernel(const SkProp P) {
    constexpr int64_t W = 64 * (NP + RW);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * SK_WAVES, n_rows = min((int64_t)P.counters[1], P.cap_rows);
    for (int64_t j = (int64_t)blockIdx.x * SK_WAVES + wave; j < n_rows; j += n_waves) {
        const uint2 item = P.row_list[j];
        if (item.x == SK_NONE) continue;
        const int64_t x = item.x;
        int64_t b, e;
        sk_row_range(P, x, b, e);
        const int64_t nseg = (e - b + P.seg - 1) / P.seg; // >= 1: what the wave kernel counted
        SkRow<NP, RW> acc = sk_load<NP, RW>(P.prev + x * W, lane);
        for (int64_t t = 0; t < nseg; t += 64) {
            const int cnt = (int)min((int64_t)64, nseg - t);
            sk_fold_tile<NP, RW>(acc, P.partial, item.y + (uint32_t)(lane < cnt ? t + lane : 0), cnt);
        }
        sk_store<NP, RW>(P.next + x * W, lane, acc);
    }
}

// ---- hop 0 ------------------------------------------------------------------------------------------------------------
// One thread per 16-byte unit of the array: a MinHash unit is one Philox block; a register unit holds 16 registers and asks
// the vertex's one register draw whether it falls among them.
__global__ void __launch_bounds__(SK_THREADS) sk_init_kernel(uint4 *sketch, int64_t n, int mh_units, int units, uint32_t reg_mask,
                                                             uint32_t k0, uint32_t k1) {
    const int64_t total = n * units, stride = (int64_t)gridDim.x * SK_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x; i < total; i += stride) {
        const int64_t x = i / units;
        const int q = (int)(i - x * units);
        uint4 o = make_uint4(0, 0, 0, 0);
        if (q < mh_units) {
            const Draw d = philox4x32_10((uint32_t)x, (uint32_t)((uint64_t)x >> 32), (uint32_t)q, TG_SKETCH_TAG_MINHASH, k0, k1);
            o = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
        } else {
            const Draw d = philox4x32_10((uint32_t)x, (uint32_t)((uint64_t)x >> 32), 0u, TG_SKETCH_TAG_HLL, k0, k1);
            const int at = (int)(d.w[0] & reg_mask) - (q - mh_units) * 16; // the register's place in this unit
            const uint32_t rank = 1u + (d.w[1] ? (uint32_t)__builtin_clz(d.w[1]) : 32u);
            const uint32_t word = rank << (8 * (at & 3));
            if (at >= 0 && at < 16) {
                if ((at >> 2) == 0) o.x = word;
                if ((at >> 2) == 1) o.y = word;
                if ((at >> 2) == 2) o.z = word;
                if ((at >> 2) == 3) o.w = word;
            }
        }
        sketch[i] = o;
    }
}

// ---- links ------------------------------------------------------------------------------------------------------------
struct SkLinks {
    const uint32_t *sketch;
    const int64_t *src, *dst;
    int64_t n, m;
    int32_t h;
    int32_t *match, *uzero, *nzero;
    uint64_t *usum, *nsum;
    int32_t *status;
};

// sum over the 256 RW registers of the wave of 2^(33 - r), and the number of them that are 0.  A lane's sum is below 2^38
// and its zeros at most 16: bits 0..23 of the sum go through one 32-bit DPP wave sum, the bits above with the zeros at bit
// 20 through a second; neither overflows (64 x 2^24 and 2^19 + 2^30).
template <int RW> __device__ __forceinline__ void sk_registers(const SkVec<RW> &r, uint64_t &sum, uint32_t &zeros) {
    uint64_t s = 0;
    uint32_t z = 0;
#pragma unroll
    for (int w = 0; w < RW; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t byte = (r.w[w] >> (8 * k)) & 0xFFu;
            z += byte == 0;
            s += 1ull << (byte > 33u ? 0u : 33u - byte);
        }
    const uint32_t lo = wave_sum<uint32_t>((uint32_t)s & 0xFFFFFFu);
    const uint32_t hi = wave_sum<uint32_t>((uint32_t)(s >> 24) + (z << 20));
    sum = ((uint64_t)(hi & 0xFFFFFu) << 24) + lo;
    zeros = hi >> 20;
}

template <int NP, int RW> __global__ void __launch_bounds__(SK_THREADS) sk_links_kernel(const SkLinks P) {
    constexpr int64_t W = 64 * (NP + RW);
    constexpr int H = TG_SKETCH_MAX_HOPS;
    const int lane = lane_id(), wave = threadIdx.x >> 6, h = P.h;
    const int64_t n_waves = (int64_t)gridDim.x * SK_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * SK_WAVES + wave; i < P.m; i += n_waves) { // wave-uniform throughout
        const int64_t u = P.src[i], v = P.dst[i];
        int32_t *match = P.match + i * h * h, *uzero = P.uzero + i * h * h, *nzero = P.nzero + i * 2 * h;
        uint64_t *usum = P.usum + i * h * h, *nsum = P.nsum + i * 2 * h;
        if ((uint64_t)u >= (uint64_t)P.n || (uint64_t)v >= (uint64_t)P.n) {
            if (lane < h * h) match[lane] = 0, uzero[lane] = 0, usum[lane] = 0;
            if (lane < 2 * h) nzero[lane] = 0, nsum[lane] = 0;
            if (lane == 0) atomicOr(P.status, TG_SKETCH_STATUS_RANGE);
            continue;
        }
        SkRow<NP, RW> ru[H], rv[H];
#pragma unroll
        for (int a = 0; a < H; ++a)
            if (a < h) {
                ru[a] = sk_load<NP, RW>(P.sketch + ((a + 1) * P.n + u) * W, lane);
                rv[a] = sk_load<NP, RW>(P.sketch + ((a + 1) * P.n + v) * W, lane);
            }
#pragma unroll
        for (int a = 0; a < H; ++a)
            if (a < h) {
                uint64_t sum;
                uint32_t zeros;
                sk_registers<RW>(ru[a].r, sum, zeros);
                if (lane == 0) nsum[a] = sum, nzero[a] = (int32_t)zeros;
                sk_registers<RW>(rv[a].r, sum, zeros);
                if (lane == 0) nsum[h + a] = sum, nzero[h + a] = (int32_t)zeros;
#pragma unroll
                for (int b = 0; b < H; ++b)
                    if (b < h) {
                        int same = 0;
                        SkVec<RW> r;
#pragma unroll
                        for (int k = 0; k < NP; ++k) same += __popcll(__ballot(ru[a].m.w[k] == rv[b].m.w[k]));
#pragma unroll
                        for (int k = 0; k < RW; ++k) r.w[k] = sk_bytemax(ru[a].r.w[k], rv[b].r.w[k]);
                        sk_registers<RW>(r, sum, zeros);
                        if (lane == 0) match[a * h + b] = same, usum[a * h + b] = sum, uzero[a * h + b] = (int32_t)zeros;
                    }
            }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------
struct SkPlan {
    int np, rw;            // n_perm / 64, m_reg / 256
    int64_t W;             // words per row
    int64_t wave_max, group_max, seg;
    int64_t cap_group, cap_rows, cap_segs, bytes;
    int64_t off_group, off_rows, off_segs, off_partial;
};

static int sk_params(const tg_sketch_params *p, int64_t n, SkPlan &pl, const char *who) {
    TG_REQUIRE(p, "%s: null params", who);
    TG_REQUIRE(p->n_perm >= 64 && p->n_perm <= 256 && p->n_perm % 64 == 0, "%s: n_perm = %d is no multiple of 64 in [64, 256]", who,
               p->n_perm);
    TG_REQUIRE(p->hll_p >= 8 && p->hll_p <= 10, "%s: hll_p = %d outside [8, 10]", who, p->hll_p);
    TG_REQUIRE(p->hops >= 1 && p->hops <= TG_SKETCH_MAX_HOPS, "%s: hops = %d outside [1, %d]", who, p->hops, TG_SKETCH_MAX_HOPS);
    TG_REQUIRE(p->reserved == 0, "%s: reserved = %d is not 0", who, p->reserved);
    TG_REQUIRE(n >= 1 && n <= ((int64_t)1 << 31), "%s: n = %lld outside [1, 2^31]", who, (long long)n);
    pl.np = p->n_perm / 64, pl.rw = 1 << (p->hll_p - 8);
    pl.W = 64 * (int64_t)(pl.np + pl.rw);
    return TG_OK;
}

static int64_t sk_over(int64_t n, int64_t n_edges, int64_t t) { return std::min(n, n_edges / (t + 1)); }

static int sk_plan(const tg_sketch_params *p, int64_t n, int64_t n_edges, int32_t form, const tg_sketch_tuning *tuning, SkPlan &pl,
                   const char *who) {
    if (const int rc = sk_params(p, n, pl, who)) return rc;
    TG_REQUIRE(n_edges >= 0, "%s: n_edges = %lld is negative", who, (long long)n_edges);
    TG_REQUIRE(form >= TG_SKETCH_FORM_AUTO && form <= TG_SKETCH_FORM_SPLIT, "%s: unknown form %d", who, form);
    const int64_t wm = tuning ? tuning->wave_max : 0, gm = tuning ? tuning->group_max : 0, sg = tuning ? tuning->split_seg : 0;
    TG_REQUIRE(wm >= 0 && wm <= (1 << 30), "%s: wave_max = %lld outside [0, 2^30]", who, (long long)wm);
    TG_REQUIRE(gm >= 0 && gm <= (1 << 30), "%s: group_max = %lld outside [0, 2^30]", who, (long long)gm);
    TG_REQUIRE(sg == 0 || (sg >= TG_SKETCH_SPLIT_SEG_MIN && sg <= TG_SKETCH_SPLIT_SEG), "%s: split_seg = %lld outside [%d, %d]", who,
               (long long)sg, TG_SKETCH_SPLIT_SEG_MIN, TG_SKETCH_SPLIT_SEG);
    pl.seg = sg ? sg : TG_SKETCH_SPLIT_SEG;
    pl.wave_max = pl.group_max = SK_NO_LIMIT;
    pl.cap_group = pl.cap_rows = pl.cap_segs = pl.bytes = 0;
    if (form == TG_SKETCH_FORM_AUTO) {
        pl.wave_max = wm ? wm : TG_SKETCH_WAVE_MAX;
        pl.group_max = std::max(gm ? gm : (int64_t)TG_SKETCH_GROUP_MAX, pl.wave_max);
        pl.cap_group = sk_over(n, n_edges, pl.wave_max);
        pl.cap_rows = sk_over(n, n_edges, pl.group_max);
    } else if (form == TG_SKETCH_FORM_SPLIT) {
        pl.wave_max = pl.group_max = 0; // every row with an entry
        pl.cap_rows = sk_over(n, n_edges, 0);
    }
    if (form == TG_SKETCH_FORM_AUTO || form == TG_SKETCH_FORM_SPLIT) {
        pl.cap_segs = pl.cap_rows + n_edges / pl.seg;
        TG_REQUIRE(pl.cap_segs < ((int64_t)1 << 32), "%s: %lld segments, fewer than 2^32 expected", who, (long long)pl.cap_segs);
        pl.off_group = 256;
        pl.off_rows = pl.off_group + sk_r256(4 * pl.cap_group);
        pl.off_segs = pl.off_rows + sk_r256(8 * pl.cap_rows);
        pl.off_partial = pl.off_segs + sk_r256(8 * pl.cap_segs);
        pl.bytes = pl.off_partial + pl.cap_segs * pl.W * 4; // < 2^32 x 2^11 + 3 x 2^35
    }
    return TG_OK;
}

// calls f.template operator()<NP, RW>() for the plan's sizes
#define SK_DISPATCH(pl, CALL)                                                                                          \
    do {                                                                                                               \
        switch ((pl).np * 8 + (pl).rw) {                                                                               \
        case 1 * 8 + 1: { CALL(1, 1); } break;                                                                         \
        case 1 * 8 + 2: { CALL(1, 2); } break;                                                                         \
        case 1 * 8 + 4: { CALL(1, 4); } break;                                                                         \
        case 2 * 8 + 1: { CALL(2, 1); } break;                                                                         \
        case 2 * 8 + 2: { CALL(2, 2); } break;                                                                         \
        case 2 * 8 + 4: { CALL(2, 4); } break;                                                                         \
        case 3 * 8 + 1: { CALL(3, 1); } break;                                                                         \
        case 3 * 8 + 2: { CALL(3, 2); } break;                                                                         \
        case 3 * 8 + 4: { CALL(3, 4); } break;                                                                         \
        case 4 * 8 + 1: { CALL(4, 1); } break;                                                                         \
        case 4 * 8 + 2: { CALL(4, 2); } break;                                                                         \
        default: { CALL(4, 4); } break;                                                                                \
        }                                                                                                              \
    } while (0)

static unsigned sk_wave_grid(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + SK_WAVES - 1) / SK_WAVES, TG_SKETCH_WAVE_GROUPS));
}
static unsigned sk_group_grid(int64_t items) { return (unsigned)std::min<int64_t>(items, TG_SKETCH_GROUP_GROUPS); }

} // namespace tg

extern "C" int tg_sketch_bytes(const tg_sketch_params *p, int64_t n, int64_t *bytes, int64_t *row_words) {
    tg::SkPlan pl;
    TG_REQUIRE(bytes, "tg_sketch_bytes: null bytes");
    if (const int rc = tg::sk_params(p, n, pl, "tg_sketch_bytes")) return rc;
    *bytes = (int64_t)(p->hops + 1) * n * pl.W * 4;
    if (row_words) *row_words = pl.W;
    return TG_OK;
}

extern "C" int tg_sketch_init(const tg_sketch_params *p, int64_t n, uint32_t *sketch, void *stream) {
    using namespace tg;
    const char *who = "tg_sketch_init";
    SkPlan pl;
    if (const int rc = sk_params(p, n, pl, who)) return rc;
    TG_REQUIRE(sketch, "%s: null sketch", who);
    TG_REQUIRE(((uintptr_t)sketch & 15u) == 0, "%s: the sketch must be 16-byte aligned", who);
    const int units = (int)(pl.W / 4);
    const unsigned grid = (unsigned)std::min<int64_t>((n * units + SK_THREADS - 1) / SK_THREADS, 64 * 1024);
    hipLaunchKernelGGL(sk_init_kernel, dim3(grid), dim3(SK_THREADS), 0, (hipStream_t)stream, reinterpret_cast<uint4 *>(sketch), n,
                       p->n_perm / 4, units, (1u << p->hll_p) - 1u, (uint32_t)p->seed, (uint32_t)(p->seed >> 32));
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_sketch_propagate_workspace_bytes(const tg_sketch_params *p, int64_t n, int64_t n_edges, int32_t form,
                                                   const tg_sketch_tuning *tuning, int64_t *bytes, int32_t *form_taken) {
    tg::SkPlan pl;
    TG_REQUIRE(bytes, "tg_sketch_propagate_workspace_bytes: null bytes");
    if (const int rc = tg::sk_plan(p, n, n_edges, form, tuning, pl, "tg_sketch_propagate_workspace_bytes")) return rc;
    *bytes = pl.bytes;
    if (form_taken) *form_taken = form;
    return TG_OK;
}

extern "C" int tg_sketch_propagate(const tg_graph *g, const tg_sketch_params *p, const uint32_t *prev, uint32_t *next, int32_t form,
                                   const tg_sketch_tuning *tuning, int32_t *status, void *workspace, int64_t workspace_bytes,
                                   void *stream_) {
    using namespace tg;
    const char *who = "tg_sketch_propagate";
    TG_REQUIRE(g, "%s: null graph", who);
    SkPlan pl;
    if (const int rc = sk_plan(p, g->n_major, g->n_edges, form, tuning, pl, who)) return rc;
    TG_REQUIRE(g->ptrs && (g->indices || g->n_edges == 0), "%s: null graph arrays", who);
    TG_REQUIRE(prev && next && status, "%s: null prev / next / status", who);
    TG_REQUIRE((((uintptr_t)prev | (uintptr_t)next) & 15u) == 0, "%s: prev and next must be 16-byte aligned", who);
    const int64_t n = g->n_major, hop_bytes = n * pl.W * 4;
    TG_REQUIRE((uintptr_t)prev + hop_bytes <= (uintptr_t)next || (uintptr_t)next + hop_bytes <= (uintptr_t)prev,
               "%s: prev and next overlap", who);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(pl.bytes == 0 || (workspace && workspace_bytes >= pl.bytes), "%s: the workspace has %lld bytes, the call needs %lld",
               who, (long long)(workspace ? workspace_bytes : 0), (long long)pl.bytes);
    TG_REQUIRE(pl.bytes == 0 || ((uintptr_t)workspace & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);

    SkProp a;
    a.g = CsrView{g->ptrs, g->indices, g->ptrs32, g->indices32, nullptr, 0};
    a.n = n, a.n_edges = g->n_edges, a.prev = prev, a.next = next, a.status = status;
    a.wave_max = pl.wave_max, a.group_max = pl.group_max, a.seg = pl.seg;
    a.cap_group = pl.cap_group, a.cap_rows = pl.cap_rows, a.cap_segs = pl.cap_segs;
    char *ws = static_cast<char *>(workspace);
    a.counters = a.group_list = a.partial = nullptr, a.row_list = a.seg_list = nullptr;
    if (pl.bytes) {
        a.counters = reinterpret_cast<uint32_t *>(ws);
        a.group_list = reinterpret_cast<uint32_t *>(ws + pl.off_group);
        a.row_list = reinterpret_cast<uint2 *>(ws + pl.off_rows);
        a.seg_list = reinterpret_cast<uint2 *>(ws + pl.off_segs);
        a.partial = reinterpret_cast<uint32_t *>(ws + pl.off_partial);
    }
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 block(SK_THREADS);
    if (pl.bytes) hipLaunchKernelGGL(sk_clear_kernel, dim3(1), dim3(1), 0, stream, a.counters);
#define SK_PROPAGATE(NP, RW)                                                                                           \
    if (form != TG_SKETCH_FORM_GROUP)                                                                                  \
        hipLaunchKernelGGL((sk_wave_kernel<NP, RW>), dim3(sk_wave_grid(n)), block, 0, stream, a);                      \
    else                                                                                                               \
        hipLaunchKernelGGL((sk_group_kernel<NP, RW>), dim3(sk_group_grid(n)), block, 0, stream, a, (int)SK_ROWS_ALL);  \
    if (pl.cap_group > 0)                                                                                              \
        hipLaunchKernelGGL((sk_group_kernel<NP, RW>), dim3(sk_group_grid(pl.cap_group)), block, 0, stream, a,          \
                           (int)SK_ROWS_LISTED);                                                                       \
    if (pl.cap_rows > 0) {                                                                                             \
        hipLaunchKernelGGL((sk_group_kernel<NP, RW>), dim3(sk_group_grid(pl.cap_segs)), block, 0, stream, a,           \
                           (int)SK_SEGMENTS);                                                                          \
        hipLaunchKernelGGL((sk_combine_kernel<NP, RW>), dim3(sk_wave_grid(pl.cap_rows)), block, 0, stream, a);         \
    }
    SK_DISPATCH(pl, SK_PROPAGATE);
#undef SK_PROPAGATE
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_sketch_links(const tg_sketch_params *p, int64_t n, const uint32_t *sketch, const int64_t *src, const int64_t *dst,
                               const tg_sketch_link_out *out, int64_t m, int32_t *status, void *stream) {
    using namespace tg;
    const char *who = "tg_sketch_links";
    SkPlan pl;
    if (const int rc = sk_params(p, n, pl, who)) return rc;
    TG_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "%s: m = %lld outside [0, 2^31)", who, (long long)m);
    TG_REQUIRE(out, "%s: null out", who);
    if (m == 0) return TG_OK; // nothing to launch
    TG_REQUIRE(sketch && src && dst && status, "%s: null sketch / src / dst / status", who);
    TG_REQUIRE(out->match && out->usum && out->uzero && out->nsum && out->nzero, "%s: null match / usum / uzero / nsum / nzero", who);
    TG_REQUIRE(((uintptr_t)sketch & 15u) == 0, "%s: the sketch must be 16-byte aligned", who);
    SkLinks a;
    a.sketch = sketch, a.src = src, a.dst = dst, a.n = n, a.m = m, a.h = p->hops;
    a.match = out->match, a.uzero = out->uzero, a.nzero = out->nzero, a.usum = out->usum, a.nsum = out->nsum, a.status = status;
#define SK_LINKS(NP, RW)                                                                                               \
    hipLaunchKernelGGL((sk_links_kernel<NP, RW>), dim3(sk_wave_grid(m)), dim3(SK_THREADS), 0, (hipStream_t)stream, a)
    SK_DISPATCH(pl, SK_LINKS);
#undef SK_LINKS
    TG_LAUNCH_CHECK();
    return TG_OK;
}
