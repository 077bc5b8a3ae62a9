// Streaming last-k neighbour state (include/tchgeo_lastn.h): a ring of k {nbr, e_id} slots per node behind
// a 64-bit count, fed by tg_lastn_insert and read by tg_lastn_sample behind tg_ns_homo_batched's output contract.
//   reset    16-byte stores over the whole state
//   insert   the rank of an entry among the call's entries of its node decides its slot, so nothing depends on scheduling:
//            LDS form   one workgroup sorts the packed words (node << 23 | entry index) with a bitonic network in LDS; a
//                       node's entries are one run, found by two binary searches; the old counts are read before a
//                       barrier and the new ones written behind it
//            grid form  a table keyed by node (open addressing, 64-bit compare-and-swap, at most half full) holds the
//                       call's entry count and newest entry index per node; round j then names every node's j-th newest
//                       entry as the maximum over the indices below round j - 1's (three rotating arrays: read, raised,
//                       cleared); the counts are written by a launch of their own, behind every reader of the old ones
//   sample   one workgroup per batch walks the hops: 256 frontier vertices at a time, their counts scanned with DPP adds
//            and four wave totals in LDS, then a lane per (vertex, slot) in groups of the next power of two >= fan-out
//            loads its 16-byte slot and stores the sample, the parent and the e_id at its scanned place
//   replay   the host loop of sample + insert launches of one call; no kernel waits on another
#include <algorithm>

#include "tg_device.h"
#include "tg_host.h"

#include "../../include/tchgeo_lastn.h"

namespace tg {

constexpr int LN_IDX_BITS = 23; // an insert has at most 2^23 entries
constexpr uint64_t LN_NO_KEY = ~0ull;
constexpr int LN_SAMPLE_THREADS = 256;

struct LnSlot {
    int64_t nbr, e_id;
};

struct LnState {
    int64_t *count;
    int4 *slots; // 16 bytes each: {nbr, e_id}
    int64_t n_nodes;
    int32_t k;
};

__host__ __device__ inline int64_t ln_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

__device__ __forceinline__ int4 ln_pack(int64_t nbr, int64_t e_id) {
    return make_int4((int)(uint32_t)nbr, (int)(uint32_t)((uint64_t)nbr >> 32), (int)(uint32_t)e_id,
                     (int)(uint32_t)((uint64_t)e_id >> 32));
}
__device__ __forceinline__ LnSlot ln_unpack(int4 w) {
    LnSlot s;
    s.nbr = (int64_t)((uint64_t)(uint32_t)w.x | ((uint64_t)(uint32_t)w.y << 32));
    s.e_id = (int64_t)((uint64_t)(uint32_t)w.z | ((uint64_t)(uint32_t)w.w << 32));
    return s;
}

// ---- reset ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lastn_reset_kernel(int4 *state, int64_t count_units, int64_t total_units) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total_units; u += (int64_t)gridDim.x * blockDim.x)
        state[u] = u < count_units ? make_int4(0, 0, 0, 0) : make_int4(-1, -1, -1, -1);
}

// ---- insert --------------------------------------------------------------------------------------------------------
struct LnInsert {
    LnState st;
    const int64_t *src, *dst, *e_id;
    int64_t e_base;
    int32_t n_entries; // events, or 2 * events under `symmetric`
    int32_t symmetric;
    int32_t *status;
    // grid form
    int64_t *keys;
    int32_t *last, *m_in, *m_out, *m_clear, *cnt, *slot_of;
    int32_t table_mask, table_shift, round;
};

__device__ __forceinline__ int64_t ln_entry_node(const LnInsert &p, int32_t i) {
    if (!p.symmetric) return p.dst[i];
    return (i & 1) ? p.src[i >> 1] : p.dst[i >> 1];
}
__device__ __forceinline__ void ln_entry_store(const LnInsert &p, int32_t i, int64_t node, int64_t ring_pos) {
    const int64_t j = p.symmetric ? (i >> 1) : i;
    const int64_t nbr = (p.symmetric && (i & 1)) ? p.dst[j] : p.src[j];
    const int64_t e = p.e_id ? p.e_id[j] : p.e_base + j;
    p.st.slots[node * p.st.k + ring_pos] = ln_pack(nbr, e);
}

__device__ __forceinline__ int ln_lower_bound(const uint64_t *keys, int n, uint64_t x) { // first position with keys[.] >= x
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one workgroup; P = the power of two >= n_entries (at least 64) words of dynamic LDS
__global__ void __launch_bounds__(1024) lastn_insert_lds_kernel(const LnInsert p, const int P) {
    extern __shared__ uint64_t ln_keys[];
    const int tid = threadIdx.x, nt = blockDim.x;
    bool bad = false;
    for (int i = tid; i < P; i += nt) {
        uint64_t key = LN_NO_KEY;
        if (i < p.n_entries) {
            const int64_t node = ln_entry_node(p, i);
            if ((uint64_t)node < (uint64_t)p.st.n_nodes) key = ((uint64_t)node << LN_IDX_BITS) | (uint64_t)i;
            else bad = true;
        }
        ln_keys[i] = key;
    }
    if (bad) atomicOr((int *)p.status, 2);
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (P >> 1); t += nt) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t a = ln_keys[i], b = ln_keys[j];
                if ((a > b) == ((i & size) == 0)) {
                    ln_keys[i] = b;
                    ln_keys[j] = a;
                }
            }
        }
    __syncthreads();
    // a thread holds at most 4096 / 64 positions; the runs' new counts wait in LDS-free registers only for P / nt <= 4,
    // so the pass is repeated instead: it is two binary searches
    for (int pass = 0; pass < 2; ++pass) {
        for (int q = tid; q < P; q += nt) {
            const uint64_t key = ln_keys[q];
            if (key == LN_NO_KEY) continue;
            const int64_t node = (int64_t)(key >> LN_IDX_BITS);
            const int32_t i = (int32_t)(key & ((1u << LN_IDX_BITS) - 1));
            const int end = ln_lower_bound(ln_keys, P, (uint64_t)(node + 1) << LN_IDX_BITS);
            if (pass == 1) { // behind the barrier: every reader of the old count is done
                if (q == end - 1) {
                    const int begin = ln_lower_bound(ln_keys, P, (uint64_t)node << LN_IDX_BITS);
                    p.st.count[node] += end - begin;
                }
                continue;
            }
            if (end - q > p.st.k) continue; // rank < c - k: overwritten by a later entry of this call
            const int begin = ln_lower_bound(ln_keys, P, (uint64_t)node << LN_IDX_BITS);
            const uint64_t n = (uint64_t)p.st.count[node];
            ln_entry_store(p, i, node, (int64_t)((n + (uint64_t)(q - begin)) % (uint64_t)p.st.k));
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t ln_hash(int64_t node, int shift) {
    return (uint32_t)(((uint64_t)node * 0x9E3779B97F4A7C15ull) >> shift);
}

__global__ void __launch_bounds__(256) lastn_grid_build_kernel(const LnInsert p) {
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= p.n_entries) return;
    const int32_t i = (int32_t)i64;
    const int64_t node = ln_entry_node(p, i);
    if ((uint64_t)node >= (uint64_t)p.st.n_nodes) {
        p.slot_of[i] = -1;
        atomicOr((int *)p.status, 2);
        return;
    }
    uint32_t h = ln_hash(node, p.table_shift) & (uint32_t)p.table_mask;
    // the table has at least twice as many places as the call has entries: the probe ends
    for (int32_t step = 0; step <= p.table_mask; ++step) {
        const unsigned long long prev = atomicCAS((unsigned long long *)&p.keys[h], ~0ull, (unsigned long long)node);
        if (prev == ~0ull || prev == (unsigned long long)node) break;
        h = (h + 1) & (uint32_t)p.table_mask;
    }
    p.slot_of[i] = (int32_t)h;
    atomicAdd(&p.cnt[h], 1);
    atomicMax(&p.last[h], i);
}

// round j: m_in holds every node's j-th newest entry index of the call (-1: it has fewer), complete since the launch before
__global__ void __launch_bounds__(256) lastn_grid_round_kernel(const LnInsert p) {
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= p.n_entries) return;
    const int32_t i = (int32_t)i64;
    const int32_t s = p.slot_of[i];
    if (s < 0) return;
    const int32_t w = p.m_in[s];
    if (w < 0 || w == i) p.m_clear[s] = -1; // next round's target: read last in the round before this one
    if (w < 0) return;
    if (i < w) {
        atomicMax(&p.m_out[s], i);
        return;
    }
    if (i > w) return; // placed in an earlier round
    const int64_t node = p.keys[s];
    const uint64_t n = (uint64_t)p.st.count[node], c = (uint64_t)p.cnt[s];
    ln_entry_store(p, i, node, (int64_t)((n + c - 1 - (uint64_t)p.round) % (uint64_t)p.st.k));
}

__global__ void __launch_bounds__(256) lastn_grid_counts_kernel(const LnInsert p) {
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= p.n_entries) return;
    const int32_t i = (int32_t)i64;
    const int32_t s = p.slot_of[i];
    if (s < 0 || p.last[s] != i) return;
    p.st.count[p.keys[s]] += p.cnt[s];
}

// ---- sample --------------------------------------------------------------------------------------------------------
struct LnSample {
    LnState st;
    const int64_t *seeds;
    int64_t n_seeds, batch0;
    int32_t n_hops;
    int32_t fanout[TG_MAX_HOPS];
    int64_t cap_nodes, cap_edges;
    int64_t *samples, *rows /* NULL: prefilled */, *cols, *edge_index, *layer_offsets, *counts;
    int32_t *status;
};

__global__ void __launch_bounds__(LN_SAMPLE_THREADS) lastn_sample_kernel(const LnSample p) {
    constexpr int NT = LN_SAMPLE_THREADS;
    __shared__ uint32_t s_off[NT];  // exclusive prefix of the tile's contributions
    __shared__ int8_t s_c[NT];      // contribution of the vertex: min(fanout, count, k)
    __shared__ int8_t s_pos[NT];    // ring position of its newest entry
    __shared__ uint32_t s_wave[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = p.batch0 + blockIdx.x;
    int64_t *samples = p.samples + b * p.cap_nodes;
    int64_t *rows = p.rows ? p.rows + b * p.cap_edges : nullptr;
    int64_t *cols = p.cols + b * p.cap_edges;
    int64_t *eidx = p.edge_index + b * p.cap_edges;
    const int64_t *seeds = p.seeds + b * p.n_seeds;
    const int k = p.st.k;
    bool bad = false;
    for (int64_t i = tid; i < p.n_seeds; i += NT) {
        const int64_t s = seeds[i];
        samples[i] = s;
        bad |= (uint64_t)s >= (uint64_t)p.st.n_nodes;
    }
    if (bad) atomicOr((int *)p.status, 2);
    int64_t begin = 0, m = p.n_seeds, ne = 0;
    for (int h = 0; h < p.n_hops; ++h) {
        __syncthreads(); // the frontier (the hop before's samples) is written
        const int f = p.fanout[h];
        int lg = 0;
        while ((1 << lg) < f) ++lg;
        if (tid == 0) {
            int64_t *lo = p.layer_offsets + (b * p.n_hops + h) * 3;
            lo[0] = p.n_seeds + ne;
            lo[1] = ne;
            lo[2] = p.n_seeds + ne;
        }
        int64_t carry = 0; // edges of this hop before the tile
        for (int64_t base = 0; base < m; base += NT) {
            const int64_t vi = base + tid;
            int c = 0;
            if (vi < m) {
                const int64_t v = samples[begin + vi];
                if ((uint64_t)v < (uint64_t)p.st.n_nodes) {
                    const int64_t n = p.st.count[v];
                    if (n > 0) {
                        c = (int)min((int64_t)min(f, k), n);
                        s_pos[tid] = (int8_t)((uint64_t)(n - 1) % (uint64_t)k);
                    }
                }
            }
            const uint32_t incl = wave_inclusive_scan_u32_dpp((uint32_t)c);
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) {
                const uint32_t t = s_wave[w];
                if (w < wave) before += t;
                total += t;
            }
            s_off[tid] = before + incl - (uint32_t)c;
            s_c[tid] = (int8_t)c;
            __syncthreads();
            const int n_items = NT << lg;
            for (int j = tid; j < n_items; j += NT) {
                const int t = j >> lg, r = j & ((1 << lg) - 1);
                if (r >= s_c[t]) continue;
                int pos = (int)s_pos[t] - r; // newest first: entries count - 1, count - 2, ...
                if (pos < 0) pos += k;
                const int64_t v = samples[begin + base + t];
                const LnSlot e = ln_unpack(p.st.slots[v * k + pos]);
                const int64_t o = ne + carry + (int64_t)s_off[t] + r;
                samples[p.n_seeds + o] = e.nbr;
                if (rows) rows[o] = p.n_seeds + o;
                cols[o] = begin + base + t;
                eidx[o] = e.e_id;
            }
            carry += total;
            __syncthreads(); // the tile's LDS is free again
        }
        begin += m;
        m = carry;
        ne += carry;
    }
    if (tid == 0) {
        p.counts[b * 2] = p.n_seeds + ne;
        p.counts[b * 2 + 1] = ne;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static int ln_state_bytes(int64_t n_nodes, int32_t k, int64_t *bytes, const char *who) {
    TG_REQUIRE(k >= 1 && k <= TG_LASTN_MAX_K, "%s: k = %d outside [1, %d]", who, k, TG_LASTN_MAX_K);
    TG_REQUIRE(n_nodes >= 1 && n_nodes <= TG_LASTN_MAX_NODES, "%s: n_nodes = %lld outside [1, 2^31]", who, (long long)n_nodes);
    *bytes = ln_r256(8 * n_nodes) + 16 * n_nodes * k;
    return TG_OK;
}

static int ln_state(const tg_lastn *st, LnState *s, const char *who) {
    TG_REQUIRE(st && st->state, "%s: null state", who);
    int64_t need = 0;
    const int rc = ln_state_bytes(st->n_nodes, st->k, &need, who);
    if (rc != TG_OK) return rc;
    TG_REQUIRE(st->state_bytes >= need, "%s: state_bytes = %lld below the %lld of %lld nodes with k = %d", who,
               (long long)st->state_bytes, (long long)need, (long long)st->n_nodes, st->k);
    TG_REQUIRE(((uintptr_t)st->state & 15u) == 0, "%s: the state must be 16-byte aligned", who);
    s->count = (int64_t *)st->state;
    s->slots = (int4 *)((char *)st->state + ln_r256(8 * st->n_nodes));
    s->n_nodes = st->n_nodes;
    s->k = st->k;
    return TG_OK;
}

struct LnGridPlan {
    int64_t table, bytes;
    int shift;
};
static LnGridPlan ln_grid_plan(int64_t entries) {
    LnGridPlan g;
    g.table = 64;
    g.shift = 64 - 6;
    while (g.table < 2 * entries) {
        g.table <<= 1;
        --g.shift;
    }
    g.bytes = ln_r256(8 * g.table) + 5 * ln_r256(4 * g.table) + ln_r256(4 * entries);
    return g;
}

// the form a call takes and its workspace; entries = events (x 2 under symmetric)
static int ln_insert_plan(int64_t n_events, int32_t symmetric, int32_t form, int64_t *entries, int32_t *taken, int64_t *bytes,
                          const char *who) {
    TG_REQUIRE(n_events >= 0 && n_events <= TG_LASTN_MAX_EVENTS, "%s: n_events = %lld outside [0, 2^22]", who,
               (long long)n_events);
    TG_REQUIRE(form >= TG_LASTN_FORM_AUTO && form <= TG_LASTN_FORM_GRID, "%s: unknown form %d", who, form);
    *entries = n_events * (symmetric ? 2 : 1);
    TG_REQUIRE(form != TG_LASTN_FORM_LDS || *entries <= TG_LASTN_LDS_ENTRIES,
               "%s: %lld entries exceed the LDS form's %d", who, (long long)*entries, TG_LASTN_LDS_ENTRIES);
    *taken = form != TG_LASTN_FORM_AUTO ? form : (*entries <= TG_LASTN_LDS_ENTRIES ? TG_LASTN_FORM_LDS : TG_LASTN_FORM_GRID);
    *bytes = *taken == TG_LASTN_FORM_GRID ? ln_grid_plan(*entries).bytes : 0;
    return TG_OK;
}

// everything is validated by the caller
static int ln_insert_launch(const LnState &s, const int64_t *src, const int64_t *dst, const int64_t *e_id, int64_t e_base,
                            int64_t entries, int32_t symmetric, int32_t taken, int32_t *status, void *ws, hipStream_t stream) {
    if (entries == 0) return TG_OK;
    LnInsert p = {};
    p.st = s;
    p.src = src;
    p.dst = dst;
    p.e_id = e_id;
    p.e_base = e_base;
    p.n_entries = (int32_t)entries;
    p.symmetric = symmetric ? 1 : 0;
    p.status = status;
    if (taken == TG_LASTN_FORM_LDS) {
        int P = 64;
        while (P < entries) P <<= 1;
        const int threads = std::min(1024, std::max(64, P / 2));
        hipLaunchKernelGGL(lastn_insert_lds_kernel, dim3(1), dim3(threads), (size_t)P * 8, stream, p, P);
        TG_LAUNCH_CHECK();
        return TG_OK;
    }
    const LnGridPlan g = ln_grid_plan(entries);
    char *w = (char *)ws;
    p.keys = (int64_t *)w;
    w += ln_r256(8 * g.table);
    int32_t *m[3];
    p.last = (int32_t *)w;
    w += ln_r256(4 * g.table);
    for (int j = 0; j < 3; ++j) {
        m[j] = (int32_t *)w;
        w += ln_r256(4 * g.table);
    }
    const int64_t ones = w - (char *)ws; // keys, last and the three round arrays start at -1
    p.cnt = (int32_t *)w;
    w += ln_r256(4 * g.table);
    p.slot_of = (int32_t *)w;
    p.table_mask = (int32_t)(g.table - 1);
    p.table_shift = g.shift;
    TG_HIP(hipMemsetAsync(ws, 0xFF, (size_t)ones, stream));
    TG_HIP(hipMemsetAsync(p.cnt, 0, (size_t)(4 * g.table), stream));
    const dim3 grid((unsigned)((entries + 255) / 256)), block(256);
    hipLaunchKernelGGL(lastn_grid_build_kernel, grid, block, 0, stream, p);
    for (int j = 0; j < s.k; ++j) {
        p.round = j;
        p.m_in = j == 0 ? p.last : m[(j - 1) % 3];
        p.m_out = m[j % 3];
        p.m_clear = m[(j + 1) % 3];
        hipLaunchKernelGGL(lastn_grid_round_kernel, grid, block, 0, stream, p);
    }
    hipLaunchKernelGGL(lastn_grid_counts_kernel, grid, block, 0, stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

static int ln_sample_check(const LnState &s, const int64_t *seeds, int64_t n_batches, int64_t n_seeds, const int64_t *fanout,
                           int32_t n_hops, const tg_ns_out *out, const int32_t *status, LnSample *p, const char *who) {
    TG_REQUIRE(out && status, "%s: null out / status", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff && n_seeds >= 0, "%s: bad sizes", who);
    TG_REQUIRE(n_hops >= 0 && n_hops <= TG_MAX_HOPS, "%s: n_hops %d outside [0, %d]", who, n_hops, TG_MAX_HOPS);
    TG_REQUIRE(fanout || n_hops == 0, "%s: null fanout", who);
    TG_REQUIRE(seeds || n_seeds == 0 || n_batches == 0, "%s: null seeds", who);
    for (int h = 0; h < n_hops; ++h)
        TG_REQUIRE(fanout[h] >= 1 && fanout[h] <= s.k, "%s: fanout[%d] = %lld outside [1, k = %d]", who, h,
                   (long long)fanout[h], s.k);
    int64_t need_nodes = 0, need_edges = 0;
    const int rc = tg_ns_homo_capacity(n_seeds, fanout, n_hops, &need_nodes, &need_edges);
    if (rc != TG_OK) return rc;
    TG_REQUIRE(out->samples && out->counts && (out->layer_offsets || n_hops == 0), "%s: null output buffers", who);
    TG_REQUIRE(out->cap_nodes >= need_nodes && out->cap_edges >= need_edges,
               "%s: output slabs too small (need %lld nodes / %lld edges per batch)", who, (long long)need_nodes,
               (long long)need_edges);
    TG_REQUIRE(need_edges == 0 || (out->rows && out->cols && out->edge_index), "%s: null edge output buffers", who);
    *p = LnSample{};
    p->st = s;
    p->seeds = seeds;
    p->n_seeds = n_seeds;
    p->n_hops = n_hops;
    for (int h = 0; h < n_hops; ++h) p->fanout[h] = (int32_t)fanout[h];
    p->cap_nodes = out->cap_nodes;
    p->cap_edges = out->cap_edges;
    p->samples = out->samples;
    p->rows = ns_rows_prefilled(out, n_seeds) ? nullptr : out->rows;
    p->cols = out->cols;
    p->edge_index = out->edge_index;
    p->layer_offsets = out->layer_offsets;
    p->counts = out->counts;
    p->status = const_cast<int32_t *>(status);
    return TG_OK;
}

} // namespace tg

extern "C" int tg_lastn_state_bytes(int64_t n_nodes, int32_t k, int64_t *bytes) {
    TG_REQUIRE(bytes, "tg_lastn_state_bytes: null bytes");
    return tg::ln_state_bytes(n_nodes, k, bytes, "tg_lastn_state_bytes");
}

extern "C" int tg_lastn_reset(const tg_lastn *st, void *stream) {
    using namespace tg;
    LnState s;
    const int rc = ln_state(st, &s, "tg_lastn_reset");
    if (rc != TG_OK) return rc;
    const int64_t count_units = ln_r256(8 * s.n_nodes) / 16, total = count_units + s.n_nodes * s.k;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(lastn_reset_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (int4 *)st->state,
                       count_units, total);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_lastn_insert_workspace_bytes(int64_t n_events, int32_t symmetric, int32_t form, int64_t *bytes,
                                               int32_t *form_taken) {
    TG_REQUIRE(bytes, "tg_lastn_insert_workspace_bytes: null bytes");
    int64_t entries = 0;
    int32_t taken = 0;
    const int rc = tg::ln_insert_plan(n_events, symmetric, form, &entries, &taken, bytes, "tg_lastn_insert_workspace_bytes");
    if (rc == TG_OK && form_taken) *form_taken = taken;
    return rc;
}

extern "C" int tg_lastn_insert(const tg_lastn *st, const int64_t *src, const int64_t *dst, const int64_t *e_id,
                               int64_t e_base, int64_t n_events, int32_t symmetric, int32_t *status, void *workspace,
                               int64_t workspace_bytes, int32_t form, void *stream) {
    using namespace tg;
    LnState s;
    int rc = ln_state(st, &s, "tg_lastn_insert");
    if (rc != TG_OK) return rc;
    int64_t entries = 0, need = 0;
    int32_t taken = 0;
    rc = ln_insert_plan(n_events, symmetric, form, &entries, &taken, &need, "tg_lastn_insert");
    if (rc != TG_OK) return rc;
    TG_REQUIRE(status, "tg_lastn_insert: null status");
    TG_REQUIRE((src && dst) || n_events == 0, "tg_lastn_insert: null src / dst");
    TG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "tg_lastn_insert: the workspace has %lld bytes, the call needs %lld",
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(need == 0 || ((uintptr_t)workspace & 7u) == 0, "tg_lastn_insert: the workspace must be 8-byte aligned");
    return ln_insert_launch(s, src, dst, e_id, e_base, entries, symmetric, taken, status, workspace, (hipStream_t)stream);
}

extern "C" int tg_lastn_sample(const tg_lastn *st, const int64_t *seeds, int64_t n_batches, int64_t n_seeds,
                               const int64_t *fanout, int32_t n_hops, const tg_ns_out *out, int32_t *status, void *stream) {
    using namespace tg;
    LnState s;
    int rc = ln_state(st, &s, "tg_lastn_sample");
    if (rc != TG_OK) return rc;
    LnSample p;
    rc = ln_sample_check(s, seeds, n_batches, n_seeds, fanout, n_hops, out, status, &p, "tg_lastn_sample");
    if (rc != TG_OK) return rc;
    if (n_batches == 0) return TG_OK;
    hipLaunchKernelGGL(lastn_sample_kernel, dim3((unsigned)n_batches), dim3(LN_SAMPLE_THREADS), 0, (hipStream_t)stream, p);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

extern "C" int tg_lastn_replay_workspace_bytes(int64_t step_events, int64_t *bytes) {
    TG_REQUIRE(bytes, "tg_lastn_replay_workspace_bytes: null bytes");
    TG_REQUIRE(step_events >= 1, "tg_lastn_replay_workspace_bytes: step_events = %lld must be >= 1", (long long)step_events);
    int64_t entries = 0;
    int32_t taken = 0;
    return tg::ln_insert_plan(step_events, 1, TG_LASTN_FORM_AUTO, &entries, &taken, bytes, "tg_lastn_replay_workspace_bytes");
}

extern "C" int tg_lastn_replay(const tg_lastn *st, const int64_t *src, const int64_t *dst, int64_t e_base, int64_t n_events,
                               int64_t step_events, const int64_t *seeds, int64_t n_seeds, const int64_t *fanout,
                               int32_t n_hops, const tg_ns_out *out, int32_t *status, void *workspace,
                               int64_t workspace_bytes, void *stream) {
    using namespace tg;
    LnState s;
    int rc = ln_state(st, &s, "tg_lastn_replay");
    if (rc != TG_OK) return rc;
    TG_REQUIRE(n_events >= 0 && n_events <= TG_LASTN_MAX_EVENTS, "tg_lastn_replay: n_events = %lld outside [0, 2^22]",
               (long long)n_events);
    TG_REQUIRE(step_events >= 1, "tg_lastn_replay: step_events = %lld must be >= 1", (long long)step_events);
    const int64_t step = std::min(step_events, std::max<int64_t>(n_events, 1)), G = (n_events + step - 1) / step;
    int64_t entries = 0, need = 0;
    int32_t taken = 0;
    rc = ln_insert_plan(step, 1, TG_LASTN_FORM_AUTO, &entries, &taken, &need, "tg_lastn_replay");
    if (rc != TG_OK) return rc;
    TG_REQUIRE((src && dst) || n_events == 0, "tg_lastn_replay: null src / dst");
    LnSample p;
    rc = ln_sample_check(s, seeds, G, n_seeds, fanout, n_hops, out, status, &p, "tg_lastn_replay");
    if (rc != TG_OK) return rc;
    TG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "tg_lastn_replay: the workspace has %lld bytes, the call needs %lld",
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
    TG_REQUIRE(need == 0 || ((uintptr_t)workspace & 7u) == 0, "tg_lastn_replay: the workspace must be 8-byte aligned");
    if (G == 0) return TG_OK;
    for (int64_t g = 0; g < G; ++g) {
        p.batch0 = g;
        hipLaunchKernelGGL(lastn_sample_kernel, dim3(1), dim3(LN_SAMPLE_THREADS), 0, (hipStream_t)stream, p);
        const int64_t e0 = g * step, n = std::min(step, n_events - e0);
        rc = ln_insert_launch(s, src + e0, dst + e0, nullptr, e_base + e0, 2 * n, 1, taken, status, workspace,
                              (hipStream_t)stream);
        if (rc != TG_OK) return rc;
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}
