// What the node dedup operators share (ns_unique.hip: tg_ns_homo_unique and tg_ns_homo_unique_grouped, ns_unique_typed.hip:
// tg_ns_typed_unique; saint_dedup.h takes the sizes, the insert, the scans and the plan, and so does chunk_scan.h for the
// induced, cluster and full-neighbour pairs, which adds what those three share among themselves: the chunk sizes, the
// find probe, the clear, the prefix over tiles of chunks, the unit rules and the host's checks, answer and round loop):
// the sizes, the open-addressing insert (atomicCAS claims the key; the caller's atomicMin of the position into the slot's
// value leaves the id's first position there; its masked variant came from ns_full.hip), the workgroup rank scan, the flat
// form's clear, flag and apply bodies as device function templates, the host's LDS limit query and raise, the plan, and
// the probe's mask and shift of a table capacity (nsu_mask_shift, once written out at five sites).
//
// The tile bodies take what differs from their caller: the view of a list's tables, what else to store for a first
// occurrence, and they hand back the ranks for the caller's own counts (counts, layer_nodes, seed_counts).  The __global__
// shells, their grids and their argument structs stay in the .hip files, so the code of a kernel does not depend on who
// else includes this header.  The insert, the edge relabel and the LDS form are NOT here: as functions they compile to
// other code than tg_ns_homo_unique's kernels had (the compiler simplifies a callee before it knows the caller's tile
// origin), and those kernels are held to their instruction streams (tools/kernel_diff.py).
#pragma once
#include <atomic>

#include "tg_host.h"
#include "tg_map.h"

namespace tg {

constexpr int NSU_THREADS = 1024;       // LDS form: the widest workgroup
constexpr int NSU_MAX_PER_THREAD = 32;  // positions a thread owns in the LDS form's scan: its flags are one 32-bit mask
constexpr int64_t NSU_LDS_MAX_NODES = (int64_t)NSU_THREADS * NSU_MAX_PER_THREAD; // 32 768: slots and local ids fit u16
constexpr int NSU_STATIC_LDS = 256;     // wave totals (upper bound)
constexpr int NSU_TILE_THREADS = 256;   // flat form: a block owns a tile of positions, a thread NSU_PER consecutive ones
constexpr int NSU_PER = 4;
constexpr int NSU_TILE = NSU_TILE_THREADS * NSU_PER;
constexpr int NSU_EDGE_PER = 8;         // edges a thread relabels
constexpr int NSU_EDGE_TILE = NSU_TILE_THREADS * NSU_EDGE_PER;
constexpr int64_t NSU_MAX_NODES = (int64_t)1 << 30; // positions and slots are 31-bit words
constexpr int64_t NSU_ROUND_MAX = 32768;            // batches per round (grid.y)
constexpr uint32_t NSU_FLAG = 0x80000000u;          // flat form: bit 31 of a position's slot word = first occurrence
constexpr uint32_t NSU_UNSEEN = 0xFFFFFFFFu;

typedef unsigned int nsu_k32;
typedef unsigned long long nsu_k64;

template <typename K> __device__ __forceinline__ K nsu_empty() { return (K)~(K)0; } // no id: ids are in [0, id_bound)
__device__ __forceinline__ uint32_t nsu_hash(nsu_k32 key, uint32_t mask, uint32_t shift) {
    return (key * 0x9E3779B1u) >> shift;
}
__device__ __forceinline__ uint32_t nsu_hash(nsu_k64 key, uint32_t mask, uint32_t shift) {
    return (uint32_t)map_hash((int64_t)key) & mask;
}
// claims (or finds) the slot of `key`; at most one pass over the table.  MASKED: the hash is masked as well, for a table
// that may have one slot (its shift is 32; the full-neighbour pair's node_cap = 0)
template <typename K, bool MASKED = false>
__device__ __forceinline__ uint32_t nsu_insert(K *keys, uint32_t mask, uint32_t shift, K key) {
    uint32_t s = MASKED ? nsu_hash(key, mask, shift & 31u) & mask : nsu_hash(key, mask, shift);
    for (uint32_t i = 0; i <= mask; ++i) {
        const K prev = atomicCAS(&keys[s], nsu_empty<K>(), key);
        if (prev == nsu_empty<K>() || prev == key) break;
        s = (s + 1) & mask;
    }
    return s;
}

// exclusive prefix of `cnt` over the threads of the workgroup in thread order, *total = the sum.  Every thread calls it.
__device__ __forceinline__ uint32_t nsu_scan(uint32_t cnt, uint32_t *s_wave, uint32_t *total) {
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

// exclusive prefix of `v` over the threads of the workgroup in thread order, *total = the sum.  Every thread calls it.  The 64-bit
// form of nsu_scan: the induced pairs' chunk prefixes and tg_cluster_*'s plan step.
__device__ __forceinline__ unsigned long long nsu_scan64(unsigned long long v, unsigned long long *s_wave,
                                                         unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long carry = 0, sum = 0;
    for (int w = 0; w < n_waves; ++w) {
        const unsigned long long x = s_wave[w];
        sum += x;
        if (w < wave) carry += x;
    }
    __syncthreads(); // s_wave is free again
    *total = sum;
    return carry + incl - v;
}

__device__ __forceinline__ int64_t nsu_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// the local id an edge end `r` (a position) maps to; -1 where r is no position of the batch (a contract violation)
template <typename Lookup> __device__ __forceinline__ int64_t nsu_end(int64_t r, int64_t n, Lookup lookup) {
    return (uint64_t)r < (uint64_t)n ? (int64_t)lookup(r) : -1;
}

// ---- flat form: the body of a block.  T is the caller's view of a list's part of the workspace: vals, slot, tile_cnt.
// s0, stride: the thread's first slot and the grid's width, taken from blockDim / gridDim in the kernel itself
// (I: the counters' type; chunk_scan.h's tables reach 2^31 slots and count in int64_t)
template <typename K, typename I = uint32_t>
__device__ __forceinline__ void nsu_clear_tile(K *keys, uint32_t *vals, I cap, I s0, I stride) {
    for (I s = s0; s < cap; s += stride) {
        keys[s] = nsu_empty<K>();
        vals[s] = NSU_UNSEEN;
    }
}

// flags the first occurrences of a tile in their slot words and counts them
template <typename T>
__device__ __forceinline__ void nsu_flag_tile(const T &t, int64_t n, int64_t tile0, uint32_t *s_wave) {
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = p0 + k;
        if (p < n) {
            const uint32_t s = t.slot[p];
            if (t.vals[s] == (uint32_t)p) {
                t.slot[p] = s | NSU_FLAG;
                ++cnt;
            }
        }
    }
    uint32_t total;
    nsu_scan(cnt, s_wave, &total);
    if (threadIdx.x == 0) t.tile_cnt[blockIdx.x] = total;
}

// names the first occurrences of a tile: local id = first occurrences in the tiles before it (base) + the scan inside it.
// The thread owns positions [p0, p0 + NSU_PER), p0 = tile0 + threadIdx.x * NSU_PER: bit k of `first` says p0 + k is a first
// occurrence, rank0 is the local id of the thread's first one, base + total = the first occurrences up to the end of the
// tile.  store(rank, p): what else a first occurrence writes (nodes[rank] = samples[p] is written here).  The caller
// writes its counts and marks from what comes back.
struct NsuRanks {
    uint32_t base, total, rank0, first;
};
template <typename T, typename Store>
__device__ __forceinline__ NsuRanks nsu_apply_tile(const T &t, int64_t n, int64_t tile0, const int64_t *samples,
                                                   int64_t *nodes, uint32_t *s_wave, Store store) {
    NsuRanks r;
    uint32_t before = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += NSU_TILE_THREADS) before += t.tile_cnt[i];
    nsu_scan(before, s_wave, &r.base);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    r.first = 0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k)
        if (p0 + k < n && (t.slot[p0 + k] & NSU_FLAG)) r.first |= 1u << k;
    r.rank0 = r.base + nsu_scan((uint32_t)__popc(r.first), s_wave, &r.total);
    uint32_t rank = r.rank0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        if (r.first & (1u << k)) {
            t.vals[t.slot[p0 + k] & ~NSU_FLAG] = rank;
            store(rank, p0 + k);
            nodes[rank++] = samples[p0 + k];
        }
    }
    return r;
}

static inline int64_t nsu_r256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// LDS a workgroup may ask for on the current device (0: no device)
static inline int64_t nsu_device_lds_limit() {
    static std::atomic<int64_t> cached[64]; // zero-initialised; a race only repeats the query
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (dev >= 0 && dev < 64 && cached[dev] > 0) return cached[dev];
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (dev >= 0 && dev < 64) cached[dev] = v;
    return v;
}

// the LDS form's request above the default limit of a launch (the plan keeps it below the device's): raised once per
// device and kernel, whenever a launch asks for more than the last one set.  raised: the kernel instantiation's own 64
// words, a function-local static of its launcher (zero-initialised; a race only sets the attribute twice).
static inline int nsu_raise_lds(const void *kernel, std::atomic<int64_t> *raised, int64_t dyn) {
    if (dyn <= 64 * 1024) return TG_OK;
    int dev = 0;
    TG_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || raised[dev] < dyn) {
        TG_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        if (dev >= 0 && dev < 64) raised[dev] = dyn;
    }
    return TG_OK;
}

// ---- host side: what a shape needs, which form it takes (tg_ns_induced_* sizes its tables by the same plan) -------------
struct NsuPlan {
    int key_bytes;
    int64_t table_cap, lds_bytes;   // of the LDS form
    int lds_ok;                     // the LDS form's words fit their widths (the LDS limit is checked apart)
    int threads;                    // of the LDS form
    int64_t n_node_tiles, vals_off, slot_off, tile_off, batch_bytes; // flat form: a batch's part of the workspace
};

static inline int nsu_plan(int64_t cap_nodes, int64_t id_bound, const char *who, NsuPlan &pl) {
    TG_REQUIRE(cap_nodes >= 0 && cap_nodes <= NSU_MAX_NODES, "%s: cap_nodes = %lld outside [0, 2^30]", who, (long long)cap_nodes);
    TG_REQUIRE(id_bound >= 1, "%s: id_bound = %lld, at least 1 expected", who, (long long)id_bound);
    pl.key_bytes = id_bound <= ((int64_t)1 << 31) ? 4 : 8;
    pl.table_cap = pow2_at_least((4 * cap_nodes + 2) / 3); // > cap_nodes: a probe always meets an empty slot
    pl.lds_bytes = pl.table_cap * (pl.key_bytes + 4) + ((2 * cap_nodes + 15) & ~(int64_t)15) + NSU_STATIC_LDS;
    pl.lds_ok = cap_nodes <= NSU_LDS_MAX_NODES;
    pl.threads = cap_nodes >= NSU_THREADS ? NSU_THREADS : (int)(cap_nodes < 64 ? 64 : (cap_nodes + 63) & ~(int64_t)63);
    pl.n_node_tiles = cap_nodes > 0 ? (cap_nodes + NSU_TILE - 1) / NSU_TILE : 1;
    pl.vals_off = nsu_r256(pl.table_cap * pl.key_bytes);
    pl.slot_off = pl.vals_off + nsu_r256(pl.table_cap * 4);
    pl.tile_off = pl.slot_off + nsu_r256(cap_nodes * 4);
    pl.batch_bytes = pl.tile_off + nsu_r256(pl.n_node_tiles * 4);
    return TG_OK;
}

// the probe's words for a table of table_cap slots (a power of two): slot = hash >> hash_shift for 32-bit keys, hash &
// cap_mask for 64-bit ones, and cap_mask wraps the probe
static inline void nsu_mask_shift(int64_t table_cap, uint32_t &cap_mask, uint32_t &hash_shift) {
    cap_mask = (uint32_t)(table_cap - 1);
    hash_shift = 32u - (uint32_t)__builtin_ctzll((unsigned long long)table_cap);
}

static inline bool nsu_fits(const NsuPlan &pl, int64_t lds_limit) { return pl.lds_ok && pl.lds_bytes <= lds_limit; }

} // namespace tg
