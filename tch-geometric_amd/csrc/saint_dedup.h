// What GraphSAINT's samplers share (saint_rw.hip: tg_saint_rw_nodes; saint_ne.hip: tg_saint_node_nodes,
// tg_saint_edge_nodes): everything behind the step that says which vertex sits at which position.  The LDS form's rank-and-
// store phase, and the flat form's clear | insert | flag | apply over a mini-batch's part of the workspace.  The kernels are
// templates over the caller's argument struct A, which has the fields
//   nodes, counts, pitch, counts_stride, P, cap_mask, hash_shift, ws, batch_bytes, vals_off, slot_off, tile_off, visit_off
// so each file keeps its own launch arguments and the code of a kernel does not depend on who else includes this header.
#pragma once
#include "ns_unique.h"

namespace tg {

constexpr uint32_t SAINT_NONE = 0xFFFFFFFFu; // flat form's visit word of a position nobody visited (ids are < 2^31)
constexpr int32_t SAINT_STATUS_RANGE = 2;    // status bit 1: an id outside its table (as tg_ns_induced_count's)

// ---- LDS form: first occurrences, ranked in position order.  A thread owns a contiguous run of positions; every thread
// calls it, after a barrier behind the last insert.  loc[p]: the slot of position p (a position nobody visited: any slot
// whose value is not p); tid, nt: the thread and the workgroup's size.  Writes nodes[b] and counts[b] of the round.
template <typename A>
__device__ __forceinline__ void saint_lds_rank_store(const A &a, int64_t b, const nsu_k32 *keys, const uint32_t *vals,
                                                     const uint16_t *loc, int n, int tid, int nt, uint32_t *s_wave) {
    const int per = (n + nt - 1) / nt; // <= NSU_MAX_PER_THREAD
    const int p0 = min(n, tid * per), p1 = min(n, p0 + per);
    uint32_t first = 0;
    for (int p = p0; p < p1; ++p)
        if (vals[loc[p]] == (uint32_t)p) first |= 1u << (p - p0);
    uint32_t n_unique;
    uint32_t rank = nsu_scan((uint32_t)__popc(first), s_wave, &n_unique);
    int64_t *nodes = a.nodes + b * a.pitch;
    for (uint32_t f = first; f;) {
        const int p = p0 + __ffs(f) - 1;
        f &= f - 1;
        nodes[rank++] = (int64_t)keys[loc[p]];
    }
    if (tid == 0) a.counts[b * a.counts_stride] = (int64_t)n_unique;
}

// ---- flat form -------------------------------------------------------------------------------------------------------
struct SaintBatch {
    nsu_k32 *keys;
    uint32_t *vals, *slot, *tile_cnt, *visit;
    template <typename A> __device__ __forceinline__ SaintBatch(const A &a, int64_t b) {
        unsigned char *base = a.ws + b * a.batch_bytes;
        keys = reinterpret_cast<nsu_k32 *>(base);
        vals = reinterpret_cast<uint32_t *>(base + a.vals_off);
        slot = reinterpret_cast<uint32_t *>(base + a.slot_off);
        tile_cnt = reinterpret_cast<uint32_t *>(base + a.tile_off);
        visit = reinterpret_cast<uint32_t *>(base + a.visit_off);
    }
};

template <typename A> __global__ void __launch_bounds__(NSU_TILE_THREADS) saint_clear_kernel(const A a) {
    const SaintBatch t(a, blockIdx.y);
    nsu_clear_tile<nsu_k32>(t.keys, t.vals, a.cap_mask + 1, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

template <typename A> __global__ void __launch_bounds__(NSU_TILE_THREADS) saint_insert_kernel(const A a) {
    const int64_t n = a.P;
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    const SaintBatch t(a, blockIdx.y);
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        const int64_t p = tile0 + k * NSU_TILE_THREADS + threadIdx.x;
        if (p < n) {
            const uint32_t v = t.visit[p];
            uint32_t s = 0; // nobody's visit: slot 0's value is not this position
            if (v != SAINT_NONE) {
                s = nsu_insert<nsu_k32>(t.keys, a.cap_mask, a.hash_shift, v);
                atomicMin(&t.vals[s], (uint32_t)p);
            }
            t.slot[p] = s;
        }
    }
}

// flags the first occurrences of a tile in their slot words and counts them
template <typename A> __global__ void __launch_bounds__(NSU_TILE_THREADS) saint_flag_kernel(const A a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t n = a.P;
    const SaintBatch t(a, blockIdx.y);
    const int64_t p0 = (int64_t)blockIdx.x * NSU_TILE + (int64_t)threadIdx.x * NSU_PER;
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

// names the first occurrences of a tile: rank = first occurrences in the tiles before it + the scan inside it
template <typename A> __global__ void __launch_bounds__(NSU_TILE_THREADS) saint_apply_kernel(const A a) {
    __shared__ uint32_t s_wave[NSU_TILE_THREADS / 64];
    const int64_t b = blockIdx.y, n = a.P;
    const int64_t tile0 = (int64_t)blockIdx.x * NSU_TILE;
    const SaintBatch t(a, b);
    uint32_t before = 0, base;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += NSU_TILE_THREADS) before += t.tile_cnt[i];
    nsu_scan(before, s_wave, &base);
    const int64_t p0 = tile0 + (int64_t)threadIdx.x * NSU_PER;
    uint32_t first = 0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k)
        if (p0 + k < n && (t.slot[p0 + k] & NSU_FLAG)) first |= 1u << k;
    uint32_t total;
    uint32_t rank = base + nsu_scan((uint32_t)__popc(first), s_wave, &total);
    int64_t *nodes = a.nodes + b * a.pitch;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k)
        if (first & (1u << k)) nodes[rank++] = (int64_t)t.keys[t.slot[p0 + k] & ~NSU_FLAG];
    if (tile0 + NSU_TILE >= n && threadIdx.x == 0) a.counts[b * a.counts_stride] = (int64_t)(base + total);
}

// ---- host side -------------------------------------------------------------------------------------------------------
struct SaintPlan {
    int64_t P;
    NsuPlan nsu;
    int64_t visit_off, batch_bytes; // flat form: a mini-batch's part of the workspace
};

// P positions of ids below 2^31 (32-bit keys): nsu_plan's tables and, behind them, a u32 visit word per position
static inline int saint_plan(int64_t P, const char *who, SaintPlan &pl) {
    pl.P = P;
    if (const int rc = nsu_plan(P, 1, who, pl.nsu)) return rc;
    pl.visit_off = pl.nsu.batch_bytes;
    pl.batch_bytes = pl.visit_off + nsu_r256(P * 4);
    return TG_OK;
}

// the table's words of the launch arguments
template <typename A> static inline void saint_plan_args(const SaintPlan &pl, void *workspace, A &a) {
    a.P = pl.P;
    nsu_mask_shift(pl.nsu.table_cap, a.cap_mask, a.hash_shift);
    a.ws = static_cast<unsigned char *>(workspace);
    a.batch_bytes = pl.batch_bytes, a.vals_off = pl.nsu.vals_off, a.slot_off = pl.nsu.slot_off;
    a.tile_off = pl.nsu.tile_off, a.visit_off = pl.visit_off;
}

// the LDS form's request above the default limit of a launch (the caller checked that it fits the device's): raised once
// per device and kernel, to the most a request that fits can ask for.  Every thread sets the SAME value, so threads with
// different requests cannot lower each other's limit, and a race only sets it twice.  raised: the kernel's own 64 words.
static inline int saint_raise_lds(const void *kernel, std::atomic<int64_t> *raised, int64_t dyn) {
    if (dyn <= 64 * 1024) return TG_OK;
    int dev = 0;
    TG_HIP(hipGetDevice(&dev));
    const int64_t most = nsu_device_lds_limit() - NSU_STATIC_LDS; // >= dyn: nsu_fits held
    if (dev < 0 || dev >= 64 || raised[dev] != most) {
        TG_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        if (dev >= 0 && dev < 64) raised[dev] = most;
    }
    return TG_OK;
}

// insert | flag | apply over the visit lists of a round (the caller cleared the tables and wrote the lists)
template <typename A> static inline int saint_launch_dedup(const A &a, const SaintPlan &pl, hipStream_t stream) {
    const dim3 grid((unsigned)pl.nsu.n_node_tiles, (unsigned)a.n_batches), block(NSU_TILE_THREADS);
    hipLaunchKernelGGL(saint_insert_kernel<A>, grid, block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(saint_flag_kernel<A>, grid, block, 0, stream, a);
    TG_LAUNCH_CHECK();
    hipLaunchKernelGGL(saint_apply_kernel<A>, grid, block, 0, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

template <typename A> static inline int saint_launch_clear(const A &a, const SaintPlan &pl, hipStream_t stream) {
    const int64_t clear_blocks = (pl.nsu.table_cap + NSU_TILE_THREADS - 1) / NSU_TILE_THREADS;
    hipLaunchKernelGGL(saint_clear_kernel<A>, dim3((unsigned)(clear_blocks < 1024 ? clear_blocks : 1024), (unsigned)a.n_batches),
                       dim3(NSU_TILE_THREADS), 0, stream, a);
    TG_LAUNCH_CHECK();
    return TG_OK;
}

} // namespace tg
