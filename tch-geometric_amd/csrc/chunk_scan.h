// What the two-pass "count, then emit" operators over a CSC graph cut into chunks share (ns_induced.hip: the plain and the
// grouped induced pair; cluster.hip: tg_cluster_count / _emit; ns_full.hip: tg_ns_full_count / _emit): the sizes, the
// column-offset read, the table probe, the clear, the prefix over tiles of chunks, the pieces of the scan's unit walk, and
// on the host the graph checks with the chunk bound, the workspace refusals, the workspace_bytes answer and the round loop.
//
// The scheme.  Pass 1 counts per chunk (cpref[c]) and adds a unit's counts to its tile's sum (ctile) with one atomicAdd;
// the chunk apply kernel turns cpref into the exclusive prefix in place (the tiles before + the scan inside the tile) and
// its last tile has the batch's total.  Pass 2 scans again and writes a chunk's items at its prefix, ranked in lane order
// by ballot + popcount, so no mask is kept between the passes.  The scan kernels run a fixed grid (cs_scan_grid) and
// stride over the chunk count in the batch's header; a wave takes a UNIT of up to CS_UNIT consecutive chunks, lanes
// 0 .. unit-1 each look one chunk up at once (cs_last_le over a chunk prefix: the dependent reads are paid once per unit
// instead of once per chunk), then the wave walks the chunks, 64 entries a step.
//
// Why CS_CHUNK = 512 (the filtered hop's group size): a chunk costs one search in a chunk prefix, one word of workspace and
// one prefix element, so it should be long enough that those vanish beside the scan (8 wave steps of 64 entries, each with
// a dependent random probe); and it should be short enough that a hub spreads: a 10^5-entry column is 196 chunks = 13 wave
// units.  2 048 (the edge-set segment) would quarter the per-chunk array (5.6 MB per loader-shaped batch on RMAT-24 at 512,
// beside the 1.4 MB node prefix and the 2 MB table) but leaves a 10^5 hub to 4 wave units.
//
// As in ns_unique.h, the __global__ shells, their argument structs and workspace views stay in the .hip files, so the code
// of a kernel does not depend on who else includes this header; and what a body needs of blockDim / gridDim it takes as
// an argument from the kernel (cs_clear's s0 and stride, the unit rules' grid_blocks): read inside a device function they
// compile to another, longer look-up than in the kernel.  The unit walk itself (the loop over units, the look-up lanes,
// the loop over a unit's chunks, pass 1's stores) is NOT here.  It was written once, as a __forceinline__ template over
// the look-up and the chunk's body as callables, and measured (tools/kernel_diff.py, tools/ab_chunk_pairs.py; the figures
// are of an earlier run than the two of this tree, kept in profiles/refactor_chunk_pairs.json beside them):
// cl_scan_kernel's emit instances went from 73 to 74 VGPRs; nsi_scan_kernel and nsf_scan_kernel kept their registers and
// LDS, but count + emit of the plain induced pair at 16 batches of 16 seeds took 1.4 % longer than the parent's (0.2548
// against 0.2514 ms, every round) and of the full-neighbour pair at its loader shape 0.6 % (0.1604 against 0.1594 ms),
// past the bar of twice the gap between two runs of the parent.  So the three kernels keep their loops as written, the
// halving of the unit included, and share the pieces around them (cs_short_quarter / cs_short_fill, cs_last_le, cs_find,
// cs_unit_counted): their instruction streams are the parent's but for the operand order of cs_last_le's midpoint.
#pragma once
#include <algorithm>

#include "ns_unique.h"

namespace tg {

constexpr int CS_CHUNK = 512;                        // CSC offsets of a chunk
constexpr int CS_UNIT = 16;                          // chunks a wave takes at once (a power of two; fewer where chunks are few)
constexpr int CS_THREADS = NSU_TILE_THREADS;         // 256
constexpr int CS_TILE = NSU_TILE;                    // positions / chunks of a prefix tile: a thread owns NSU_PER consecutive ones
constexpr int CS_HEADER = 256;                       // bytes at the head of a batch's workspace: word 0 = its chunks (0: none, refused)
constexpr int64_t CS_MAX_CHUNKS = (int64_t)1 << 31;  // of the bound
constexpr int64_t CS_ROUND_MAX = NSU_ROUND_MAX;      // batches per launch (grid.y)
constexpr int CS_SCAN_BLOCKS = 2048;                 // of the fixed grid: 256 CUs x 4 SIMDs x 8 waves in 4-wave workgroups
static_assert(CS_TILE % CS_UNIT == 0, "a unit's chunks share a tile");

__device__ __forceinline__ int64_t csc_ptr(const int64_t *ptrs, const uint32_t *ptrs32, int64_t v) {
    return ptrs32 ? (int64_t)ptrs32[v] : ptrs[v];
}

// looks `key` up, at most one pass over the table.  VALUE: returns the slot's value (the first position), else the slot;
// NSU_UNSEEN where the key has none.  MASKED: nsu_insert<K, true>'s hash, for a table that may have one slot
template <bool VALUE, bool MASKED, typename K>
__device__ __forceinline__ uint32_t cs_find(const K *keys, const uint32_t *vals, uint32_t mask, uint32_t shift, K key) {
    uint32_t s = MASKED ? nsu_hash(key, mask, shift & 31u) & mask : nsu_hash(key, mask, shift);
    for (uint32_t i = 0; i <= mask; ++i) {
        const K k = keys[s];
        if (k == key) return VALUE ? vals[s] : s;
        if (k == nsu_empty<K>()) break;
        s = (s + 1) & mask;
    }
    return NSU_UNSEEN;
}

// pass 1's first kernel: the table, the tile sums and the first HDR_WORDS header words of a batch.  s0, stride: the
// thread's first index and the grid's width, taken from blockDim / gridDim in the kernel itself (as nsu_clear_tile's)
template <int HDR_WORDS, typename K, typename W>
__device__ __forceinline__ void cs_clear(K *keys, uint32_t *vals, int64_t table_cap, W *ctile, int64_t chunk_tiles,
                                         unsigned long long *hdr, int64_t s0, int64_t stride) {
    nsu_clear_tile<K, int64_t>(keys, vals, table_cap, s0, stride);
    for (int64_t s = s0; s < chunk_tiles; s += stride) ctile[s] = 0;
    if (s0 == 0) {
#pragma unroll
        for (int w = 0; w < HDR_WORDS; ++w) hdr[w] = 0;
    }
}

__device__ __forceinline__ uint32_t cs_scan(uint32_t v, uint32_t *s_wave, uint32_t *total) { return nsu_scan(v, s_wave, total); }
__device__ __forceinline__ unsigned long long cs_scan(unsigned long long v, unsigned long long *s_wave, unsigned long long *total) {
    return nsu_scan64(v, s_wave, total);
}

// the sum of the tiles before this block's: tile[0] .. tile[blockIdx.x - 1].  Every thread calls it
template <typename W> __device__ __forceinline__ W cs_tiles_before(const W *tile, W *s_wave) {
    W before = 0, base;
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += CS_THREADS) before += tile[i];
    cs_scan(before, s_wave, &base);
    return base;
}

// a block of the chunk apply kernel: the exclusive prefix over its tile of chunks, in place.  The thread owns chunks
// [c0, c0 + NSU_PER) and pre[k] (where the caller passes its array: one inside the result would leave the registers once
// it is indexed by a variable) is the prefix of chunk c0 + k; base = the tiles before, base + total = up to the tile's end.
// last: this is the batch's last tile (tile 0 of a batch without chunks); its thread 0 closes the prefix in the caller,
// cpref[n_chunks] = base + total, in one branch with what else the total is (n_edges, n_nodes, edge_marks).
// The caller leaves first where cs_tile_idle says so.
template <typename W> struct CsTile {
    W base, total;
    unsigned long long c0;
    bool last;
};
__device__ __forceinline__ bool cs_tile_idle(unsigned long long n) { // uniform
    return (unsigned long long)blockIdx.x * CS_TILE >= n && blockIdx.x != 0;
}
template <typename W>
__device__ __forceinline__ CsTile<W> cs_chunk_apply_tile(W *cpref, const W *ctile, unsigned long long n_chunks, W *s_wave,
                                                         W *pre = nullptr) {
    CsTile<W> r;
    const unsigned long long tile0 = (unsigned long long)blockIdx.x * CS_TILE;
    r.base = cs_tiles_before(ctile, s_wave);
    r.c0 = tile0 + (unsigned long long)threadIdx.x * NSU_PER;
    W h[NSU_PER], mine = 0;
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        h[k] = r.c0 + k < n_chunks ? cpref[r.c0 + k] : 0;
        mine += h[k];
    }
    W run = r.base + cs_scan(mine, s_wave, &r.total);
#pragma unroll
    for (int k = 0; k < NSU_PER; ++k) {
        if (pre) pre[k] = run;
        if (r.c0 + k < n_chunks) cpref[r.c0 + k] = run;
        run += h[k];
    }
    r.last = tile0 + CS_TILE >= n_chunks;
    return r;
}

// the last entry of pref[0 .. n) whose prefix is <= c, where pref[0] = 0 <= c < pref[n]: the entry that owns chunk c
template <typename I, typename W> __device__ __forceinline__ I cs_last_le(const W *pref, I n, unsigned long long c) {
    I lo = 0, hi = n;
    while (hi - lo > 1) {
        const I mid = (lo + hi) >> 1;
        if (pref[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// The unit of a batch with few chunks: a scan kernel starts at CS_UNIT and halves the unit while its rule says the batch is
// short of chunks for it, `int unit = CS_UNIT; while (unit > 1 && cs_short_...(n_chunks, unit, gridDim.x, waves)) unit >>= 1;`
// (the loop stays in the kernel: behind a function the compiler no longer sees that unit is a power of two, and the
// division by it becomes a real one).  Two rules; grid_blocks * waves = the wavefronts of the batch's grid.  They were
// measured apart and differ on purpose: do not unify them.
// The induced pairs: a batch with fewer units than a quarter of the grid's waves takes shorter units, so that a lone hub
// still spreads
__device__ __forceinline__ bool cs_short_quarter(unsigned long long n_chunks, int unit, unsigned grid_blocks, int waves) {
    return 4 * n_chunks < (unsigned long long)unit * grid_blocks * waves;
}
// The cluster and the full-neighbour pair: shorter units while the batch's wavefronts would not all get one.  A small
// batch (a thousand short columns, a chunk each) is latency, not work, and a chunk is a chain of dependent accesses
__device__ __forceinline__ bool cs_short_fill(unsigned long long n_chunks, int unit, unsigned grid_blocks, int waves) {
    return (n_chunks + unit - 1) / unit < (unsigned long long)grid_blocks * waves;
}

// pass 1, after a unit's chunks have each stored their count in cpref: the unit's sum goes to its tile (a unit's chunks
// share a tile)
template <typename W> __device__ __forceinline__ void cs_unit_counted(W *ctile, unsigned long long u, int unit, W sum, int lane) {
    if (lane == 0 && sum) atomicAdd(&ctile[u * unit / CS_TILE], sum);
}

static inline unsigned cs_scan_grid(int64_t nb) { return (unsigned)std::max<int64_t>(1, CS_SCAN_BLOCKS / nb); }

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the graph's sizes and the chunks a batch may have: chunk_cap > 0 is the caller's capacity, else lists of `pitch`
// entries with disjoint columns (distinct nodes, distinct clusters) end in at most one ragged chunk each.  pitch is the
// caller's, already held to its range
static int cs_plan_chunks(const tg_graph *csc, int64_t pitch, int64_t chunk_cap, const char *who, int64_t &chunk_bound,
                          int64_t &chunk_tiles) {
    TG_REQUIRE(csc, "%s: null graph", who);
    TG_REQUIRE(csc->n_major >= 0 && csc->n_edges >= 0, "%s: negative graph size (n_major = %lld, n_edges = %lld)", who,
               (long long)csc->n_major, (long long)csc->n_edges);
    TG_REQUIRE(chunk_cap <= CS_MAX_CHUNKS, "%s: chunk_cap = %lld, at most 2^31 expected", who, (long long)chunk_cap);
    chunk_bound = chunk_cap > 0 ? chunk_cap : pitch + (csc->n_edges + CS_CHUNK - 1) / CS_CHUNK;
    TG_REQUIRE(chunk_bound <= CS_MAX_CHUNKS, "%s: %lld chunks per batch, at most 2^31 expected", who, (long long)chunk_bound);
    chunk_tiles = chunk_bound / CS_TILE + 1;
    return TG_OK;
}

// what count and emit refuse alike once the plan has batch_bytes (the division cannot overflow)
static int cs_check_launch(const tg_graph *csc, int64_t n_batches, int64_t batch_bytes, const void *workspace,
                           int64_t workspace_bytes, const char *who) {
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    TG_REQUIRE(workspace_bytes >= 0, "%s: workspace_bytes = %lld is negative", who, (long long)workspace_bytes);
    TG_REQUIRE(workspace && workspace_bytes / batch_bytes >= n_batches,
               "%s: workspace too small (%lld bytes, %lld batches of %lld expected)", who,
               (long long)(workspace ? workspace_bytes : 0), (long long)n_batches, (long long)batch_bytes);
    TG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    TG_REQUIRE(csc->ptrs && csc->indices, "%s: null ptrs / indices", who);
    return TG_OK;
}

// n_batches workspaces of batch_bytes have a size in int64 (n_batches >= 0)
static int cs_bytes_fit(int64_t batch_bytes, int64_t n_batches, const char *who) {
    TG_REQUIRE(batch_bytes <= INT64_MAX / std::max<int64_t>(1, n_batches), "%s: %lld batches of %lld bytes overflow int64", who,
               (long long)n_batches, (long long)batch_bytes);
    return TG_OK;
}

// the answer of a *_workspace_bytes query once the plan has batch_bytes
static int cs_answer_bytes(int64_t batch_bytes, int64_t n_batches, const char *who, int64_t *bytes, int64_t *bytes_min) {
    TG_REQUIRE(bytes && bytes_min, "%s: null output", who);
    TG_REQUIRE(n_batches >= 0 && n_batches <= 0x7fffffff, "%s: n_batches = %lld outside [0, 2^31)", who, (long long)n_batches);
    if (const int rc = cs_bytes_fit(batch_bytes, n_batches, who)) return rc;
    *bytes_min = batch_bytes;
    *bytes = batch_bytes * n_batches;
    return TG_OK;
}

// round(b0, nb) launches batches [b0, b0 + nb), nb <= CS_ROUND_MAX, until n_batches are done or one fails
template <typename Round> static int cs_rounds(int64_t n_batches, Round round) {
    for (int64_t b0 = 0; b0 < n_batches; b0 += CS_ROUND_MAX)
        if (const int rc = round(b0, std::min(CS_ROUND_MAX, n_batches - b0))) return rc;
    return TG_OK;
}

} // namespace tg
