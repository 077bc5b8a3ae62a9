// What the node2vec walk kernels share (random_walk.hip: tg_random_walk / tg_random_walk_es; rw_skipgram.hip:
// tg_rw_skipgram): the CSR view, has_edge (binary search or edge-set probe) and ONE step of one walker.
#pragma once
#include "tg_device.h"
#include "tg_host.h"

namespace tg {

// CSR accessors: the optional u32 shadows (tg_graph.ptrs32 / indices32) hold the same values in half the bytes --
// twice the entries per gathered line, and the whole offset table of RMAT-24 (67 MB) stays in the Infinity Cache
struct CsrView {
    const int64_t *ptrs, *indices;
    const uint32_t *ptrs32, *indices32;
    const uint64_t *edge_set; // optional hash set of the edges (tg_edge_set_build) and its slot mask
    uint64_t edge_mask;
    __device__ __forceinline__ int64_t ptr(int64_t i) const { return ptrs32 ? (int64_t)ptrs32[i] : ptrs[i]; }
    __device__ __forceinline__ int64_t idx(int64_t e) const { return indices32 ? (int64_t)indices32[e] : indices[e]; }
};

// ---- the edge set: has_edge as a hash probe --------------------------------------------------------------------------
// graph.rs:80-83 answers has_edge(x, y) by a binary search of row x: log2(deg) DEPENDENT random line requests, ~13 on
// RMAT-24, and node2vec with p != q asks once per proposal -- the walk then sits on the chip's random-request ceiling.
// The set holds every edge once as the key x << 32 | y in an open-addressing table (linear probing, load <= 1/2, 8-byte
// slots: a probe sequence usually stays inside one 128-byte line), so the same question is ONE line request, with the
// same answer (a multi-edge is one key; ids must be < 2^32 - 1).
constexpr uint64_t EDGE_SET_EMPTY = ~0ull;
__device__ __forceinline__ uint64_t edge_key_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 29;
    return k;
}
__device__ __forceinline__ bool edge_set_has(const uint64_t *__restrict__ slots, uint64_t mask, int64_t x, int64_t y) {
    const uint64_t key = ((uint64_t)x << 32) | (uint64_t)y;
    for (uint64_t s = edge_key_hash(key) & mask;; s = (s + 1) & mask) {
        const uint64_t v = slots[s];
        if (v == key) return true;
        if (v == EDGE_SET_EMPTY) return false;
    }
}

__device__ __forceinline__ bool has_edge(const CsrView &g, int64_t x, int64_t y) { // graph.rs:80-83
    if (g.edge_set) return edge_set_has(g.edge_set, g.edge_mask, x, y);
    int64_t lo = g.ptr(x), hi = g.ptr(x + 1);
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t v = g.idx(mid);
        if (v == y) return true;
        if (v < y)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

// the three acceptance probabilities of random_walk.rs:29-36 (computed on the host, all in f32)
struct WalkProbs {
    float prob0, prob1, prob2;
    __host__ __device__ bool always_accept() const { return prob0 >= 1.0f && prob1 >= 1.0f && prob2 >= 1.0f; } // r < 1 always holds
};

// Step l of walker `id` standing at `cur` (the vertex before it: `prev`, -1 at the start): random_walk.rs:45-66.
// The proposal of attempt a is the draw (ck, id, l, a): its low 64 bits pick the neighbour, word 2 is the acceptance
// test's uniform.  false: `cur` has no out-edge (the walk is over); true: prev / cur moved on.
__device__ __forceinline__ bool walk_step(const CsrView &g, CallKey ck, uint64_t id, uint32_t l, const WalkProbs &pr,
                                          bool always_accept, int64_t &prev, int64_t &cur) {
    const int64_t b = g.ptr(cur), e = g.ptr(cur + 1);
    if (e <= b) return false; // random_walk.rs:45-47
    const uint64_t deg = (uint64_t)(e - b);
    int64_t next;
    for (uint32_t attempt = 0;; ++attempt) { // :52-66
        const Draw d = draw(ck, id, l, attempt);
        next = g.idx(b + (int64_t)bounded64(d.a(), deg));
        if (always_accept) break;
        const float r = u32_to_f32_01(d.w[2]);
        if (next == prev) {
            if (r < pr.prob0) break;
        } else if (prev >= 0 && has_edge(g, next, prev)) {
            if (r < pr.prob1) break;
        } else if (r < pr.prob2) {
            break;
        }
    }
    prev = cur;
    cur = next;
    return true;
}

} // namespace tg

// ---- host side ---------------------------------------------------------------------------------------------------------
static inline int64_t edge_set_slots(int64_t n_edges) {
    int64_t cap = 64;
    while (cap < 2 * n_edges) cap <<= 1;
    return cap;
}
static inline tg::WalkProbs walk_probs(float p, float q) { // random_walk.rs:29-36, all in f32
    const float inv_p = 1.0f / p, inv_q = 1.0f / q;
    float max_prob = inv_p;
    if (1.0f >= max_prob) max_prob = 1.0f;
    if (inv_q >= max_prob) max_prob = inv_q;
    return tg::WalkProbs{1.0f / p / max_prob, 1.0f / max_prob, 1.0f / q / max_prob};
}
