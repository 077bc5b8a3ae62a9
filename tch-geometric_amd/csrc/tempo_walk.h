// One step of the temporal walk (random_walk.rs:117-153), by one WAVEFRONT, shared by rw_tempo_kernel (random_walk.hip)
// and the skip-gram batch kernel (tempo_skipgram.hip): the wave streams the row's timestamps coalesced, ranks the
// admissible neighbours with ballot + popcount, resolves the one-slot reservoir from one addressed draw per chunk of 64 row
// positions, restarts from an earlier position of the walk when nothing is admissible, and fetches the one neighbour id
// the step needs.  Both callers draw the same blocks, so their walks agree value for value.
#pragma once
#include "row_stream.h"
#include "tg_device.h"

namespace tg {

struct TempoStep {
    int64_t node, ts;
};

// cur: where the walker stands; l: the step (it fills column l + 1); it: the walker's start time, [wlo, whi) = it + window;
// hist: the walk so far in LDS, nodes at hist[0 .. l], their timestamps at hist[L .. L + l] (read for a restart only).
// Every lane returns the same (node, ts).
__device__ __forceinline__ TempoStep tempo_walk_step(const int64_t *__restrict__ ptrs, const int64_t *__restrict__ indices,
                                                     const int64_t *__restrict__ node_ts, const int64_t *__restrict__ edge_ts,
                                                     const CallKey ck, uint64_t step_id, int64_t cur, int64_t l, int64_t it,
                                                     int64_t wlo, int64_t whi, const int64_t *hist, int64_t L, int lane,
                                                     uint64_t lt_mask) {
    const int64_t b = ptrs[cur], e = ptrs[cur + 1];
    // one-slot reservoir over the candidates in row order (sampling.rs:12-24 with k = 1), philox-mode: ONE draw per chunk
    // of 64 raw row positions (the CPU checker's orc_reservoir_one_chunked states the law).  Candidates of rank >= 1 are
    // eligible; a chunk with m of them, after `seen` earlier ones, takes the slot with probability m / (seen + m) and
    // gives it to one of its m.  The draws of 64 consecutive chunks are computed TOGETHER, lane l the block of chunk
    // 64 g + l, when the row first needs one of group g: a Philox block per 4 096 row positions and wavefront instead
    // of one per 64 (a block per chunk on the scalar unit costs what the per-candidate blocks cost on the vector unit:
    // both issue once per chunk -- measured 101 ms against 75).
    uint32_t n_pass = 0, seen = 0;
    int64_t best_v = -1, best_t = -1; // the slot's candidate (edge position, time), held by one lane
    bool have_best = false;
    int64_t first_v = -1, first_t = -1; // candidate of rank 0 (held by one lane)
    bool has_first = false;
    uint32_t group = 0xffffffffu; // the group of 64 chunks whose draws the lanes hold
    Draw gd;
    gd.w[0] = gd.w[1] = gd.w[2] = gd.w[3] = 0u;
    auto visit = [&](int64_t v, bool valid, int64_t ts) { // v: edge position
        const bool ok = valid && ((ts == -1 || it == -1) || (wlo <= ts && ts < whi)); // :129-138
        const uint64_t mask = __ballot(ok);
        const uint32_t rank = n_pass + (uint32_t)__popcll(mask & lt_mask);
        if (ok && rank == 0) {
            first_v = v;
            first_t = ts;
            has_first = true;
        }
        const bool eligible = ok && rank >= 1;
        const uint64_t emask = __ballot(eligible);
        const uint32_t m = (uint32_t)__popcll(emask);
        if (m > 0) { // uniform
            const uint32_t chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((v - b) >> 6));
            if ((chunk >> 6) != group) { // uniform
                group = chunk >> 6;
                gd = draw(ck, step_id, (group << 6) + (uint32_t)lane, D1_CHUNK);
            }
            const int from = (int)(chunk & 63u);
            const uint64_t da = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)gd.w[0], from) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)gd.w[1], from) << 32);
            const uint64_t db = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)gd.w[2], from) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)gd.w[3], from) << 32);
            if (seen == 0 || bounded64(da, (uint64_t)(seen + m)) < (uint64_t)m) {
                const uint32_t r = (uint32_t)bounded64(db, (uint64_t)m);
                have_best = eligible && (uint32_t)__popcll(emask & lt_mask) == r;
                if (have_best) {
                    best_v = v;
                    best_t = ts;
                }
            }
            seen += m;
        }
        n_pass += (uint32_t)__popcll(mask);
    };
    // loads in flight per lane: few -- most rows are short and every load of a round is issued whether the row reaches
    // it or not (RMAT-24, 1 M walkers x 20 steps: 97.6 / 85.1 / 74.5 / 73.8 ms with 8 / 4 / 2 / 1 chunks per round)
    if (e - b <= 128)
        stream_row_ts<1>(indices, edge_ts, node_ts, b, e, lane, visit);
    else
        stream_row_ts<2>(indices, edge_ts, node_ts, b, e, lane, visit);
    TempoStep next;
    if (n_pass == 0) { // :144-148 restart from an earlier position of this walk
        const Draw d = draw(ck, step_id, 0u, D1_RESTART);
        const int64_t rr = (int64_t)bounded64(d.a(), (uint64_t)(l + 1));
        wave_lds_handoff();
        next.node = hist[rr];
        next.ts = hist[L + rr];
    } else {
        const uint64_t owner = (seen > 0) ? __ballot(have_best) : __ballot(has_first);
        const int src = __ffsll((long long)owner) - 1;
        next.node = indices[__shfl((seen > 0) ? best_v : first_v, src, 64)]; // the one neighbour id the step needs
        next.ts = __shfl((seen > 0) ? best_t : first_t, src, 64);
    }
    return next;
}

} // namespace tg
