// SEAL enclosing subgraphs with double-radius node labels (tg_seal_nodes; the rule in include/tchgeo_seal.h).
// The device code described here lives in seal.h, which seal_capped.hip shares; this file holds the kernel and the entry points.
//   One workgroup of 256 threads owns one slot -- a link (u, v) -- from its first hop to its output rows; a persistent grid
//   walks slots i, i + grid, ...; the rounds are workgroup barriers.
//   table    open addressing over T places (a power of two >= max(1024, 2 * node_cap)): key / du / dv as three u32 arrays,
//            the LIST of claimed places in claim order (node_cap words; u first, v second), a QUEUE of T words and two MARK
//            bits per place (T / 16 words).  One kernel template over where the table lives: LDS (ds atomics; T = 1024 or
//            4096) or the caller's workspace (global atomics; words they write are read at agent scope, past the CU's L1).
//   deal     a frontier is walked 256 vertices at a time: every thread fetches its vertex's row, a ballot compacts the
//            rows that have entries into an LDS queue of {row begin, exclusive prefix of the degrees, two bits}, and the
//            tile's entries are dealt out FLAT: thread t takes entries t, t + 256, ... of the concatenated rows and finds
//            its row by a search of the prefix, the row of its entry before tried first.  Consecutive lanes read consecutive
//            `indices` words and a hub row costs d / 256 per thread.  The rows of a frontier are distinct vertices, but a
//            graph may hold more than 2^32 entries: the prefix is 64 bits wide.
//   hops     h claiming hops from {u, v}: a vertex met for the first time claims a place by compare-and-swap and takes the
//            next list position from a counter; hop t's frontier is the list range that hop t - 1 appended.  The counter
//            passing node_cap is the overflow: claims stop at once, so a probe always ends.
//   rounds   both restricted searches as ONE synchronous pass that only looks up: a queue entry is a place with two bits
//            (wave of u, wave of v).  A round deals the entries queued by the round before; a target inside N whose distance
//            for a wave is still unset gets that wave's mark bit (never v for u's wave, never u for v's), and whoever sets a
//            place's first mark of the round appends it to the queue.  Behind the round's last tile the marks become the
//            distances and the queue entries' bits; no distance is written while a round reads them.  A place is queued
//            at most twice (once per wave), so 2 * node_cap <= T words hold every round.
//   output   the others' (id << 32 | place) words are sorted by a bitonic network over the dead queue, then u, v and the
//            sorted places write nodes / z / du / dv.
//   cleanup  only the listed places are reset (every mark is cleared by the round that set it); a refused slot, whose claims
//            may have passed the list, clears its whole table.
// LDS: 18.25 T bytes of table, list, queue and marks + 5 184 B of deal queue and counters: 23.3 KiB at T = 1024 -- six
// workgroups fit a CU's 160 KiB -- and 78.1 KiB at T = 4096 -- two fit.  The workspace form keeps only the 5 184 B.
#include "seal.h"

namespace tg {

template <bool LDS> __global__ void __launch_bounds__(SEAL_THREADS) seal_nodes_kernel(const SealParams P) {
    extern __shared__ __align__(16) unsigned char seal_lds[];
    __shared__ SealShared s;
    SealEveryHop hops;
    seal_slots<LDS>(P, s, seal_lds, hops);
}

} // namespace tg

extern "C" int tg_seal_workspace_bytes(int64_t m, int32_t node_cap, int32_t form, int64_t *bytes, int32_t *form_taken) {
    TG_REQUIRE(bytes, "tg_seal_workspace_bytes: null bytes");
    tg::SealPlan pl;
    const int rc = tg::seal_plan(m, node_cap, form, &pl, "tg_seal_workspace_bytes");
    if (rc != TG_OK) return rc;
    *bytes = pl.groups * pl.group_bytes;
    if (form_taken) *form_taken = pl.form;
    return TG_OK;
}

extern "C" int tg_seal_nodes(const tg_graph *g, const tg_seal_in *in, const tg_seal_out *out, int64_t m, int32_t form,
                             int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_) {
    using namespace tg;
    const char *who = "tg_seal_nodes";
    TG_REQUIRE(g && in && out, "%s: null graph / in / out", who);
    SealPlan pl;
    int rc = seal_plan(m, in->node_cap, form, &pl, who);
    if (rc != TG_OK) return rc;
    SealParams p;
    bool launch;
    rc = seal_params(g, in, out, m, pl, status, workspace, workspace_bytes, &p, &launch, who);
    if (rc != TG_OK || !launch) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (pl.form == TG_SEAL_FORM_LDS) {
        // as many workgroups as stay resident on 256 CUs walk the slots: six per CU with the small table, two with the large
        const int64_t grid = std::min<int64_t>(m, pl.log_t == SEAL_LOG_T_SMALL ? 256 * 6 : 256 * 2);
        if (pl.lds_bytes > 64 * 1024)
            TG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&seal_nodes_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
        hipLaunchKernelGGL(seal_nodes_kernel<true>, dim3((unsigned)grid), dim3(SEAL_THREADS), (size_t)pl.lds_bytes, stream, p);
    } else {
        hipLaunchKernelGGL(seal_nodes_kernel<false>, dim3((unsigned)pl.groups), dim3(SEAL_THREADS), 0, stream, p);
    }
    TG_LAUNCH_CHECK();
    return TG_OK;
}
