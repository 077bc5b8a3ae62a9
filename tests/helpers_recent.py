"""NumPy restatement of TG_SAMPLER_RECENT (include/tchgeo.h at the define): the k most recent admitted edges of every
frontier vertex, and the reference's loop over hops (neighbor_sampling.rs:188-223) around it.  Deliberately plain: one
Python loop per vertex, a stable sort per column."""
import numpy as np

FILTER_NONE, FILTER_STATIC, FILTER_RELATIVE, FILTER_DYNAMIC = -1, 0, 1, 2


def admitted(ts, state, filter_mode, forward, window):
    """neighbor_sampling.rs:55-67 over an int64 array, in wrapping arithmetic."""
    ts = np.asarray(ts, dtype=np.int64)
    if filter_mode == FILTER_NONE:
        return np.ones(ts.shape, dtype=bool)
    with np.errstate(over="ignore"):
        if filter_mode == FILTER_STATIC:
            x = ts
        else:
            d = ts - np.int64(state)
            x = d if forward else -d
    return (np.int64(window[0]) <= x) & (x <= np.int64(window[1]))


def recent_hop(ptrs, idx, ts, vertices, states, k, filter_mode=FILTER_NONE, forward=False, window=(0, 0)):
    """-> (cnt[m], offsets[m + 1], neighbors, edge_ptrs, parents, states_out), grouped by frontier vertex in rank order.
    vertices < 0 are empty slots; states may be None without a filter (states_out is then all 0)."""
    ptrs, idx, ts = (np.asarray(a, dtype=np.int64) for a in (ptrs, idx, ts))
    cnt, nbr, eps, par, sto = [], [], [], [], []
    for i, w in enumerate(np.asarray(vertices, dtype=np.int64)):
        if w < 0:
            cnt.append(0)
            continue
        s = 0 if states is None else int(states[i])
        e = np.arange(ptrs[w], ptrs[w + 1], dtype=np.int64)
        e = e[admitted(ts[e], s, filter_mode, forward, window)]
        # rank: forward the smaller timestamp first, else the larger; ties the smaller edge pointer (e ascends: stable)
        order = np.lexsort((e, ts[e] if forward else ~ts[e]))
        e = e[order][:k]
        cnt.append(len(e))
        nbr.append(idx[e])
        eps.append(e)
        par.append(np.full(len(e), i, dtype=np.int64))
        sto.append(ts[e] if filter_mode == FILTER_DYNAMIC else np.full(len(e), s, dtype=np.int64))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.empty(0, dtype=np.int64)
    cnt = np.asarray(cnt, dtype=np.int64).reshape(-1)
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return cnt, offsets, cat(nbr), cat(eps), cat(par), cat(sto)


def recent_ns_homo(ptrs, idx, ts, seeds, fanout, seeds_state=None, filter_mode=FILTER_NONE, forward=False, window=(0, 0)):
    """The reference's loop over hops with recent_hop as the sampler ->
    (samples, rows, cols, edge_index, layer_offsets, counts, states)."""
    seeds = np.asarray(seeds, dtype=np.int64)
    n_seeds = len(seeds)
    samples = [seeds]
    states = [np.zeros(n_seeds, dtype=np.int64) if seeds_state is None else np.asarray(seeds_state, dtype=np.int64)]
    rows, cols, eidx, layer_offsets = [], [], [], []
    begin, ne = 0, 0
    frontier, fstate = samples[0], states[0]
    for k in fanout:
        layer_offsets.append((n_seeds + ne, ne, n_seeds + ne))                     # :193
        cnt, off, nbr, ep, par, sto = recent_hop(ptrs, idx, ts, frontier, fstate, int(k), filter_mode, forward, window)
        tot = int(off[-1])
        rows.append(np.arange(n_seeds + ne, n_seeds + ne + tot, dtype=np.int64))    # :217 j
        cols.append(begin + par)                                                   # :217 i
        eidx.append(ep)
        samples.append(nbr)
        states.append(sto)
        begin += len(frontier)                                                     # :221: the next frontier starts here
        ne += tot
        frontier, fstate = nbr, sto
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.empty(0, dtype=np.int64)
    return (cat(samples), cat(rows), cat(cols), cat(eidx), layer_offsets, (n_seeds + ne, ne), cat(states))


# ---- the graph and timestamp sets of the device tests
CRAFTED_DEGREES = (0, 1, 6, 7, 8, 32, 33, 34, 63, 64, 65, 128, 129)   # 0, 1, k - 1, k, k + 1 for k in 7, 33, 64; 128, 129
HUB_DEGREE = 5000


def recent_test_graph(scale=10, seed=0x7E57):
    """2^scale vertices, R-MAT x 16 edges, the last vertices given columns of exactly CRAFTED_DEGREES edges and one hub
    column of HUB_DEGREE -> (ptrs, idx, n, crafted vertex ids, hub vertex id)."""
    import orc
    n = 1 << scale
    row, col = orc.rmat_edges(scale, n * 16, seed)
    crafted = np.arange(n - len(CRAFTED_DEGREES) - 1, n - 1, dtype=np.int64)
    hub = n - 1
    keep = col < crafted[0]
    rs = np.random.default_rng(seed)
    rows, cols = [row[keep]], [col[keep]]
    for v, d in list(zip(crafted, CRAFTED_DEGREES)) + [(hub, HUB_DEGREE)]:
        rows.append(rs.integers(0, n, d))
        cols.append(np.full(d, v, dtype=np.int64))
    ptrs, idx, _ = orc.to_csc(np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int64), n)
    assert np.array_equal(np.diff(ptrs)[crafted], CRAFTED_DEGREES) and ptrs[hub + 1] - ptrs[hub] == HUB_DEGREE
    return ptrs, idx, n, crafted, hub


def recent_test_times(ptrs, hub, kind, seed=5):
    """ties: values in [0, 8).  asc / desc: distinct values, the hub column ascending (every chunk displaces entries of a
    most-recent-first list) or descending (no chunk after the first is a candidate) by edge pointer.  wide: c + j * 2**33
    with c and j of both signs, |t| <= 2**61 -- a key cut to 32 bits, or compared as unsigned, orders these wrongly."""
    rs = np.random.default_rng(seed)
    E = int(ptrs[-1])
    if kind == "ties":
        return rs.integers(0, 8, E).astype(np.int64)
    if kind == "wide":
        return (rs.integers(-1000, 1001, E) + rs.integers(-(1 << 27), (1 << 27) + 1, E) * (1 << 33)).astype(np.int64)
    ts = rs.permutation(E).astype(np.int64)
    a, b = int(ptrs[hub]), int(ptrs[hub + 1])
    ts[a:b] = np.sort(ts[a:b]) if kind == "asc" else np.sort(ts[a:b])[::-1]
    return ts
