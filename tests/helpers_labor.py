"""NumPy restatement of TG_SAMPLER_LABOR / TG_SAMPLER_LABOR_SHARED (include/tchgeo.h at the defines): layer-neighbor
sampling.  A vectorised Philox4x32-10, the key of a neighbour, one hop (helpers_recent.recent_hop with the key in the
timestamp's place and the filter on the real times) and the reference's loop over hops around it.  Deliberately plain."""
import numpy as np

from helpers_recent import CRAFTED_DEGREES, HUB_DEGREE, admitted, recent_test_graph  # noqa: F401

FILTER_NONE, FILTER_STATIC, FILTER_RELATIVE, FILTER_DYNAMIC = -1, 0, 1, 2
SAMPLER_LABOR, SAMPLER_LABOR_SHARED = 4, 5
TAG_LABOR = 14
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (or scalars) of 32-bit words held in uint64 -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) & M32 for a in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0           # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def call_key(seed, call_id, tag):
    """DESIGN.md "Randomness": Philox(key = seed, counter = (call id, tag, "tchg")), words 0 and 1"""
    seed, call_id = np.asarray(seed, dtype=np.uint64), np.asarray(call_id, dtype=np.uint64)
    w = philox4x32_10(call_id, call_id >> np.uint64(32), np.uint64(tag), np.uint64(0x74636867), seed, seed >> np.uint64(32))
    return w[0], w[1]


def named_draw(seed, call_id, tag, ids, d0, d1):
    """the four words of the draw (seed, call id, tag, id, d0, d1), vectorised over every argument"""
    k0, k1 = call_key(seed, call_id, tag)
    ids = np.asarray(ids).astype(np.uint64)
    return philox4x32_10(d0, d1, ids, ids >> np.uint64(32), k0, k1)


def labor_key(seed, call_id, t, layer, tag=TAG_LABOR, bits=63):
    """key of neighbour t: the low 64 bits of the draw (call key of (seed, call id, tag), id = t, d0 = layer, d1 = 0),
    shifted right by one: a non-negative int64.  bits < 63 keeps only the top `bits` (the negative control of the law)."""
    w = named_draw(seed, call_id, tag, t, layer, 0)
    a = w[0] | (w[1] << np.uint64(32))
    return (a >> np.uint64(64 - bits)).astype(np.int64)


def labor_hop(ptrs, idx, ts, vertices, states, k, seed, call_ids, layer, filter_mode=FILTER_NONE, forward=False,
              window=(0, 0), tag=TAG_LABOR, bits=63):
    """-> (cnt[m], offsets[m + 1], neighbors, edge_ptrs, parents, states_out), grouped by frontier vertex in rank order.
    call_ids: one per frontier vertex, or a scalar.  vertices < 0 are empty slots; ts / states may be None without a
    filter (states_out is then all 0)."""
    ptrs, idx = np.asarray(ptrs, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    vertices = np.asarray(vertices, dtype=np.int64)
    call_ids = np.broadcast_to(np.asarray(call_ids, dtype=np.uint64), vertices.shape)
    # every key of the hop in one vectorised pass: one per (frontier vertex, edge of its column)
    w = np.maximum(vertices, 0)
    deg = np.where(vertices >= 0, ptrs[w + 1] - ptrs[w], 0)
    start = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    owner = np.repeat(np.arange(len(vertices)), deg)
    edges = ptrs[w][owner] + (np.arange(start[-1], dtype=np.int64) - start[owner])
    keys_all = labor_key(seed, call_ids[owner], idx[edges], layer, tag, bits)
    cnt, nbr, eps, par, sto = [], [], [], [], []
    for i, v in enumerate(vertices):
        if v < 0:
            cnt.append(0)
            continue
        s = 0 if states is None else int(states[i])
        e, keys = edges[start[i]:start[i + 1]], keys_all[start[i]:start[i + 1]]
        if filter_mode != FILTER_NONE:
            ok = admitted(np.asarray(ts, dtype=np.int64)[e], s, filter_mode, forward, window)
            e, keys = e[ok], keys[ok]
        e = e[np.lexsort((e, keys))][:k]              # the smaller key first; ties: the smaller edge pointer
        cnt.append(len(e))
        nbr.append(idx[e])
        eps.append(e)
        par.append(np.full(len(e), i, dtype=np.int64))
        sto.append(np.asarray(ts, dtype=np.int64)[e] if filter_mode == FILTER_DYNAMIC else np.full(len(e), s, dtype=np.int64))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.empty(0, dtype=np.int64)
    cnt = np.asarray(cnt, dtype=np.int64).reshape(-1)
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return cnt, offsets, cat(nbr), cat(eps), cat(par), cat(sto)


def labor_ns_homo(ptrs, idx, ts, seeds, fanout, seed, call_id, sampler=SAMPLER_LABOR, seeds_state=None,
                  filter_mode=FILTER_NONE, forward=False, window=(0, 0), tag=TAG_LABOR):
    """The reference's loop over hops (neighbor_sampling.rs:188-223) with labor_hop as the sampler, layer = the hop for
    SAMPLER_LABOR and 0 for SAMPLER_LABOR_SHARED -> (samples, rows, cols, edge_index, layer_offsets, counts, states)."""
    seeds = np.asarray(seeds, dtype=np.int64)
    n_seeds = len(seeds)
    samples = [seeds]
    states = [np.zeros(n_seeds, dtype=np.int64) if seeds_state is None else np.asarray(seeds_state, dtype=np.int64)]
    rows, cols, eidx, layer_offsets = [], [], [], []
    begin, ne = 0, 0
    frontier, fstate = samples[0], states[0]
    for h, k in enumerate(fanout):
        layer_offsets.append((n_seeds + ne, ne, n_seeds + ne))
        layer = h if sampler == SAMPLER_LABOR else 0
        cnt, off, nbr, ep, par, sto = labor_hop(ptrs, idx, ts, frontier, fstate, int(k), seed, call_id, layer, filter_mode,
                                                forward, window, tag)
        tot = int(off[-1])
        rows.append(np.arange(n_seeds + ne, n_seeds + ne + tot, dtype=np.int64))
        cols.append(begin + par)
        eidx.append(ep)
        samples.append(nbr)
        states.append(sto)
        begin += len(frontier)
        ne += tot
        frontier, fstate = nbr, sto
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.empty(0, dtype=np.int64)
    return (cat(samples), cat(rows), cat(cols), cat(eidx), layer_offsets, (n_seeds + ne, ne), cat(states))


# ---- the graph of the device tests
def long_degrees(LONG):
    return (LONG - 1, LONG, LONG + 1, 2 * LONG + 63, 16 * LONG + 17)


def labor_test_graph(LONG, scale=10, seed=0x1AB0):
    """helpers_recent.recent_test_graph (R-MAT, the crafted degrees, the hub) with more columns appended as NEW vertices
    (they have columns but are nobody's neighbour): the long-column threshold's neighbourhood, one column made of the same
    neighbour 70 times (equal keys throughout: pure pointer order), two columns that share 200 neighbours among 260 / 300.
    -> dict(ptrs, idx, n (vertices in all), base (recent_test_graph's), crafted, hub, long, same, shared)"""
    ptrs, idx, n0, crafted, hub = recent_test_graph(scale)
    rs = np.random.default_rng(seed)
    cols = [rs.integers(0, n0, d).astype(np.int64) for d in long_degrees(LONG)]
    cols.append(np.full(70, 5, dtype=np.int64))
    common = rs.permutation(n0)[:320].astype(np.int64)
    cols.append(rs.permutation(np.concatenate([common[:200], common[200:260]])))
    cols.append(rs.permutation(np.concatenate([common[:200], common[260:320], common[:40]])))   # 40 parallel edges
    new_ptrs = np.concatenate([ptrs, ptrs[-1] + np.cumsum([len(c) for c in cols])]).astype(np.int64)
    new_idx = np.concatenate([idx] + cols).astype(np.int64)
    first = n0
    return dict(ptrs=new_ptrs, idx=new_idx, n=n0 + len(cols), base=n0, crafted=crafted, hub=hub,
                long=np.arange(first, first + 5, dtype=np.int64), same=first + 5,
                shared=(first + 6, first + 7), common=common[:200])
