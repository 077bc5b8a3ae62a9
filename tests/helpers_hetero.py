"""Two oracle-free tools for neighbor_sampling_heterogenous under a temporal filter or the weighted sampler.

worst_case_bounds   restates the sizing recursion of the driver (host/python_module.cpp, the device-driven branch of
                    neighbor_sampling_heterogenous), so a test can assert which route its shape takes: packed or
                    padded frontier per round, short or long scans, first or eightfold group bound, device- or
                    host-driven.
check_hetero_result validates a returned (samples, rows, cols, edge_index, layer_offsets) from the inputs and the
                    graphs alone.  It knows nothing of oracle/ or of Philox; the rules are written from the
                    reference's Rust:
                      neighbor_sampling.rs:55-67   TemporalFilter::filter (inclusive window; STATIC on t, RELATIVE and
                                                   DYNAMIC on t - state forward, -(t - state) backward)
                      neighbor_sampling.rs:69-76   TemporalFilter::mutate (the state carried to a sample)
                      neighbor_sampling.rs:292-349 the hop / relation loop: layer offsets, append order, slices
                      utils/sampling.rs:6-26       reservoir_sampling returns min(k, candidates), distinct candidates
                      utils/sampling.rs:28-55      reservoir_sampling_weighted: the first k candidates fill the
                                                   reservoir whatever their weight, a later one enters only if
                                                   j < w, so never with weight 0; min(k, candidates), distinct
                      utils/sampling.rs:57-69      replacement_sampling: k draws if there is any candidate
                      neighbor_sampling.rs:118-122 ... and none otherwise
"""
import numpy as np

FILTER_STATIC, FILTER_RELATIVE, FILTER_DYNAMIC = 0, 1, 2

# include/tchgeo.h ("layout_dev ... Needs m <= 2^17 and group_cap <= 2^20"); python_module.cpp, flush() in the
# all_at_once branch: lay = (m_round <= 1 << 17 && groups_of_hop(h) <= 1 << 20) ? layout : nullptr
PACKED_M_MAX = 1 << 17
PACKED_GROUPS_MAX = 1 << 20
# python_module.cpp, device-driven branch: "if (fr > 0 && k > ((int64_t)1 << 40) / fr) affordable = false" and
# "if (affordable && words * 8 <= 8e9 && ...)"
AFFORDABLE_PRODUCT = 1 << 40
AFFORDABLE_BYTES = 8e9
# include/tchgeo.h: TG_HET_HOP_MAX_ENTRIES, TG_HOP_MAX_SEGMENTS
ROUND_MAX_ENTRIES = 16
ROUND_MAX_SEGMENTS = 8
GROUP_EDGES = 512


def rel_key(et):
    return "%s__%s__%s" % tuple(et)


def group_bound(m, edges_over_512, mult=1):
    """groups_of_hop: group_mult * max(1024, sum E_r / 512 + 2 m + 2)"""
    return mult * max(1024, edges_over_512 + 2 * m + 2)


def _round(m_round, entries, segments, gb):
    """one begin / sample / end round of a hop; packed: python_module.cpp, flush(): both bounds within the layout's"""
    return dict(m_round=m_round, entries=entries, segments=segments,
                packed=m_round <= PACKED_M_MAX and gb <= PACKED_GROUPS_MAX)


def worst_case_bounds(node_types, edge_types, num_neighbors, num_hops, n_inputs, n_edges, has_state, group_mult=1):
    """num_neighbors / n_edges: dict by relation key; n_inputs: dict by node type (missing = 0).

    Returns a dict: hop_m[h], group_bound[h] (times group_mult), rounds[h] = [{m_round, entries, segments, packed}],
    words, bytes, affordable, route ("device" | "host")."""
    T = {t: i for i, t in enumerate(node_types)}
    rels = [(rel_key(et), T[et[0]], T[et[2]]) for et in edge_types]
    R, H = len(rels), num_hops
    fsz = [int(n_inputs.get(t, 0)) for t in node_types]
    cap_list = list(fsz)
    cap_e = [0] * R
    cap_f = [[0] * R for _ in range(H)]
    max_f = max_out = max_k = 1
    affordable = True
    for h in range(H):
        fresh = [0] * len(node_types)
        for r, (key, src, dst) in enumerate(rels):
            fr, k = fsz[dst], int(num_neighbors[key][h])
            if fr > 0 and k > AFFORDABLE_PRODUCT // fr:
                affordable = False
                break
            cap_f[h][r] = fr
            cap_e[r] += fr * k
            fresh[src] += fr * k
            max_f, max_out, max_k = max(max_f, fr), max(max_out, fr * k), max(max_k, k)
        if not affordable:
            break
        for t in range(len(node_types)):
            fsz[t] = fresh[t]
            cap_list[t] += fresh[t]
    words = float(sum(cap_list)) * (2 if has_state else 1) + 3.0 * sum(cap_e)
    words += (max_f * 5.0 + max_out * 4.0) * max(R, 1)        # filter / weights: one frontier buffer for R relations
    hop_m, bounds, rounds = [], [], []
    for h in range(H):
        m = sum(cap_f[h])
        g = sum(int(n_edges[key]) // GROUP_EDGES for r, (key, _, _) in enumerate(rels) if cap_f[h][r] > 0)
        gb = group_bound(m, g, group_mult)
        hop_m.append(m)
        bounds.append(gb)
        rr, ent, seg, m_round = [], 0, 0, 0
        for r in range(R):
            cf = cap_f[h][r]
            if ent == ROUND_MAX_ENTRIES or (cf > 0 and seg == ROUND_MAX_SEGMENTS):
                rr.append(_round(m_round, ent, seg, gb))
                ent = seg = m_round = 0
            if cf > 0:
                seg += 1
                m_round += cf
            ent += 1
        if ent:
            rr.append(_round(m_round, ent, seg, gb))
        rounds.append(rr)
    device = affordable and words * 8 <= AFFORDABLE_BYTES
    return dict(hop_m=hop_m, group_bound=bounds, rounds=rounds, words=words, bytes=words * 8, affordable=affordable,
                route="device" if device else "host", cap_f=cap_f)


def frontier_groups(col_ptrs, frontier):
    """sum over the frontier of ceil(deg / 512): the column groups one relation's frontier really needs"""
    P = np.asarray(col_ptrs, dtype=np.int64)
    v = np.asarray(frontier, dtype=np.int64)
    deg = P[v + 1] - P[v]
    return int(((deg + GROUP_EDGES - 1) // GROUP_EDGES).sum())


def admissible(ts, state, mode, forward, window):
    """neighbor_sampling.rs:55-67"""
    lo, hi = window
    if mode == FILTER_STATIC:
        d = ts
    elif forward:
        d = ts - state
    else:
        d = -(ts - state)
    return (d >= lo) & (d <= hi)


def _admissible_counts(P, verts, states, TS, flt):
    """admissible edges of column verts[i] seen from states[i], for every i (grouped by distinct (vertex, state))"""
    if flt is None:
        return P[verts + 1] - P[verts]
    mode, forward, window = flt["mode"], flt["forward"], flt["window"]
    if mode == FILTER_STATIC:
        keys, inv = np.unique(verts, return_inverse=True)
        uv, us = keys, np.zeros(len(keys), dtype=np.int64)
    else:
        keys, inv = np.unique(np.stack([verts, states], 1), axis=0, return_inverse=True)
        uv, us = keys[:, 0], keys[:, 1]
    inv = inv.reshape(-1)
    deg = P[uv + 1] - P[uv]
    out = np.zeros(len(uv), dtype=np.int64)
    step = 1 << 22                                            # bounded temporaries for hub columns
    start = 0
    while start < len(uv):
        stop, tot = start, 0
        while stop < len(uv) and (stop == start or tot + deg[stop] <= step):
            tot += deg[stop]
            stop += 1
        d = deg[start:stop]
        off = np.concatenate([[0], np.cumsum(d)])
        owner = np.repeat(np.arange(stop - start), d)
        pos = np.repeat(P[uv[start:stop]], d) + (np.arange(off[-1]) - off[owner])
        ok = admissible(TS[pos], us[start:stop][owner], mode, forward, window)
        out[start:stop] = np.bincount(owner, weights=ok, minlength=stop - start).astype(np.int64)
        start = stop
    return out[inv]


def check_hetero_result(node_types, edge_types, col_ptrs, row_indices, inputs, num_neighbors, num_hops, result,
                        replace=False, weights=None, flt=None, states=None):
    """Raises AssertionError naming the relation (or node type) at the first violated rule; returns the filter states
    the mode prescribes for every sample, per node type (None without a filter).

    flt: None or dict(mode, forward, window=(lo, hi), timestamps={relation: [E]}, inputs_state={type: [n]}).
    states: optional {type: array}, states a sampler reports for the samples; checked against the prescribed ones."""
    samples, rows, cols, eidx, los = result
    H = num_hops
    S = {t: np.asarray(samples[t], dtype=np.int64) for t in node_types}
    n_in = {t: len(np.asarray(inputs[t])) if t in inputs else 0 for t in node_types}
    for t in node_types:
        assert len(S[t]) >= n_in[t] and np.array_equal(S[t][:n_in[t]], np.asarray(inputs.get(t, []), dtype=np.int64)), \
            "type %s: samples do not start with the inputs" % t
    ST = None
    if flt is not None:
        ST = {t: np.full(len(S[t]), np.iinfo(np.int64).min, dtype=np.int64) for t in node_types}
        for t in node_types:
            if n_in[t]:
                ST[t][:n_in[t]] = np.asarray(flt["inputs_state"][t], dtype=np.int64)
    origin = {t: np.full(len(S[t]), -1, dtype=np.int64) for t in node_types}   # the relation that appended a sample
    length = dict(n_in)
    fbeg = {t: 0 for t in node_types}
    fend = dict(n_in)
    ne = {rel_key(et): 0 for et in edge_types}
    for h in range(H):
        for ri, et in enumerate(edge_types):
            key, src, dst = rel_key(et), et[0], et[2]
            who = "relation %s hop %d" % (key, h)
            P = np.asarray(col_ptrs[key], dtype=np.int64)
            I = np.asarray(row_indices[key], dtype=np.int64)
            RW, CL, EI = (np.asarray(a[key], dtype=np.int64) for a in (rows, cols, eidx))
            assert len(RW) == len(CL) == len(EI), "%s: rows / cols / edge_index differ in length" % who
            lo = [tuple(int(x) for x in q) for q in los[key]]
            assert len(lo) == H, "%s: %d layer offsets for %d hops" % (who, len(lo), H)
            want = (length[src], ne[key], length[dst])
            assert lo[h] == want, "%s: layer offset %s, the lists say %s" % (who, lo[h], want)
            e0 = lo[h][1]
            e1 = lo[h + 1][1] if h + 1 < H else len(RW)
            assert e0 <= e1 <= len(RW), "%s: edge slice [%d, %d) outside the %d edges" % (who, e0, e1, len(RW))
            n = e1 - e0
            k = int(num_neighbors[key][h])
            r_, c_, e_ = RW[e0:e1], CL[e0:e1], EI[e0:e1]
            assert np.array_equal(r_, np.arange(length[src], length[src] + n)), "%s: rows are not the append range" % who
            assert length[src] + n <= len(S[src]), "%s: rows run past samples[%s]" % (who, src)
            assert n == 0 or (c_.min() >= fbeg[dst] and c_.max() < fend[dst]), \
                "%s: cols outside the hop's frontier slice [%d, %d)" % (who, fbeg[dst], fend[dst])
            assert np.all(np.diff(c_) >= 0), "%s: cols do not ascend (the reference visits the frontier in order)" % who
            assert n == 0 or (e_.min() >= 0 and e_.max() < len(I)), "%s: edge_index outside the relation's edges" % who
            v = S[dst][c_]
            assert np.all((P[v] <= e_) & (e_ < P[v + 1])), "%s: edge_index outside the column of samples[dst][cols]" % who
            assert np.array_equal(S[src][r_], I[e_]), "%s: samples[src][rows] != row_indices[edge_index]" % who
            nf = fend[dst] - fbeg[dst]
            got = np.bincount(c_ - fbeg[dst], minlength=nf) if n else np.zeros(nf, dtype=np.int64)
            assert nf == 0 or got.max() <= k, "%s: a frontier vertex has more than %d edges" % (who, k)
            if not replace and n:
                pair = np.stack([c_, e_], 1)
                assert len(np.unique(pair, axis=0)) == n, "%s: an edge pointer is sampled twice for one vertex" % who
            fv = S[dst][fbeg[dst]:fend[dst]]
            fs = ST[dst][fbeg[dst]:fend[dst]] if flt is not None else None
            TS = np.asarray(flt["timestamps"][key], dtype=np.int64) if flt is not None else None
            adm = _admissible_counts(P, fv, fs, TS, flt)
            expect = np.where(adm > 0, k, 0) if replace else np.minimum(k, adm)
            bad = np.flatnonzero(got != expect)
            assert len(bad) == 0, "%s: frontier slot %d has %d edges, the rule gives %d (%d admissible, fan-out %d)" % (
                who, fbeg[dst] + (bad[0] if len(bad) else 0), got[bad[0]] if len(bad) else 0,
                expect[bad[0]] if len(bad) else 0, adm[bad[0]] if len(bad) else 0, k)
            if flt is not None:
                ps = ST[dst][c_]
                ok = admissible(TS[e_], ps, flt["mode"], flt["forward"], flt["window"])
                assert np.all(ok), "%s: edge %d is not admissible for its parent's state" % (who, e0 + int(np.argmin(ok)) if n else 0)
                ST[src][r_] = TS[e_] if flt["mode"] == FILTER_DYNAMIC else ps      # neighbor_sampling.rs:69-76
            if weights is not None:
                W = np.asarray(weights[key], dtype=np.float64)
                for j in np.flatnonzero(W[e_] == 0):         # legal only from the fill of the first k candidates
                    col = np.arange(P[v[j]], P[v[j] + 1])
                    if flt is not None:
                        col = col[admissible(TS[col], ST[dst][c_[j]], flt["mode"], flt["forward"], flt["window"])]
                    assert e_[j] in col[:k], "%s: zero-weight edge %d sampled after the reservoir was full" % (who, e_[j])
            origin[src][r_] = ri
            length[src] += n
            ne[key] += n
        for t in node_types:                                 # neighbor_sampling.rs:345-348
            fbeg[t], fend[t] = fend[t], length[t]
    for t in node_types:
        assert len(S[t]) == length[t], "type %s: %d samples, the edges account for %d" % (t, len(S[t]), length[t])
    for et in edge_types:
        key = rel_key(et)
        assert len(np.asarray(rows[key])) == ne[key], "relation %s: %d edges, the hops account for %d" % (
            key, len(np.asarray(rows[key])), ne[key])
    if states is not None:
        assert flt is not None
        for t in node_types:
            got = np.asarray(states[t], dtype=np.int64)
            assert len(got) == len(ST[t]), "type %s: %d states for %d samples" % (t, len(got), len(ST[t]))
            bad = np.flatnonzero(got != ST[t])
            if len(bad):
                o = int(origin[t][bad[0]])
                raise AssertionError("%s: the state carried to samples[%s][%d] is %d, mode %d prescribes %d" % (
                    "relation " + rel_key(edge_types[o]) if o >= 0 else "inputs of type " + t, t, bad[0], got[bad[0]],
                    flt["mode"], ST[t][bad[0]]))
    return ST
