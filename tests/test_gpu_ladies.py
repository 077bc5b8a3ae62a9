"""tg_ladies_count / tg_ladies_emit on hand-built graphs: every output word (n_nodes, n_edges, n_cand, total, chunks,
nodes_out, node_count, node_weight, rows, cols, edge_index, edge_weight as bits, the status word, and sentinel words before
and after every written range) equals the NumPy restatement (helpers_ladies).  The main graph has a hub column of six
chunks whose sources repeat across its chunks and reappear in other columns, a run of 80 empty columns, self loops, parallel
edges and sources that are frontier nodes; the laws are tested on the nested graph with exact_laws.chi2_gof."""
import numpy as np
import pytest
import torch

import exact_laws
import helpers_ladies as hl
from helpers_ladies import CHUNK, HUB, N, chunk_bound, refused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7            # the sentinel word (-7.0f in edge_weight)
GAP = 3              # sentinel words before, between and after the batches' ranges
SEED = 0x1AD1E5
# the widths of the scans used: a wave step of a chunk (64 entries), a chunk (512), the draw's workgroup (1 024 slots a
# pass) and a tile of chunks (1 024 chunks: test_columns_at_the_tile_and_unit_seams)
WIDTHS = (64, 512, 1024)


def graph_dict(ptrs, indices):
    from tch_geometric import _cabi, _cabi_ladies
    dp, di = torch.from_numpy(ptrs).to(DEV), torch.from_numpy(indices).to(DEV)
    plain = _cabi.graph_view(dp, di)
    shadow = _cabi.graph_view(dp, di, indices32=di.to(torch.int32), ptrs32=dp.to(torch.int32))
    return dict(ops=_cabi_ladies, ptrs=ptrs, indices=indices, plain=plain, shadow=shadow, prep={}, done={}, dev_w={})


@pytest.fixture(scope="module")
def K():
    k = graph_dict(*hl.ladies_test_graph())
    k["order"] = hl.frontier_order()
    return k


def rules(K, lists, s, call_ids, weights, id_bound):
    """the restatement of every list of a launch; the draw-independent part is computed once per distinct list, the picks
    of all its batches in one vectorised Philox call, the rest once per distinct selection"""
    wkey = None if weights is None else id(weights)
    groups = {}
    for b, nodes in enumerate(lists):
        key = (nodes.tobytes(), wkey, id_bound)
        if key not in K["prep"]:
            K["prep"][key] = hl.prepare(K["ptrs"], K["indices"], weights, nodes, id_bound=id_bound)
        groups.setdefault(key, []).append(b)
    out = [None] * len(lists)
    for key, members in groups.items():
        p = K["prep"][key]
        sel = None
        if p.S and p.cand.size:
            sel = hl.select(p, hl.draw_t(SEED, np.array([call_ids[b] for b in members], dtype=np.uint64), s, p.S))
        for i, b in enumerate(members):
            done = key + (s, None if sel is None else sel[i].tobytes())
            if done not in K["done"]:
                K["done"][done] = hl.finish(p, s, None, sel=None if sel is None else sel[i])
            out[b] = K["done"][done]
    return out


def rule(K, nodes, s, call_id, weights, id_bound):
    return rules(K, [nodes], s, [call_id], weights, id_bound)[0]


def need_of(r, id_bound=N):
    return r["n"] + min(r["m"], id_bound)


def run(K, lists, s, max_nodes=None, node_cap=None, chunk_cap=0, id_bound=None, shadows=True, with_nodes=True, base=0,
        weights=None, call_id=1000, stride=1):
    """one launch of the pair over `lists`, every word compared -> (expected per batch, refused per batch)"""
    ops = K["ops"]
    n_major = K["ptrs"].size - 1
    id_bound = n_major if id_bound is None else id_bound
    G = len(lists)
    max_nodes = max([l.size for l in lists] + [0]) if max_nodes is None else max_nodes
    want = rules(K, [l[:max_nodes] for l in lists], s, [call_id + b * stride for b in range(G)], weights, id_bound)
    if node_cap is None:
        node_cap = max([need_of(w, id_bound) for w in want] + [max_nodes])
    bound = chunk_bound(max_nodes, K["indices"].size, chunk_cap)
    no = [refused(w["n"], w["m"], w["chunks"], node_cap, bound, id_bound) for w in want]
    status = 1 if any(no) else 0
    for r, w in zip(no, want):
        status |= w["status"] & (2 if r else 6)
    flat = np.concatenate([np.full(base, 10 ** 12, np.int64)] + list(lists) + [np.zeros(0, np.int64)])
    node_ptr = base + np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.int64)
    dw = None
    if weights is not None:
        if id(weights) not in K["dev_w"]:
            K["dev_w"][id(weights)] = (weights, torch.from_numpy(weights).to(DEV))
        dw = K["dev_w"][id(weights)][1]
    op = ops.Ladies(K["shadow" if shadows else "plain"], id_bound, max_nodes, node_cap, chunk_cap, s, G, DEV, weights=dw)
    n_nodes, n_edges, n_cand, total, chunks, st = op.count(torch.from_numpy(flat).to(DEV), torch.from_numpy(node_ptr).to(DEV),
                                                           SEED, call_id, call_stride=stride)
    assert n_nodes.cpu().tolist() == [0 if r else w["out_nodes"].size for r, w in zip(no, want)]
    assert n_edges.cpu().tolist() == [w["m"] if r else w["rows"].size for r, w in zip(no, want)]   # refused: all its triples
    assert n_cand.cpu().tolist() == [0 if r else w["n_cand"] for r, w in zip(no, want)]
    assert total.cpu().tolist() == [0 if r else w["total"] for r, w in zip(no, want)]
    assert chunks.cpu().tolist() == [w["chunks"] for w in want]
    assert int(st.cpu()[0]) == status
    # the caller's prefixes, with GAP sentinel words around every range
    gap_n, gap_e, gap_w = np.full((3, GAP), SENT), np.full((3, GAP), SENT), np.full(GAP, SENT, np.float32)
    exp_nodes, exp_trip, exp_w, node_off, edge_off = [gap_n], [gap_e], [gap_w], [], []
    n_at, e_at = GAP, GAP
    for r, w in zip(no, want):
        node_off.append(n_at)
        edge_off.append(e_at)
        if not r:
            exp_nodes.append(np.stack([w["out_nodes"], w["node_count"], w["node_weight"]]))
            exp_trip.append(np.stack([w["rows"], w["cols"], w["edge_index"]]))
            exp_w.append(w["edge_weight"])
            n_at += w["out_nodes"].size
            e_at += w["rows"].size
        exp_nodes.append(gap_n)
        exp_trip.append(gap_e)
        exp_w.append(gap_w)
        n_at, e_at = n_at + GAP, e_at + GAP
    exp_nodes, exp_trip, exp_w = np.concatenate(exp_nodes, axis=1), np.concatenate(exp_trip, axis=1), np.concatenate(exp_w)
    o = dict(dtype=torch.int64, device=DEV)
    per_node = torch.full((3, exp_nodes.shape[1]), SENT, **o)
    trip = torch.full((3, exp_trip.shape[1]), SENT, **o)
    ew = torch.full((exp_w.size,), float(SENT), dtype=torch.float32, device=DEV)
    for _ in range(2):                                               # emit only reads the workspace: a second one writes the same
        op.emit(torch.tensor(node_off, **o) if with_nodes else None, torch.tensor(edge_off, **o),
                per_node[0] if with_nodes else None, per_node[1] if with_nodes else None, per_node[2] if with_nodes else None,
                trip[0], trip[1], trip[2], ew)
        assert np.array_equal(trip.cpu().numpy(), exp_trip)
        assert np.array_equal(ew.cpu().numpy().view(np.uint32), exp_w.view(np.uint32))
        assert np.array_equal(per_node.cpu().numpy(), exp_nodes if with_nodes else np.full(exp_nodes.shape, SENT))
    return want, no


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 513, 1025])
def test_frontier_sizes(K, n):
    want, no = run(K, [K["order"][:n]], 96)
    assert not any(no) and want[0]["out_nodes"].size >= n
    if n >= 3:
        assert want[0]["rows"].size > 0 and (want[0]["node_count"][:n] > 0).any()     # frontier nodes are drawn


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 512, 4096, 8192])
def test_budgets(K, s):
    want, no = run(K, [K["order"][:90], K["order"][200:203], K["order"][83:84]], s)
    assert not any(no) and all(int(w["node_count"].sum()) == s for w in want if w["total"])
    if s == 8192:
        assert want[2]["n_cand"] < s and (want[2]["node_count"][1:] > 0).all()   # s above the candidate count: all drawn
        assert want[0]["n_cand"] < s


@pytest.fixture(scope="module")
def widths():
    """column v holds the sources 0 .. d_v - 1 for d one below, at and above every width of WIDTHS: a frontier of one
    column has exactly d candidates.  uni: weights that make every q_e = 1, so S = n_cand and every boundary of P is hit"""
    degs = [w + k for w in WIDTHS for k in (-1, 0, 1)]
    n = max(degs) + len(degs)
    cols = [np.arange(d, dtype=np.int64) + len(degs) for d in degs] + [np.zeros(0, np.int64)] * (n - len(degs))
    ptrs = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    k = graph_dict(ptrs, np.concatenate(cols))
    k["degs"], k["uni"] = degs, np.full(int(ptrs[-1]), 2.0 ** -16, np.float32)
    return k


@pytest.mark.parametrize("weighted", [False, True], ids=["row-normalised", "q=1"])
def test_candidate_counts_around_every_width(widths, weighted):
    degs = widths["degs"]
    assert degs == [63, 64, 65, 511, 512, 513, 1023, 1024, 1025]
    lists = [np.array([v], dtype=np.int64) for v in range(len(degs))] + [np.arange(len(degs), dtype=np.int64)]
    want, no = run(widths, lists, 8192, weights=widths["uni"] if weighted else None)
    assert not any(no) and [w["n_cand"] for w in want[:-1]] == degs
    if weighted:
        assert [w["total"] for w in want[:-1]] == degs                # S = n_cand
        assert all((w["node_count"][1:] > 0).sum() > 0.99 * d for w, d in zip(want, degs))
        assert (want[0]["node_count"][1:] > 0).all() and want[0]["node_count"].size == 1 + 63   # every boundary was hit


def _weights(K, kind):
    rs = np.random.default_rng(17)
    E = K["indices"].size
    w = (rs.random(E) * 1.4).astype(np.float32)                      # some above 1: they count as 1 in the law
    if kind == "zeros-between":
        w[np.isin(K["indices"], np.arange(100, 400, 2))] = 0.0       # every other hub source has W = 0
    elif kind == "nan-negative":
        w[::3], w[1::7] = np.nan, -0.5
    elif kind == "S=0":
        w[:] = np.where(np.arange(E) % 2 == 0, 0.0, -1.0)
        w[::5] = np.nan
    return w


@pytest.mark.parametrize("kind", ["plain", "zeros-between", "nan-negative", "S=0"])
def test_weighted_mode(K, kind):
    key = "w_" + kind
    if key not in K:
        K[key] = _weights(K, kind)
    want, no = run(K, [K["order"][:90], K["order"][500:520]], 700, weights=K[key])
    assert not any(no)
    w0 = want[0]
    if kind == "zeros-between":
        zero = (w0["node_weight"] == 0) & (np.arange(w0["out_nodes"].size) >= 90)
        assert not zero.any()                                         # a candidate of weight 0 is never selected
        p = K["prep"][(K["order"][:90].tobytes(), id(K[key]), N)]
        assert ((p.W == 0)[:-1] & (p.W > 0)[1:]).sum() > 50           # ... though many sit between positive ones
    if kind == "S=0":
        assert w0["status"] == 4 and w0["total"] == 0 and w0["n_cand"] > 0 and w0["rows"].size == 0
    if kind == "nan-negative":
        assert np.isnan(w0["edge_weight"]).any() and (w0["edge_weight"] < 0).any()   # kept entries carry their own w_e


def test_total_above_2_54():
    n = 16385 + 3
    ptrs = np.concatenate([np.arange(16386), [16385, 16385, 16385]]).astype(np.int64)
    k = graph_dict(ptrs, (np.arange(16385, dtype=np.int64) * 7 + 3) % n)
    want, no = run(k, [np.arange(16385, dtype=np.int64)], 4096)
    assert not any(no) and want[0]["total"] == 16385 << 40 and want[0]["total"] > 2 ** 54 and want[0]["n_cand"] == 16385


def test_ids_out_of_range_raise_bit_1(K):
    nodes = np.array([1, N, -1, 2, 2 ** 40, HUB], dtype=np.int64)
    want, no = run(K, [nodes, K["order"][:5]], 50)
    assert want[0]["status"] == 2 and want[1]["status"] == 0 and not any(no)


def test_frontier_ids_between_n_major_and_id_bound(K):
    nodes = np.array([1, N + 5, 2], dtype=np.int64)
    want, no = run(K, [nodes], 50, id_bound=N + 10)
    assert want[0]["status"] == 2 and not any(no)


@pytest.mark.parametrize("short", [1, 0])
def test_node_cap_one_below_and_at_the_need(K, short):
    lists = [K["order"][3:9], K["order"][:90], K["order"][100:130]]
    needs = [need_of(rule(K, l, 40, 1000 + b, None, N)) for b, l in enumerate(lists)]
    assert needs[1] > max(needs[0], needs[2])
    want, no = run(K, lists, 40, node_cap=needs[1] - short, chunk_cap=1000)
    assert no == [False, bool(short), False]                          # the neighbours of the refused batch are intact


@pytest.mark.parametrize("short", [1, 0])
def test_chunk_cap_one_below_and_at_the_need(K, short):
    lists = [K["order"][83:90], K["order"][:90], K["order"][100:110]]
    chunks = [rule(K, l, 40, 1000 + b, None, N)["chunks"] for b, l in enumerate(lists)]
    assert chunks[1] > max(chunks[0], chunks[2]) and chunks[1] - short >= 1
    want, no = run(K, lists, 40, node_cap=5000, chunk_cap=chunks[1] - short)
    assert no == [False, bool(short), False]


def test_ragged_lists_a_base_a_stride_and_a_list_longer_than_max_nodes(K):
    order = K["order"]
    lists = [order[200:205], order[:40], np.zeros(0, np.int64), order[300:303]]
    want, no = run(K, lists, 33, max_nodes=10, base=17, stride=3)
    assert not any(no) and want[1]["out_nodes"][:10].tolist() == order[:10].tolist() and want[1]["n"] == 10


@pytest.mark.parametrize("G", [1, 3, 300, 32773])
def test_batch_counts(K, G):
    order = K["order"]
    if G == 32773:                                                   # tiny frontiers, one slot: the rounds of 32 768
        kinds = [order[90 + j:90 + j + j % 3] for j in range(7)]
        lists, s = [kinds[b % 7] for b in range(G)], 1
    else:
        rs = np.random.default_rng(G)
        lists, s = [order[int(a):int(a) + int(k)] for a, k in zip(rs.integers(0, 1100, G), rs.integers(0, 21, G))], 9
    want, no = run(K, lists, s)
    assert not any(no)
    if G == 32773:                                                   # the draws differ from batch to batch, also past a round
        assert len({w["out_nodes"].tobytes() for w in want}) > 20 and len({w["out_nodes"].tobytes() for w in want[32768:]}) > 3


def test_key_widths_and_shadows_agree(K):
    lists = [K["order"][:70], K["order"][500:520]]
    a, _ = run(K, lists, 128)
    b, _ = run(K, lists, 128, id_bound=2 ** 31 + 1)                  # 64-bit keys
    c, _ = run(K, lists, 128, shadows=False)
    d, _ = run(K, lists, 128, id_bound=2 ** 31 + 1, shadows=False)
    for other in (b, c, d):
        assert all(hl.same(x, y) for x, y in zip(a, other))


def test_node_outputs_may_be_null(K):
    run(K, [K["order"][:70], K["order"][500:520]], 128, with_nodes=False)


@pytest.fixture(scope="module")
def seams():
    """columns 0 .. 3 of 1 024 * 512, 1 024 * 512 + 1, 16 * 512 and 16 * 512 + 1 entries, built on the device: the chunk
    prefixes (candidates, their W, kept entries) end with a tile, have a second tile of one chunk of one entry, are one unit,
    are a unit and one chunk.  A column's last entry is a source that it names nowhere else"""
    n = 3000
    deg = [1024 * CHUNK, 1024 * CHUNK + 1, 16 * CHUNK, 16 * CHUNK + 1]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(13)
    di = torch.randint(4, n - 8, (sum(deg),), device=DEV, generator=gen)
    dp = torch.full((n + 1,), sum(deg), dtype=torch.int64, device=DEV)
    dp[:5] = torch.tensor([0] + np.cumsum(deg).tolist(), device=DEV)
    di[dp[1:5] - 1] = torch.arange(n - 4, n, device=DEV)
    return graph_dict(dp.cpu().numpy(), di.cpu().numpy())


def test_columns_at_the_tile_and_unit_seams(seams):
    lists = [np.array([v], dtype=np.int64) for v in range(4)] + [np.array([3, 1, 2], dtype=np.int64)]
    want, no = run(seams, lists, 2048)
    assert not any(no) and [w["chunks"] for w in want] == [1024, 1025, 16, 17, 17 + 1025 + 16]
    assert want[1]["rows"].size > 1024 * CHUNK // 4                   # kept entries in every chunk of both tiles


# ---- the laws, on the nested graph: G mini-batches of the frontier 0 .. 5 in one launch
N_LAW = 1 << 16


def _nested_counts(s):
    """-> per mini-batch the drawn nodes' counts [N_LAW, 12]"""
    ptrs, indices, law = hl.nested_graph()
    k = graph_dict(ptrs, indices)
    front = np.arange(6, dtype=np.int64)
    G = N_LAW
    op = k["ops"].Ladies(k["shadow"], 12, 6, 6 + 12, 0, s, G, DEV)
    flat = torch.from_numpy(np.tile(front, G)).to(DEV)
    node_ptr = torch.arange(0, 6 * G + 1, 6, device=DEV)
    n_nodes, n_edges, n_cand, total, _, st = op.count(flat, node_ptr, SEED, 77)
    assert int(st.cpu()[0]) == 0 and bool((n_cand == 12).all()) and bool((total == total[0]).all())
    node_off, edge_off = torch.cumsum(n_nodes, 0) - n_nodes, torch.cumsum(n_edges, 0) - n_edges
    o = dict(dtype=torch.int64, device=DEV)
    nt, et = int(n_nodes.sum()), int(n_edges.sum())
    nodes_out, cnt, rows = torch.empty(nt, **o), torch.empty(nt, **o), torch.empty((3, et), **o)
    op.emit(node_off, edge_off, nodes_out, cnt, None, rows[0], rows[1], rows[2], torch.empty(et, dtype=torch.float32, device=DEV))
    batch = torch.repeat_interleave(torch.arange(G, device=DEV), n_nodes)
    counts = torch.zeros((G, 12), **o)
    counts.index_put_((batch, nodes_out), cnt, accumulate=True)
    assert bool((counts.sum(1) == s).all())
    # one mini-batch in full against the restatement
    r = hl.ladies_rule(ptrs, indices, None, front, s, SEED, 77 + 12345)
    got = counts[12345].cpu().numpy()
    exp = np.zeros(12, np.int64)
    np.add.at(exp, r["out_nodes"], r["node_count"])
    assert np.array_equal(got, exp)
    return counts.cpu().numpy(), np.array([float(p) for p in law])


def test_one_slot_law():
    counts, law = _nested_counts(1)
    exact_laws.chi2_gof(counts.sum(0), law, "one slot against W_u / S")


def test_two_slot_product_law():
    """the slots are independent: the unordered pair {u, v} has probability p_u^2 (u = v) or 2 p_u p_v"""
    counts, law = _nested_counts(2)
    cat = {}
    probs = []
    for u in range(12):
        for v in range(u, 12):
            cat[(u, v)] = len(probs)
            probs.append(law[u] * law[v] * (1 if u == v else 2))
    first = counts.argmax(1)                                         # the smaller id of the pair (or the one drawn twice)
    rest = counts.copy()
    rest[np.arange(N_LAW), first] -= 1
    second = rest.argmax(1)
    lo, hi = np.minimum(first, second), np.maximum(first, second)
    ids = np.array([cat[(a, b)] for a, b in zip(lo.tolist(), hi.tolist())])
    exact_laws.chi2_gof(np.bincount(ids, minlength=len(probs)), np.array(probs), "two slots against the product law")
