"""tg_ns_full_count / tg_ns_full_emit on one hand-built graph: every output word (n_nodes, n_edges, chunks, nodes_out, rows,
cols, edge_index, the status word, and sentinel words before and after every written range) equals the NumPy restatement
(helpers_full).  The graph has a hub column of six chunks whose sources repeat across its chunks and reappear in other
columns, a run of 80 empty columns, self loops, parallel edges and sources that are frontier nodes."""
import numpy as np
import pytest
import torch

from helpers_full import CHUNK, chunk_bound, chunks_of, full_rule, refused, status_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1200
HUB, EMPTY0, EMPTY1 = 0, 400, 480
SENT = -7            # the sentinel word
GAP = 3              # sentinel words before, between and after the batches' ranges


def build_graph():
    rs = np.random.default_rng(11)
    cols = []
    for v in range(N):
        cols.append(np.zeros(0, np.int64) if EMPTY0 <= v < EMPTY1 else rs.integers(0, N, int(rs.integers(0, 41))))
    cols[HUB] = 100 + (np.arange(2600) * 7) % 300                # sources 100 .. 399, each eight or nine times, in every chunk
    cols[1] = np.array([1, 1, 0, 150, 150, 2])                   # a self loop twice (parallel), frontier nodes, a hub source twice
    cols[2] = np.array([2, 1, 0, 399])
    ptrs = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    return ptrs, np.concatenate(cols).astype(np.int64)


def frontier_order():
    rest = [v for v in np.random.default_rng(5).permutation(N).tolist() if v > 2 and not EMPTY0 <= v < EMPTY1]
    return np.array([HUB, 1, 2] + list(range(EMPTY0, EMPTY1)) + rest, dtype=np.int64)


@pytest.fixture(scope="module")
def K():
    from tch_geometric import _cabi
    ptrs, indices = build_graph()
    dp, di = torch.from_numpy(ptrs).to(DEV), torch.from_numpy(indices).to(DEV)
    plain = _cabi.graph_view(dp, di)
    shadow = _cabi.graph_view(dp, di, indices32=di.to(torch.int32), ptrs32=dp.to(torch.int32))
    return dict(cabi=_cabi, ptrs=ptrs, indices=indices, plain=plain, shadow=shadow, order=frontier_order(), cache={})


def rule(K, nodes):
    """the restatement of one list, computed once -> (out_nodes, rows, cols, edge_index, chunks, status)"""
    key = tuple(nodes.tolist())
    if key not in K["cache"]:
        K["cache"][key] = full_rule(K["ptrs"], K["indices"], nodes) + (chunks_of(K["ptrs"], nodes), status_of(K["ptrs"], nodes))
    return K["cache"][key]


def need_of(K, nodes, id_bound=N):
    out, rows = rule(K, nodes)[:2]
    return nodes.size + min(rows.size, id_bound)


def run(K, lists, max_nodes=None, node_cap=None, chunk_cap=0, id_bound=N, shadows=True, with_nodes=True, base=0):
    """one launch of the pair over `lists`, every word compared -> (expected per batch, refused per batch)"""
    cabi = K["cabi"]
    G = len(lists)
    max_nodes = max([l.size for l in lists] + [0]) if max_nodes is None else max_nodes
    eff = [l[:max_nodes] for l in lists]
    want = [rule(K, l) for l in eff]
    if node_cap is None:
        node_cap = max([need_of(K, l, id_bound) for l in eff] + [max_nodes])
    bound = chunk_bound(max_nodes, K["indices"].size, chunk_cap)
    no = [refused(l.size, w[1].size, w[4], node_cap, bound, id_bound) for l, w in zip(eff, want)]
    status = (1 if any(no) else 0)
    for w in want:
        status |= w[5]
    flat = np.concatenate([np.full(base, 10 ** 12, np.int64)] + list(lists) + [np.zeros(0, np.int64)])
    node_ptr = base + np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.int64)
    op = cabi.NsFull(K["shadow" if shadows else "plain"], id_bound, max_nodes, node_cap, chunk_cap, G, DEV)
    n_nodes, n_edges, chunks, st = op.count(torch.from_numpy(flat).to(DEV), torch.from_numpy(node_ptr).to(DEV))
    assert n_nodes.cpu().tolist() == [0 if r else w[0].size for r, w in zip(no, want)]
    assert n_edges.cpu().tolist() == [w[1].size for w in want]                    # exact, refused or not
    assert chunks.cpu().tolist() == [w[4] for w in want]
    assert int(st.cpu()[0]) == status
    # the caller's prefixes, with GAP sentinel words around every range
    exp_nodes, exp_trip, node_off, edge_off = [np.full(GAP, SENT)], [np.full((3, GAP), SENT)], [], []
    n_at, e_at = GAP, GAP
    for r, w in zip(no, want):
        node_off.append(n_at)
        edge_off.append(e_at)
        if not r:
            exp_nodes.append(w[0])
            exp_trip.append(np.stack(w[1:4]))
            n_at += w[0].size
            e_at += w[1].size
        exp_nodes.append(np.full(GAP, SENT))
        exp_trip.append(np.full((3, GAP), SENT))
        n_at, e_at = n_at + GAP, e_at + GAP
    exp_nodes, exp_trip = np.concatenate(exp_nodes), np.concatenate(exp_trip, axis=1)
    o = dict(dtype=torch.int64, device=DEV)
    nodes_out = torch.full((exp_nodes.size,), SENT, **o)
    trip = torch.full((3, exp_trip.shape[1]), SENT, **o)
    op.emit(torch.tensor(node_off, **o) if with_nodes else None, torch.tensor(edge_off, **o),
            nodes_out if with_nodes else None, trip[0], trip[1], trip[2])
    assert np.array_equal(trip.cpu().numpy(), exp_trip)
    assert np.array_equal(nodes_out.cpu().numpy(), exp_nodes if with_nodes else np.full(exp_nodes.size, SENT))
    return want, no


def test_the_graph_has_what_the_cases_need(K):
    ptrs, indices, order = K["ptrs"], K["indices"], K["order"]
    hub = indices[ptrs[HUB]:ptrs[HUB + 1]]
    assert hub.size >= 2049 and -(-hub.size // CHUNK) > 4
    chunk_of_first = {}
    across = [s for j, s in enumerate(hub.tolist()) if chunk_of_first.setdefault(s, j // CHUNK) != j // CHUNK]
    assert len(set(across)) == 300                                   # every hub source is seen again in a later chunk
    assert 150 in hub and 150 in indices[ptrs[1]:ptrs[2]]            # ... and reappears in another column
    deg = np.diff(ptrs)
    assert (deg[EMPTY0:EMPTY1] == 0).all() and EMPTY1 - EMPTY0 >= 70 and order[3:83].tolist() == list(range(EMPTY0, EMPTY1))
    col1 = indices[ptrs[1]:ptrs[2]].tolist()
    assert col1.count(1) == 2 and col1.count(150) == 2               # a self loop; parallel edges
    assert 0 in col1 and order[0] == 0                               # a source that is a frontier node
    out, rows, cols, _ = full_rule(ptrs, indices, order[:3])
    assert rows[(cols == 1)].tolist()[:3] == [1, 1, 0]               # its row points into the frontier prefix


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 513, 1025])
def test_frontier_sizes(K, n):
    want, no = run(K, [K["order"][:n]])
    assert not any(no) and want[0][0].size >= n


def test_frontier_with_repeats(K):
    nodes = np.array([1, HUB, 1, 2, HUB, 7, 7, 2], dtype=np.int64)
    want, no = run(K, [nodes], chunk_cap=64)
    assert not any(no) and want[0][1].size == 2 * 2600 + 2 * 6 + 2 * 4 + 2 * np.diff(K["ptrs"])[7]
    assert set(want[0][1][want[0][2] == 4].tolist()) <= set(range(8, 8 + 300)) | {0, 1, 3}     # rows: first positions only


def test_ids_out_of_range_raise_bit_1(K):
    nodes = np.array([1, N, -1, 2, 2 ** 40, HUB], dtype=np.int64)
    want, no = run(K, [nodes, K["order"][:5]])
    assert want[0][5] == 2 and want[1][5] == 0 and not any(no)


@pytest.mark.parametrize("short", [1, 0])
def test_node_cap_one_below_and_at_the_need(K, short):
    lists = [K["order"][3:9], K["order"][:90], K["order"][100:130]]
    needs = [need_of(K, l) for l in lists]
    assert needs[1] > max(needs[0], needs[2])
    want, no = run(K, lists, node_cap=needs[1] - short, chunk_cap=1000)
    assert no == [False, bool(short), False]                          # the neighbours of the refused batch are intact


@pytest.mark.parametrize("short", [1, 0])
def test_chunk_cap_one_below_and_at_the_need(K, short):
    lists = [K["order"][83:90], K["order"][:90], K["order"][100:110]]
    chunks = [rule(K, l)[4] for l in lists]
    assert chunks[1] > max(chunks[0], chunks[2]) and chunks[1] - short >= 1
    want, no = run(K, lists, node_cap=5000, chunk_cap=chunks[1] - short)
    assert no == [False, bool(short), False]


def test_ragged_lists_a_base_and_a_list_longer_than_max_nodes(K):
    order = K["order"]
    lists = [order[200:205], order[:40], np.zeros(0, np.int64), order[300:303]]
    want, no = run(K, lists, max_nodes=10, base=17)
    assert not any(no) and want[1][0][:10].tolist() == order[:10].tolist() and want[1][1].size == rule(K, order[:10])[1].size


@pytest.mark.parametrize("G", [1, 3, 300, 32773])
def test_batch_counts(K, G):
    order = K["order"]
    if G == 32773:                                                   # tiny frontiers: the rounds of 32 768
        kinds = [order[90 + j:90 + j + j % 3] for j in range(7)]
        lists = [kinds[b % 7] for b in range(G)]
    else:
        rs = np.random.default_rng(G)
        lists = [order[int(s):int(s) + int(k)] for s, k in zip(rs.integers(0, 1100, G), rs.integers(0, 21, G))]
    want, no = run(K, lists)
    assert not any(no)


def test_key_widths_and_shadows_agree(K):
    lists = [K["order"][:70], K["order"][500:520]]
    a, _ = run(K, lists, id_bound=N)
    b, _ = run(K, lists, id_bound=2 ** 31 + 1)                       # 64-bit keys
    c, _ = run(K, lists, id_bound=N, shadows=False)
    d, _ = run(K, lists, id_bound=2 ** 31 + 1, shadows=False)
    for other in (b, c, d):
        assert all(np.array_equal(x, y) for p, q in zip(a, other) for x, y in zip(p[:4], q[:4]))


def test_nodes_out_may_be_null(K):
    run(K, [K["order"][:70], K["order"][500:520]], with_nodes=False)


def test_against_the_induced_pair_over_out_nodes(K):
    cabi = K["cabi"]
    nodes = K["order"][:90]
    out, rows, cols, e = rule(K, nodes)[:4]
    run(K, [nodes])
    o = dict(dtype=torch.int64, device=DEV)
    ind = cabi.NsInduced(K["shadow"], torch.from_numpy(out).to(DEV).view(1, -1), torch.tensor([out.size], **o), 1, 1, N).count()
    m = int(ind.n_edges.cpu()[0])
    trip = torch.empty((3, m), **o)
    ind.emit(torch.zeros(1, **o), trip[0], trip[1], trip[2])
    trip = trip.cpu().numpy()
    assert int(ind.status.cpu()[0]) == 0
    mine = trip[:, trip[1] < nodes.size]                             # the induced triples whose column is a frontier position
    assert np.array_equal(mine, np.stack([rows, cols, e]))


@pytest.fixture(scope="module")
def seams():
    """columns 0 .. 3 of 1 024 * 512, 1 024 * 512 + 1, 16 * 512 and 16 * 512 + 1 entries, built on the device: the chunk
    prefix ends with a tile, has a second tile of one chunk of one entry, is one unit, is a unit and one chunk.  A column's
    last entry is a source that it names nowhere else: a new node in its last chunk"""
    from tch_geometric import _cabi
    n = 3000
    deg = [1024 * CHUNK, 1024 * CHUNK + 1, 16 * CHUNK, 16 * CHUNK + 1]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(13)
    di = torch.randint(4, n - 8, (sum(deg),), device=DEV, generator=gen)
    dp = torch.full((n + 1,), sum(deg), dtype=torch.int64, device=DEV)
    dp[:5] = torch.tensor([0] + np.cumsum(deg).tolist(), device=DEV)
    di[dp[1:5] - 1] = torch.arange(n - 4, n, device=DEV)
    plain = _cabi.graph_view(dp, di)
    shadow = _cabi.graph_view(dp, di, indices32=di.to(torch.int32), ptrs32=dp.to(torch.int32))
    return dict(cabi=_cabi, ptrs=dp.cpu().numpy(), indices=di.cpu().numpy(), plain=plain, shadow=shadow, cache={}, keep=(dp, di))


@pytest.mark.parametrize("shadows", [True, False])
def test_columns_at_the_tile_and_unit_seams(seams, shadows):
    n = seams["ptrs"].size - 1
    lists = [np.array([v], dtype=np.int64) for v in range(4)]
    want, no = run(seams, lists, id_bound=n, shadows=shadows)
    assert not any(no) and [w[4] for w in want] == [1024, 1025, 16, 17]
    for v, w in enumerate(want):
        assert w[0][-1] == n - 4 + v and w[1][-1] == w[0].size - 1           # the last entry's source is the last new node
    want, no = run(seams, [np.array([3, 1, 2], dtype=np.int64)], id_bound=n, shadows=shadows)   # 17 + 1 025 + 16 chunks
    assert not any(no) and want[0][4] == 17 + 1025 + 16
