"""GraphSAINT's random-walk sampler (tg_saint_rw_nodes, tg_saint_coverage_add, tg_saint_norm, GraphSAINTRandomWalkLoader),
host-only parts: the NumPy restatement against brute-force dict versions, the exports, the arithmetic of the capacity /
form / workspace queries around the largest LDS table, every refusal that comes before a launch and the loader's argument
refusals.  No GPU: every device pointer handed over is null or an address that is never read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers_saint import coverage_counts, node_list, norms, presample_launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_saint_rw_capacity", "tg_saint_rw_form", "tg_saint_rw_workspace_bytes", "tg_saint_rw_nodes",
         "tg_saint_coverage_add", "tg_saint_norm")
LDS = 160 * 1024


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


# ---- the restatement against brute force -------------------------------------------------------------------------------
def brute_node_list(walks, skip=()):
    """position by position with a dict: the definition"""
    B, L = len(walks), len(walks[0])
    first = {}
    for l in range(L):
        for i in range(B):
            v = int(walks[i][l])
            if i in skip or v < 0:
                continue
            first.setdefault(v, l * B + i)
    return [v for v, _ in sorted(first.items(), key=lambda kv: kv[1])]


def random_walks(rs, B, T, n):
    """a walk matrix as tg_random_walk writes it: -1 from a walker's dead end on"""
    walks = rs.integers(0, n, (B, T + 1)).astype(np.int64)
    stop = rs.integers(1, 2 * (T + 1), B)                  # about half of the walkers stop early
    for i in range(B):
        walks[i, stop[i]:] = -1
    return walks


@pytest.mark.parametrize("seed", range(8))
def test_node_list_equals_brute_force(seed):
    rs = np.random.default_rng(seed)
    B, T, n = int(rs.integers(1, 12)), int(rs.integers(1, 5)), int(rs.integers(2, 15))
    walks = random_walks(rs, B, T, n)
    assert node_list(walks).tolist() == brute_node_list(walks)
    skip = [int(i) for i in rs.permutation(B)[:B // 3]]
    assert node_list(walks, skip=skip).tolist() == brute_node_list(walks, set(skip))
    roots = [int(v) for v in dict.fromkeys(walks[:, 0].tolist())]
    assert node_list(walks).tolist()[:len(roots)] == roots             # step-major: the distinct roots lead


@pytest.mark.parametrize("seed", range(4))
def test_coverage_counts_equal_brute_force(seed):
    rs = np.random.default_rng(100 + seed)
    N, E = 9, 14
    node_lists = [rs.integers(-1, N + 1, rs.integers(0, 12)) for _ in range(5)]       # with ids outside the tables
    edge_lists = [rs.integers(-1, E + 1, rs.integers(0, 20)) for _ in range(3)]
    nc, ec = coverage_counts(node_lists, edge_lists, N, E)
    want_n, want_e = [0] * N, [0] * E
    for ids in node_lists:
        for v in ids.tolist():
            if 0 <= v < N:
                want_n[v] += 1
    for ids in edge_lists:
        for e in ids.tolist():
            if 0 <= e < E:
                want_e[e] += 1
    assert nc.tolist() == want_n and ec.tolist() == want_e


def brute_norms(ptrs, nc, ec, n_samples):
    f32 = np.float32
    n = len(ptrs) - 1
    node_norm, edge_norm = [], []
    for v in range(n):
        d = f32(0.1) if nc[v] == 0 else f32(nc[v])
        node_norm.append(f32(f32(f32(n_samples) / d) / f32(n)))
    for c in range(n):
        for e in range(ptrs[c], ptrs[c + 1]):
            if nc[c] == 0 and ec[e] == 0:
                edge_norm.append(f32(0.1))
            elif ec[e] == 0:
                edge_norm.append(f32(1e4))
            else:
                edge_norm.append(min(max(f32(f32(nc[c]) / f32(ec[e])), f32(0)), f32(1e4)))
    return np.array(node_norm, dtype=f32), np.array(edge_norm, dtype=f32)


@pytest.mark.parametrize("seed", range(4))
def test_norms_equal_brute_force(seed):
    rs = np.random.default_rng(200 + seed)
    n = 11
    deg = rs.integers(0, 5, n)
    deg[0], deg[1], deg[3] = 2, 1, 0                        # column 3 is empty
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nc = rs.integers(0, 4, n).astype(np.int64) * rs.integers(0, 30000, n)
    ec = rs.integers(0, 3, ptrs[-1]).astype(np.int64)       # zeros (x/0, 0/0) and ratios above 1e4
    nc[0], nc[1], ec[:3] = 0, 5, (0, 1, 0)                  # 0/0, 0/1 and 5/0 whatever the draws
    got = norms(ptrs, nc, ec, 37)
    want = brute_norms(ptrs.tolist(), nc.tolist(), ec.tolist(), 37)
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[1] == np.float32(0.1)).any() and (got[1] == np.float32(1e4)).any()


def test_stopping_rule():
    assert presample_launches([10, 10, 10, 10], 6, 5) == 3                # 30 >= 30 at the third launch
    assert presample_launches([10, 10, 10, 10], 6, 4) == 3                # 20 < 24
    assert presample_launches([100], 6, 5) == 1
    with pytest.raises(ValueError):
        presample_launches([1, 1], 6, 5)


# ---- exports and the queries' arithmetic -------------------------------------------------------------------------------------
def test_symbols_and_struct(cabi):
    for name in NAMES:
        assert name in cabi.EXPORTS and hasattr(cabi.lib, name)
    assert [f for f, _ in cabi.TgSaintRwOut._fields_] == ["nodes", "pitch_nodes", "counts", "counts_stride"]
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    for name in NAMES:
        assert "TG_API int %s(" % name in header


def r256(x):
    return (x + 255) & ~255


def test_capacity_form_and_workspace_arithmetic(cabi):
    """P = 12 288 is the largest LDS table of 160 KiB (16 384 slots of 8 bytes + 2 bytes per position + 256 static bytes);
    one position more doubles the table and takes the flat form.  Nothing here touches a device."""
    assert cabi.saint_rw_capacity(3072, 3) == 12288 and cabi.saint_rw_capacity(3073, 3) == 12292
    assert cabi.saint_rw_capacity(12289, 1) == 2 * 12289 and cabi.saint_rw_capacity(0, 5) == 0
    assert cabi.saint_rw_form(3072, 3, LDS) == (1, 16384 * 8 + 2 * 12288 + 256)
    assert cabi.saint_rw_form(6144, 1, LDS) == (1, 16384 * 8 + 2 * 12288 + 256)
    assert cabi.saint_rw_capacity(1, 12288) == 12289                    # P = 12 289: one root, 12 288 steps
    form, lds = cabi.saint_rw_form(1, 12288, LDS)                        # 4P/3 = 16 385.3 -> 32 768 slots
    assert form == 2 and lds == 32768 * 8 + ((2 * 12289 + 15) & ~15) + 256
    form, lds = cabi.saint_rw_form(12289, 1, LDS)                        # P = 24 578: 4P/3 = 32 770.7 -> 65 536 slots
    assert form == 2 and lds == 65536 * 8 + ((2 * 24578 + 15) & ~15) + 256
    form, lds = cabi.saint_rw_form(3073, 3, LDS)                         # P = 12 292: the first B * 4 above 12 288
    assert form == 2 and lds == 32768 * 8 + ((2 * 12292 + 15) & ~15) + 256
    assert cabi.saint_rw_form(3072, 3, 16384 * 8 + 2 * 12288 + 255)[0] == 2      # one byte short
    assert cabi.saint_rw_form(1, 1, 1024) == (1, 64 * 8 + 16 + 256)      # the smallest table has 64 slots
    for B, T in ((3072, 3), (1, 12288), (3073, 3), (63, 1)):
        P = B * (T + 1)
        cap = 64
        while cap < (4 * P + 2) // 3:
            cap *= 2
        per = r256(cap * 4) + r256(cap * 4) + r256(P * 4) + r256(((P + 1023) // 1024) * 4) + r256(P * 4)
        assert cabi.saint_rw_workspace_bytes(5, B, T, form=2) == (5 * per, per)
        assert cabi.saint_rw_workspace_bytes(5, B, T, form=1) == (0, per)
        assert cabi.saint_rw_workspace_bytes(0, B, T, form=2) == (0, per)


def test_the_plan_is_the_dedup_operators(cabi):
    """tg_saint_rw_form sizes its table as tg_ns_homo_unique_form does for as many positions under 32-bit keys"""
    assert cabi.ns_homo_unique_form(12288, 1 << 20, LDS)[:2] == cabi.saint_rw_form(3072, 3, LDS)
    assert cabi.ns_homo_unique_form(12289, 1 << 20, LDS)[:2] == cabi.saint_rw_form(1, 12288, LDS)
    assert cabi.ns_homo_unique_form(12292, 1 << 20, LDS)[:2] == cabi.saint_rw_form(3073, 3, LDS)


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a non-null address that is never read: every call below is refused before anything is launched


def call_nodes(cabi, n_major=100, roots=FAKE, G=2, B=4, T=2, rng=True, nodes=FAKE, pitch=None, counts=FAKE, stride=1,
               status=FAKE, ws=None, ws_bytes=0, form=2, csr=True, ptrs=FAKE):
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, FAKE, n_major, 10
    out = cabi.TgSaintRwOut(nodes, B * (T + 1) if pitch is None else pitch, counts, stride)
    r = cabi.TgRng(1, 2)
    return cabi.lib.tg_saint_rw_nodes(C.byref(g) if csr else None, C.c_void_p(roots), C.c_int64(G), C.c_int64(B), C.c_int64(T),
                                      C.byref(r) if rng else None, C.byref(out), C.c_void_p(status), C.c_void_p(ws),
                                      C.c_int64(ws_bytes), C.c_int32(form), None)


@pytest.mark.parametrize("kw, word", [
    (dict(csr=False), "null argument"),
    (dict(rng=False), "null argument"),
    (dict(ptrs=None), "null graph"),
    (dict(roots=None), "null roots"),
    (dict(nodes=None), "null roots"),
    (dict(counts=None), "null roots"),
    (dict(status=None), "null roots"),
    (dict(T=0), "walk_length"),
    (dict(B=-1), "batch_size"),
    (dict(pitch=11), "pitch_nodes"),
    (dict(stride=0), "counts_stride"),
    (dict(form=3), "unknown form"),
    (dict(G=-1), "n_batches"),
    (dict(B=3073, T=3, form=1), "does not fit"),
    (dict(ws=None, ws_bytes=0), "workspace too small"),
    (dict(ws=FAKE, ws_bytes=100), "workspace too small"),
    (dict(ws=FAKE + 4, ws_bytes=1 << 30), "8-byte aligned"),
    (dict(B=1 << 29, T=2), "above 2\\^30"),
])
def test_rw_nodes_refusals(cabi, kw, word):
    import re
    assert call_nodes(cabi, **kw) == 1                                   # TG_ERR_INVALID
    assert re.search(word, cabi.lib.tg_last_error().decode()), cabi.lib.tg_last_error()


def test_rw_nodes_graph_limit_and_empty_launches(cabi):
    assert call_nodes(cabi, n_major=(1 << 31) + 1, ws=FAKE, ws_bytes=1 << 30) == 3       # TG_ERR_UNSUPPORTED
    assert b"32-bit hash keys" in cabi.lib.tg_last_error()
    assert call_nodes(cabi, G=0, ws=FAKE, ws_bytes=1 << 30) == 0                          # nothing to launch
    assert call_nodes(cabi, B=0, ws=FAKE, ws_bytes=1 << 30) == 0
    assert call_nodes(cabi, G=0, form=0) == 0 and call_nodes(cabi, G=0, form=1) == 0    # before any question to a device
    assert call_nodes(cabi, G=0, form=2) == 1                                             # the flat form's workspace is still checked


def test_query_refusals(cabi):
    lib = cabi.lib
    x, y, f = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    assert lib.tg_saint_rw_capacity(C.c_int64(4), C.c_int64(0), C.byref(x)) == 1
    assert lib.tg_saint_rw_capacity(C.c_int64(-1), C.c_int64(2), C.byref(x)) == 1
    assert lib.tg_saint_rw_capacity(C.c_int64(4), C.c_int64(2), None) == 1
    assert lib.tg_saint_rw_capacity(C.c_int64(1 << 30), C.c_int64(1), C.byref(x)) == 1
    assert lib.tg_saint_rw_form(C.c_int64(4), C.c_int64(2), C.c_int64(LDS), None, C.byref(x)) == 1
    assert lib.tg_saint_rw_form(C.c_int64(4), C.c_int64(0), C.c_int64(LDS), C.byref(f), C.byref(x)) == 1
    assert lib.tg_saint_rw_workspace_bytes(C.c_int64(-1), C.c_int64(4), C.c_int64(2), C.c_int32(2), C.byref(x), C.byref(y)) == 1
    assert lib.tg_saint_rw_workspace_bytes(C.c_int64(1), C.c_int64(4), C.c_int64(2), C.c_int32(5), C.byref(x), C.byref(y)) == 1
    assert lib.tg_saint_rw_workspace_bytes(C.c_int64(1), C.c_int64(4), C.c_int64(2), C.c_int32(2), None, C.byref(y)) == 1
    # 2^31 - 1 mini-batches of 2^30 positions: the byte count does not fit int64
    assert lib.tg_saint_rw_workspace_bytes(C.c_int64(0x7fffffff), C.c_int64(1 << 28), C.c_int64(3), C.c_int32(2), C.byref(x),
                                           C.byref(y)) == 1
    assert b"overflow" in lib.tg_last_error()


def test_coverage_and_norm_refusals(cabi):
    lib = cabi.lib
    p, i64 = C.c_void_p, C.c_int64
    add = lambda nodes=FAKE, pitch=4, counts=FAKE, stride=1, G=1, ids=FAKE, n_ids=1, nc=FAKE, N=5, ec=FAKE, E=5, st=FAKE: \
        lib.tg_saint_coverage_add(p(nodes), i64(pitch), p(counts), i64(stride), i64(G), p(ids), i64(n_ids), p(nc), i64(N),
                                  p(ec), i64(E), p(st), None)
    for kw in (dict(nodes=None), dict(counts=None), dict(stride=0), dict(G=-1), dict(ids=None), dict(n_ids=-1),
               dict(nc=None), dict(ec=None), dict(st=None), dict(N=-1), dict(pitch=-1)):
        assert add(**kw) == 1, kw
    assert add(G=0, n_ids=0) == 0                                        # nothing to add, nothing launched
    g = cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = FAKE, FAKE, 5, 7
    norm = lambda graph=g, nc=FAKE, ec=FAKE, n=3, nn=FAKE, en=FAKE: \
        lib.tg_saint_norm(C.byref(graph) if graph is not None else None, p(nc), p(ec), i64(n), p(nn), p(en), None)
    for kw in (dict(graph=None), dict(nc=None), dict(ec=None), dict(n=-1), dict(nn=None), dict(en=None)):
        assert norm(**kw) == 1, kw
    g0 = cabi.TgGraph()
    g0.n_major = 5
    assert norm(graph=g0) == 1                                           # null ptrs


# ---- the loader's refusals ---------------------------------------------------------------------------------------------------------
def _graph(**attrs):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=5, **attrs)


@pytest.mark.parametrize("args, kw, word", [
    ((0, 2, 3), {}, "batch_size"),
    ((4, 0, 3), {}, "walk_length"),
    ((4, 2, 0), {}, "num_steps"),
    ((4, 2, 3), dict(sample_coverage=-1), "sample_coverage"),
    ((4, 2, 3), dict(prefetch=0), "prefetch"),
    ((4, 2, 3), dict(form=3), "form"),
    ((1 << 29, 2, 3), {}, "2\\^30"),
    ((4, 2, 3), dict(call_id0=-1), "call_id0"),
    ((4, 2, 3), dict(call_id0=1 << 62), "call_id0"),
])
def test_loader_refusals_need_no_device(cabi, args, kw, word):
    from tch_geometric.loader import GraphSAINTRandomWalkLoader
    with pytest.raises(ValueError, match=word):
        GraphSAINTRandomWalkLoader(_graph(), *args, device="cuda:0", **kw)


@pytest.mark.parametrize("name, n", [("node_norm", 5), ("edge_norm", 6)])
def test_loader_refuses_data_that_hides_its_norms(cabi, name, n):
    import tch_geometric
    assert tch_geometric.GraphSAINTRandomWalkLoader is tch_geometric.loader.GraphSAINTRandomWalkLoader
    with pytest.raises(ValueError, match=name):
        tch_geometric.GraphSAINTRandomWalkLoader(_graph(**{name: torch.zeros(n)}), 4, 2, 3, sample_coverage=1, device="cuda:0")
