"""Per-group node dedup (tg_ns_homo_unique_grouped, PyG's disjoint=True), host-only parts: the NumPy statement of the rule
(helpers_disjoint) against a brute-force dict version and against the plain dedup's statement, the link loaders' group
maps, the exports, the form and workspace queries, the argument checks that run before anything is launched, and
transforms.unique_nodes(seed_group=...) on CPU tensors.  No GPU: every device pointer handed over is null (the workspace
of the short-workspace case is a host buffer that is never read)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers_disjoint import BINARY, TRIPLET, brute_force, disjoint_rule, link_groups, roots
from helpers_unique import unique_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024                                        # a gfx950 workgroup's LDS
NAMES = ("tg_ns_homo_unique_grouped_form", "tg_ns_homo_unique_grouped_workspace_bytes", "tg_ns_homo_unique_grouped")


def random_forest(rs, n_seeds, fanouts, id_bound):
    """A forest as the sampler lays it out: hop h gives every position of hop h - 1 (the seeds for h = 0) up to fanouts[h]
    children; edge e makes position n_seeds + e.  -> (samples, rows, cols, layer_starts)."""
    cols, starts, prev = [], [], list(range(n_seeds))
    for k in fanouts:
        starts.append(n_seeds + len(cols))
        cur = []
        for p in prev:
            for _ in range(int(rs.integers(0, k + 1))):
                cur.append(n_seeds + len(cols))
                cols.append(p)
        prev = cur
    cols = np.array(cols, dtype=np.int64)
    n = n_seeds + cols.size
    return rs.integers(0, id_bound, n), n_seeds + np.arange(cols.size), cols, starts


def same(a, b):
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y), (x, y)
    assert list(a[5]) == list(b[5])


def test_rule_agrees_with_brute_force_on_random_forests():
    rs = np.random.default_rng(11)
    merged = 0
    for trial in range(300):
        n_seeds = int(rs.integers(1, 7))
        fanouts = [int(rs.integers(1, 4)) for _ in range(int(rs.integers(0, 4)))]
        s, rows, cols, starts = random_forest(rs, n_seeds, fanouts, int(rs.integers(2, 12)))
        n_groups = int(rs.integers(1, n_seeds + 1))
        sg = None if trial % 3 == 0 else rs.integers(0, n_groups, n_seeds)
        got = disjoint_rule(s, rows, cols, n_seeds, sg, starts)
        same(got, brute_force(s, rows, cols, n_seeds, sg, starts))
        nodes, group, inverse = got[:3]
        assert len(set(zip(group.tolist(), nodes.tolist()))) == nodes.size       # pairs are distinct
        assert np.array_equal(nodes[inverse], s)
        assert np.array_equal(group[got[3]], group[got[4]])                      # both ends of an edge share the group
        merged += nodes.size < s.size
    assert merged > 100


def test_one_group_is_the_plain_dedup():
    rs = np.random.default_rng(12)
    for _ in range(50):
        n_seeds = int(rs.integers(1, 9))
        s, rows, cols, starts = random_forest(rs, n_seeds, [3, 2], 15)
        nodes, group, inverse, rows_u, cols_u, layers = disjoint_rule(s, rows, cols, n_seeds, np.zeros(n_seeds, np.int64), starts)
        plain = unique_rule(s, rows, cols, starts)
        for got, want in zip((nodes, inverse, rows_u, cols_u), plain[:4]):
            assert np.array_equal(got, want)
        assert layers == plain[4] and group.size == nodes.size and (group == 0).all()


def test_identity_map_keeps_a_node_apart_under_two_roots():
    # seeds 5, 5; each has the child 9; seed 0 also has the grandchild 5 (its own id again: merged inside the group)
    s = np.array([5, 5, 9, 9, 5])
    cols = np.array([0, 1, 2])
    rows = 2 + np.arange(3)
    assert roots(cols, 5, 2).tolist() == [0, 1, 0, 1, 0]
    nodes, group, inverse, rows_u, cols_u, layers = disjoint_rule(s, rows, cols, 2, None, [2, 4])
    assert nodes.tolist() == [5, 5, 9, 9] and group.tolist() == [0, 1, 0, 1]
    assert inverse.tolist() == [0, 1, 2, 3, 0] and layers == [2, 4]
    assert rows_u.tolist() == [2, 3, 0] and cols_u.tolist() == [0, 1, 2]
    one = disjoint_rule(s, rows, cols, 2, [0, 0], [2, 4])                     # one group: src_j == dst_j merge
    assert one[0].tolist() == [5, 9] and one[1].tolist() == [0, 0] and one[5] == [1, 2]


@pytest.mark.parametrize("E,K", [(1, 0), (5, 0), (4, 2), (3, 3)])
def test_link_group_maps(E, K):
    P = E + E * K
    sg, ti, ng = link_groups(E, K, BINARY)
    assert sg.size == ti.size == 2 * P and ng == P and sorted(set(sg.tolist())) == list(range(P))
    for j in range(P):
        assert sg[j] == sg[P + j] == j and ti[j] == ti[P + j] == (j if j < E else (j - E) // K)   # src_j and dst_j together
    sg, ti, ng = link_groups(E, K, TRIPLET)
    assert sg.size == 2 * E + E * K and ng == E and np.array_equal(sg, ti)
    for i in range(E):
        assert sg[i] == sg[E + i] == i
        assert (sg[2 * E + i * K:2 * E + (i + 1) * K] == i).all()


# ---- the C ABI without a device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


def test_symbols_exported_and_declared(cabi):
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    declared = set(re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", header))
    for name in NAMES:
        assert name in cabi.EXPORTS and name in declared and hasattr(cabi.lib, name)
    assert "tg_ns_unique_grouped_out" in header
    assert [f for f, _ in cabi.TgNsUniqueGroupedOut._fields_] == ["nodes", "inverse", "rows", "cols", "counts", "layer_nodes",
                                                                  "group"]


def test_form_and_workspace_against_the_plain_operator(cabi):
    """The pair key picks the key width; the LDS form holds one more u16 per position and needs n_groups <= 65 536; a
    batch's workspace holds one more u32 per position (rounded to 256 bytes).  The plain operator's sizes are what they were."""
    for cap, id_bound, n_groups in ((124, 34, 4), (3072, 1 << 16, 64), (12288, 1 << 24, 1), (169984, 1 << 24, 1024)):
        plain_form, plain_lds, _ = cabi.ns_homo_unique_form(cap, id_bound * n_groups, LDS)
        form, lds = cabi.ns_homo_unique_grouped_form(cap, id_bound, n_groups, LDS)
        assert lds == plain_lds + ((2 * cap + 15) & ~15)
        assert form == (1 if cap <= 32768 and lds <= LDS else 2) and (form == 2 or plain_form == 1)
        _, plain_min = cabi.ns_homo_unique_workspace_bytes(cap, id_bound * n_groups, 16)
        total, least = cabi.ns_homo_unique_grouped_workspace_bytes(cap, id_bound, n_groups, 16)
        assert least == plain_min + ((4 * cap + 255) & ~255)
        assert total in (0, 16 * least) and (cap <= 12288 or total == 16 * least)
    # 32-bit keys up to n_groups * id_bound = 2^31, 64-bit ones above: 4 more bytes per slot
    k32 = cabi.ns_homo_unique_grouped_form(3072, 1 << 28, 8, LDS)[1]
    k64 = cabi.ns_homo_unique_grouped_form(3072, 1 << 31, 8, LDS)[1]
    assert k64 - k32 == 4096 * 4
    assert cabi.ns_homo_unique_grouped_form(1024, 1 << 10, 65536, LDS)[0] == 1
    assert cabi.ns_homo_unique_grouped_form(1024, 1 << 10, 65537, LDS)[0] == 2      # a group no longer fits a u16 word
    with pytest.raises(cabi.TchGeoError, match="2\\^63"):
        cabi.ns_homo_unique_grouped_form(1024, 1 << 62, 2, LDS)
    assert cabi.ns_homo_unique_grouped_form(1024, (1 << 62) - 1, 2, LDS)[0] == 1    # 2^63 - 2: the largest pair bound
    with pytest.raises(cabi.TchGeoError, match="n_groups"):
        cabi.ns_homo_unique_grouped_form(1024, 1 << 20, 0, LDS)
    with pytest.raises(cabi.TchGeoError, match="n_groups"):
        cabi.ns_homo_unique_grouped_workspace_bytes(1024, 1 << 20, -3, 4)
    with pytest.raises(cabi.TchGeoError, match="n_batches"):
        cabi.ns_homo_unique_grouped_workspace_bytes(1024, 1 << 20, 4, -1)


def _call(cabi, src=True, dst=True, n_batches=4, n_seeds=4, n_hops=2, id_bound=1 << 20, cap_nodes=124, cap_edges=120,
          ws=None, ws_bytes=0, form=2, n_groups=4, seed_group=None):
    so, uo = cabi.TgNsOut(), cabi.TgNsUniqueGroupedOut()
    so.cap_nodes, so.cap_edges = cap_nodes, cap_edges
    rc = cabi.lib.tg_ns_homo_unique_grouped(C.byref(so) if src else None, C.c_int64(n_batches), C.c_int64(n_seeds),
                                            C.c_int32(n_hops), C.c_int64(id_bound), seed_group, C.c_int64(n_groups),
                                            C.byref(uo) if dst else None, ws, C.c_int64(ws_bytes), C.c_int32(form), None)
    return rc, cabi.lib.tg_last_error().decode()


def _refused(cabi, word, **kw):
    rc, msg = _call(cabi, **kw)
    assert rc == 1, (rc, msg)                                                 # TG_ERR_INVALID
    assert "tg_ns_homo_unique_grouped" in msg and word in msg, msg


def test_refusals_before_any_launch(cabi):
    """Every bad argument returns TG_ERR_INVALID with a message that names it; the slab pointers are all null, so nothing
    can have been launched."""
    least = cabi.ns_homo_unique_grouped_workspace_bytes(124, 1 << 20, 4, 4)[1]
    buf = C.create_string_buffer(least + 16)                                  # stands in for a workspace; never read
    ws = C.c_void_p((C.addressof(buf) + 7) & ~7)
    odd = C.c_void_p(ws.value + 4)
    sg = C.c_void_p(C.addressof(buf))                                         # stands in for a map; never read
    ok = dict(ws=ws, ws_bytes=least)
    _refused(cabi, "null", src=False, **ok)
    _refused(cabi, "null", dst=False, **ok)
    _refused(cabi, "n_batches", n_batches=-1, **ok)
    _refused(cabi, "n_seeds", n_seeds=-4, seed_group=sg, **ok)
    _refused(cabi, "n_hops", n_hops=-1, **ok)
    _refused(cabi, "n_hops", n_hops=9, **ok)
    _refused(cabi, "cap_nodes", cap_nodes=-5, **ok)
    _refused(cabi, "cap_edges", cap_edges=-5, **ok)
    _refused(cabi, "id_bound", id_bound=0, **ok)
    _refused(cabi, "n_groups", n_groups=0, seed_group=sg, **ok)
    _refused(cabi, "n_groups", n_groups=-1, **ok)
    _refused(cabi, "without a seed_group", n_groups=3, **ok)                  # the identity has n_seeds groups
    _refused(cabi, "without a seed_group", n_groups=5, **ok)
    _refused(cabi, "2^63", id_bound=1 << 61, n_groups=4, **ok)
    _refused(cabi, "workspace_bytes", ws=ws, ws_bytes=-1)
    _refused(cabi, "workspace too small", ws=ws, ws_bytes=least - 1)          # below bytes_min
    _refused(cabi, "workspace too small", ws=None, ws_bytes=1 << 30)          # a size without a workspace
    _refused(cabi, "aligned", ws=odd, ws_bytes=least)
    _refused(cabi, "form", form=3, **ok)
    _refused(cabi, "form", form=-1, **ok)
    _refused(cabi, "does not fit", form=1, cap_nodes=200000)                  # past any workgroup's LDS
    # well-formed sizes and a large enough workspace: the null slabs are refused, still before any launch
    _refused(cabi, "null", **ok)
    _refused(cabi, "null", n_groups=2, seed_group=sg, **ok)
    assert _call(cabi, n_batches=0, **ok)[0] == 0                             # nothing to do
    # the plain operator's bytes_min is what it was: the group word is the grouped call's alone
    assert least > cabi.ns_homo_unique_workspace_bytes(124, 1 << 22, 4)[1]


@pytest.mark.parametrize("case", ["identity", "two groups", "one group", "no hops", "empty"])
def test_unique_nodes_with_seed_group_on_cpu_tensors(cabi, case):
    from tch_geometric.transforms import unique_nodes
    rs = np.random.default_rng(5)
    n_seeds = 0 if case == "empty" else 6
    s, rows, cols, _ = random_forest(rs, n_seeds, [] if case in ("no hops", "empty") else [3, 2, 2], 9)
    sg = {"identity": np.arange(6), "two groups": np.array([0, 1, 1, 0, 1, 0]), "one group": np.zeros(6, np.int64),
          "no hops": np.array([2, 0, 2, 0, 1, 1]), "empty": np.zeros(0, np.int64)}[case]
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64))
    got = unique_nodes(t(s), t(rows), t(cols), seed_group=t(sg))
    nodes, group, inverse, rows_u, cols_u, _ = disjoint_rule(s, rows, cols, n_seeds, sg)
    assert len(got) == 5
    for g, w in zip(got, (nodes, rows_u, cols_u, inverse, group)):
        assert g.dtype == torch.int64 and np.array_equal(g.numpy(), w)
    if case == "one group":                                                  # and the five-tuple's head is the plain call's
        for g, w in zip(got[:4], unique_nodes(t(s), t(rows), t(cols))):
            assert torch.equal(g, w)
    with pytest.raises(ValueError):
        unique_nodes(t(s), t(rows), t(cols), seed_group=t(sg), n_seeds=n_seeds + 1)
    assert len(unique_nodes(t(s), t(rows), t(cols))) == 4                     # without the map: as before


# ---- the loaders' refusals: raised before any device work, so they need no device -----------------------------------------
def _graph():
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=5, time=torch.arange(6))


@pytest.mark.parametrize("kw,word", [
    (dict(disjoint=True), "unique=True"),                                                            # nothing to keep apart
    (dict(unique=True, induced=True, disjoint=True), "out of scope"),
    (dict(unique=True, induced=True, disjoint=True, time_attr="time", input_time=torch.zeros(5, dtype=torch.int64)), "out of scope"),
    (dict(unique=True, time_attr="time", input_time=torch.zeros(5, dtype=torch.int64)), "needs disjoint=True"),
])
def test_neighbor_loader_refusals_need_no_device(cabi, kw, word):
    from tch_geometric.loader import NeighborLoader
    with pytest.raises(ValueError, match=word):
        NeighborLoader(_graph(), [2, 2], device="cuda:0", **kw)


@pytest.mark.parametrize("kw,word", [
    (dict(edge_label_time=torch.zeros(6, dtype=torch.int64)), "come together"),                      # no time_attr
    (dict(time_attr="time"), "come together"),                                                       # no edge_label_time
    (dict(time_attr="time", edge_label_time=torch.zeros(6, dtype=torch.int32)), "edge_label_time"),  # int64 only
    (dict(time_attr="time", edge_label_time=torch.zeros(5, dtype=torch.int64)), "edge_label_time"),  # one per label edge
    (dict(time_attr="time", edge_label_time=[0] * 6), "edge_label_time"),                            # a tensor
    (dict(disjoint=True), "unique=True"),
])
def test_link_loader_refusals_need_no_device(cabi, kw, word):
    from tch_geometric.loader import LinkNeighborLoader
    with pytest.raises(ValueError, match=word):
        LinkNeighborLoader(_graph(), [2], device="cuda:0", **kw)
