"""Per-type node dedup of the typed slabs (tg_ns_typed_unique), host-only parts: the exports, the form query with a
stated LDS limit, the workspace sizes, the argument checks that run before anything is launched, and
transforms.unique_nodes_hetero on CPU tensors against the NumPy statement of the rule applied per type.  No GPU: every
device pointer handed over is null (the workspace of the refusals is a host buffer that is never read)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers_unique import unique_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024                                        # a gfx950 workgroup's LDS
NAMES = ("tg_ns_typed_unique_form", "tg_ns_typed_unique_workspace_bytes", "tg_ns_typed_unique")


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


def slots_of(pitch):
    slots = 64
    while slots < (4 * pitch + 2) // 3:
        slots *= 2
    return slots


def test_symbols_exported_and_declared(cabi):
    header = open(os.path.join(ROOT, "include", "tchgeo.h")).read()
    declared = set(re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", header))
    for name in NAMES:
        assert name in cabi.EXPORTS and name in declared and hasattr(cabi.lib, name)
    assert "tg_ns_typed_in" in header and "tg_ns_typed_unique_out" in header
    assert [f for f, _ in cabi.TgNsTypedUniqueOut._fields_] == ["nodes", "inverse", "rows", "cols", "counts", "seed_counts"]
    assert [f for f, _ in cabi.TgNsTypedIn._fields_] == ["n_types", "n_rels", "rel_src", "rel_dst", "samples", "pitch_nodes",
                                                         "rows", "cols", "pitch_edges", "counts", "counts_stride",
                                                         "n_inputs", "id_bound"]


def test_form_query_with_a_stated_lds_limit(cabi):
    """The LDS form needs the largest type's table (2^k >= 4/3 pitch slots of key + u32) plus a u16 word per position of
    every type: 3 small types fit, raising one pitch flips the form exactly where lds_bytes passes the limit."""
    ask = lambda pitches, bounds=(1 << 20,) * 3: cabi.ns_typed_unique_form(list(pitches), list(bounds), LDS)
    form, lds = ask((124, 300, 77))
    assert form == 1 and slots_of(300) * 8 + 2 * (124 + 300 + 77) <= lds <= slots_of(300) * 8 + 2 * (124 + 300 + 77) + 512
    # raise the middle pitch: the form is 1 exactly while lds_bytes fits, and lds_bytes never shrinks
    prev, flipped = lds, None
    for pitch in sorted(set(list(range(300, 40000, 997)) + [12288, 12289, 32768, 32769])):
        form, lds = ask((124, pitch, 77))
        assert lds >= prev, pitch
        assert form == (1 if lds <= LDS and pitch <= 32768 else 2), (pitch, lds)
        if form == 2 and flipped is None:
            flipped = pitch
        assert flipped is None or form == 2                                   # once flat, flat from there on
        prev = lds
    assert flipped is not None and 6144 < flipped <= 12288 + 997              # 16 384 slots x 8 B = 128 KiB still fits
    assert ask((124, 12288, 77))[0] == 1 and ask((124, 12289, 77))[0] == 2    # the next table is 32 768 slots: 256 KiB
    # monotone in every pitch, not only the largest
    base = ask((1000, 2000, 3000))[1]
    for t in range(3):
        for more in (1, 8, 500, 5000):
            p = [1000, 2000, 3000]
            p[t] += more
            assert ask(p)[1] >= base, (t, more)
    assert ask((1000, 2000, 3008))[1] > base and ask((1008, 2000, 3000))[1] > base
    # the u16 words of the OTHER types count: a table that fits alone is pushed out by them
    assert ask((12288, 0, 0))[0] == 1 and ask((12288, 12288, 12288))[0] == 2
    # a 64-bit id_bound on the largest type: 12 bytes per slot instead of 8
    wide = ask((1000, 2000, 3000), (1 << 20, 1 << 20, 1 << 40))[1]
    assert wide == base + slots_of(3000) * 4
    assert ask((1000, 2000, 3000), (1 << 20, 1 << 20, 1 << 31))[1] == base     # [0, 2^31) still fits 32-bit keys
    assert ask((1000, 2000, 3000), (1 << 40, 1 << 20, 1 << 20))[1] == base     # 2 048 x 12 B stays below 4 096 x 8 B
    assert ask((124, 12288, 77), (1 << 20, 1 << 40, 1 << 20))[0] == 2          # 16 384 x 12 B = 192 KiB
    # a limit of its own: a device with 64 KiB
    assert cabi.ns_typed_unique_form([3072, 100], [1 << 20] * 2, 64 * 1024)[0] == 1
    assert cabi.ns_typed_unique_form([3073, 100], [1 << 20] * 2, 64 * 1024)[0] == 2
    with pytest.raises(cabi.TchGeoError, match="pitch_nodes"):
        ask((124, -1, 77))
    with pytest.raises(cabi.TchGeoError, match="id_bound"):
        ask((124, 300, 77), (1 << 20, 0, 1 << 20))
    with pytest.raises(cabi.TchGeoError, match="n_types"):
        cabi.ns_typed_unique_form([], [], LDS)
    with pytest.raises(cabi.TchGeoError, match="n_types"):
        cabi.ns_typed_unique_form([8] * 9, [8] * 9, LDS)


@pytest.mark.parametrize("pitches,bounds", [((124, 300, 77), (34, 50, 60)), ((40000, 5, 2000), (1 << 24,) * 3),
                                            ((169984, 87040, 15360), (1 << 23, 1 << 22, 1 << 41)), ((0, 33000), (5, 5))])
def test_workspace_sizes(cabi, pitches, bounds):
    """bytes_min is one batch's tables, slot words and tile counts of every type; bytes is all batches at once, or 0 where
    an auto call takes the LDS form on the current device (without a device it never does)."""
    total, least = cabi.ns_typed_unique_workspace_bytes(list(pitches), list(bounds), 16)
    floor = sum(slots_of(p) * ((4 if b <= 1 << 31 else 8) + 4) + 4 * p for p, b in zip(pitches, bounds))
    assert least % 256 == 0 and floor <= least <= floor + sum(4 * (p // 1024 + 1) + 4 * 256 for p in pitches)
    assert cabi.ns_typed_unique_workspace_bytes(list(pitches), list(bounds), 1)[1] == least
    auto_form = cabi.ns_typed_unique_form(list(pitches), list(bounds), 0)[0]  # asks the same device, if any
    assert total == (0 if auto_form == 1 else 16 * least)
    if max(pitches) > 32768:
        assert cabi.ns_typed_unique_form(list(pitches), list(bounds), LDS)[0] == 2
        assert total == 16 * least > 0                                        # fits no LDS anywhere
    with pytest.raises(cabi.TchGeoError, match="n_batches"):
        cabi.ns_typed_unique_workspace_bytes(list(pitches), list(bounds), -1)


def _call(cabi, src=True, dst=True, n_batches=4, n_types=3, n_rels=4, rel_src=(0, 1, 2, 0), rel_dst=(1, 0, 2, 2),
          pitch_nodes=(124, 300, 77), pitch_edges=(120, 60, 30, 8), stride=None, id_bound=(1 << 20,) * 3, ws=None, ws_bytes=0,
          form=2):
    i32 = lambda xs, n: (C.c_int32 * n)(*(list(xs) + [0] * n)[:n])
    i64 = lambda xs, n: (C.c_int64 * n)(*(list(xs) + [1] * n)[:n])
    T, R = max(n_types, 1), max(n_rels, 1)
    keep = [i32(rel_src, R), i32(rel_dst, R), i64(pitch_nodes, T), i64(pitch_edges, R), i64(id_bound, T), i64([4, 0, 0], T)]
    si, so = cabi.TgNsTypedIn(), cabi.TgNsTypedUniqueOut()
    si.n_types, si.n_rels, si.rel_src, si.rel_dst = n_types, n_rels, keep[0], keep[1]
    si.pitch_nodes, si.pitch_edges, si.id_bound, si.n_inputs = keep[2], keep[3], keep[4], keep[5]
    si.counts_stride = n_types + n_rels if stride is None else stride
    rc = cabi.lib.tg_ns_typed_unique(C.byref(si) if src else None, C.c_int64(n_batches), C.byref(so) if dst else None, ws,
                                     C.c_int64(ws_bytes), C.c_int32(form), None)
    return rc, cabi.lib.tg_last_error().decode()


def _refused(cabi, word, **kw):
    rc, msg = _call(cabi, **kw)
    assert rc == 1, (rc, msg)                                                 # TG_ERR_INVALID
    assert "tg_ns_typed_unique" in msg and word in msg, msg


def test_refusals_before_any_launch(cabi):
    """Every bad argument returns TG_ERR_INVALID with a message that names it; the slab pointers are all null, so nothing
    can have been launched."""
    least = cabi.ns_typed_unique_workspace_bytes([124, 300, 77], [1 << 20] * 3, 4)[1]
    buf = C.create_string_buffer(least + 16)                                  # stands in for a workspace; never read
    base = (C.addressof(buf) + 7) & ~7
    ws = C.c_void_p(base)
    ok = dict(ws=ws, ws_bytes=least)
    _refused(cabi, "null", src=False, **ok)
    _refused(cabi, "null", dst=False, **ok)
    _refused(cabi, "n_batches", n_batches=-1, **ok)
    _refused(cabi, "n_types", n_types=0, **ok)
    _refused(cabi, "n_types", n_types=9, pitch_nodes=(8,) * 9, id_bound=(8,) * 9, **ok)
    _refused(cabi, "n_rels", n_rels=17, rel_src=(0,) * 17, rel_dst=(0,) * 17, pitch_edges=(8,) * 17, **ok)
    _refused(cabi, "n_rels", n_rels=-1, **ok)
    _refused(cabi, "rel_src", rel_src=(0, 3, 2, 0), **ok)
    _refused(cabi, "rel_src", rel_src=(0, -1, 2, 0), **ok)
    _refused(cabi, "rel_dst", rel_dst=(1, 0, 2, 7), **ok)
    _refused(cabi, "counts_stride", stride=6, **ok)
    _refused(cabi, "pitch_nodes", pitch_nodes=(124, -300, 77), **ok)
    _refused(cabi, "pitch_nodes", pitch_nodes=(124, (1 << 30) + 1, 77), **ok)
    _refused(cabi, "pitch_edges", pitch_edges=(120, 60, -30, 8), **ok)
    _refused(cabi, "id_bound", id_bound=(1 << 20, 1 << 20, 0), **ok)
    _refused(cabi, "workspace_bytes", ws=ws, ws_bytes=-1)
    _refused(cabi, "form", form=3, **ok)
    _refused(cabi, "form", form=-1, **ok)
    _refused(cabi, "does not fit", form=1, pitch_nodes=(124, 200000, 77))     # past any workgroup's LDS
    _refused(cabi, "workspace too small", ws=ws, ws_bytes=least - 1)          # below bytes_min
    _refused(cabi, "workspace too small", ws=None, ws_bytes=1 << 30)          # the flat form without a workspace
    _refused(cabi, "aligned", ws=C.c_void_p(base + 4), ws_bytes=least)        # misaligned workspace
    # well-formed sizes and a large enough workspace: the null slabs are refused, still before any launch
    _refused(cabi, "null", **ok)
    assert _call(cabi, n_batches=0, **ok)[0] == 0                             # nothing to do
    assert _call(cabi, n_batches=0, stride=10, **ok)[0] == 0                  # a wider counts row is fine


def rule_per_type(samples, rows, cols, ends):
    """unique_rule applied per node type, the relations relabelled through the two inverses."""
    per = {t: unique_rule(s, [], []) for t, s in samples.items()}
    nodes, inverse = {t: per[t][0] for t in per}, {t: per[t][1] for t in per}
    rows_u = {k: inverse[ends[k][0]][np.asarray(rows[k], dtype=np.int64)] for k in rows}
    cols_u = {k: inverse[ends[k][1]][np.asarray(cols[k], dtype=np.int64)] for k in rows}
    return nodes, rows_u, cols_u, inverse


def test_unique_nodes_hetero_on_cpu_tensors_matches_the_rule(cabi):
    from tch_geometric.transforms import unique_nodes_hetero
    rs = np.random.default_rng(11)
    samples = {"a": rs.integers(0, 40, 300), "b": np.concatenate([[5, 5, 2, 5], rs.integers(0, 9, 50)]),
               "c": np.zeros(0, dtype=np.int64), "d": np.full(20, 7)}
    edge_types = [("a", "to", "b"), ("b", "rev", "a"), ("a", "self", "a"), ("d", "to", "a"), ("c", "none", "c")]
    ends = {"__".join(et): (et[0], et[2]) for et in edge_types}
    rows, cols = {}, {}
    for k, (s, d) in ends.items():
        m = 0 if "c" in (s, d) else 2 * samples[s].size + 3
        rows[k], cols[k] = rs.integers(0, max(samples[s].size, 1), m), rs.integers(0, max(samples[d].size, 1), m)
    samples = {t: np.asarray(v, dtype=np.int64) for t, v in samples.items()}
    want = rule_per_type(samples, rows, cols, ends)
    tt = lambda d: {k: torch.from_numpy(np.asarray(v, dtype=np.int64)) for k, v in d.items()}
    got = unique_nodes_hetero(tt(samples), tt(rows), tt(cols), edge_types, num_nodes={"a": 40, "b": 9})
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            assert g[k].dtype == torch.int64 and np.array_equal(g[k].numpy(), w[k]), k
    nodes, rows_u, cols_u, inverse = got
    assert nodes["c"].numel() == 0 and nodes["d"].tolist() == [7] and nodes["b"][:2].tolist() == [5, 2]
    for k, (s, d) in ends.items():                                           # an edge still joins the same two ids
        assert np.array_equal(nodes[s].numpy()[rows_u[k].numpy()], samples[s][rows[k]])
        assert np.array_equal(nodes[d].numpy()[cols_u[k].numpy()], samples[d][cols[k]])
    with pytest.raises(ValueError):
        unique_nodes_hetero({"a": torch.zeros(3, dtype=torch.int32)}, {}, {}, [])
    with pytest.raises(ValueError):
        unique_nodes_hetero(tt(samples), {"a__to__zz": torch.zeros(0, dtype=torch.int64)},
                            {"a__to__zz": torch.zeros(0, dtype=torch.int64)}, edge_types)


def test_unique_nodes_hetero_on_cpu_tensors_gives_minus_one_for_an_end_outside_its_list(cabi):
    """rows index the source type's list and cols the destination's: a negative end or one past ITS list's length is no
    position and gives -1 (as the device path does), also where it would be a position of the other type's list."""
    from tch_geometric.transforms import unique_nodes_hetero
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    samples = {"a": i64([9, 4, 9, 7, 4]), "b": i64([3, 3]), "c": i64([])}
    edge_types = [("a", "to", "b"), ("b", "to", "c"), ("a", "self", "a")]
    rows = {"a__to__b": i64([0, -1, 4, 5, 2]), "b__to__c": i64([1, 2, -3]), "a__self__a": i64([4, 1 << 40, 3])}
    cols = {"a__to__b": i64([1, 0, 2, 0, -1]), "b__to__c": i64([0, 0, 0]), "a__self__a": i64([-1, 0, 5])}
    nodes, rows_u, cols_u, inverse = unique_nodes_hetero(samples, rows, cols, edge_types)
    assert nodes["a"].tolist() == [9, 4, 7] and nodes["b"].tolist() == [3] and nodes["c"].numel() == 0
    assert inverse["a"].tolist() == [0, 1, 0, 2, 1] and inverse["b"].tolist() == [0, 0]
    assert rows_u["a__to__b"].tolist() == [0, -1, 1, -1, 0] and cols_u["a__to__b"].tolist() == [0, 0, -1, 0, -1]
    assert rows_u["b__to__c"].tolist() == [0, -1, -1] and cols_u["b__to__c"].tolist() == [-1, -1, -1]
    assert rows_u["a__self__a"].tolist() == [1, -1, 2] and cols_u["a__self__a"].tolist() == [-1, 0, -1]
    for k in rows:
        assert rows_u[k].dtype == torch.int64 and cols_u[k].dtype == torch.int64
