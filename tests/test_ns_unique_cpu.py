"""Per-batch node dedup (tg_ns_homo_unique), host-only parts: the exports, the form query with a stated LDS limit, the
workspace sizes, the argument checks that run before anything is launched, and transforms.unique_nodes on CPU tensors
against the NumPy statement of the rule.  No GPU: every device pointer handed over is null (the workspace of the
short-workspace case is a host buffer that is never read)."""
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
NAMES = ("tg_ns_homo_unique_form", "tg_ns_homo_unique_workspace_bytes", "tg_ns_homo_unique")


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
    assert sorted(cabi.EXPORTS) == sorted(declared)
    assert "tg_ns_unique_out" in header
    assert [f for f, _ in cabi.TgNsUniqueOut._fields_] == ["nodes", "inverse", "rows", "cols", "counts", "layer_nodes"]


def test_form_query_with_a_stated_lds_limit(cabi):
    """A table of 2^k >= 4/3 cap_nodes slots of (key, u32 value) plus a u16 word per position must fit the workgroup: with
    160 KiB and 32-bit keys that is cap_nodes <= 12 288 (16 384 slots x 8 B = 128 KiB + 24 KiB of words)."""
    form, lds, bound = cabi.ns_homo_unique_form(12288, 1 << 24, LDS)
    assert form == 1 and 16384 * 8 + 2 * 12288 <= lds <= LDS and bound == 12288
    assert cabi.ns_homo_unique_form(bound + 1, 1 << 24, LDS)[0] == 2          # one slot more than the reported bound
    assert cabi.ns_homo_unique_form(124, 1 << 24, LDS)[0] == 1
    assert cabi.ns_homo_unique_form(169984, 1 << 24, LDS)[0] == 2             # the loader's shape: 1 024 x [15, 10]
    form64k, _, bound64k = cabi.ns_homo_unique_form(3072, 1 << 24, 64 * 1024)
    assert form64k == 1 and bound64k == 3072 < bound                         # a device with less LDS
    assert cabi.ns_homo_unique_form(3073, 1 << 24, 64 * 1024)[0] == 2
    # ids past 2^31 take 64-bit keys: 12 bytes per slot, half the bound
    assert cabi.ns_homo_unique_form(12288, 1 << 31, LDS)[0] == 1              # [0, 2^31) still fits 32-bit keys
    form, lds, bound64 = cabi.ns_homo_unique_form(6144, (1 << 31) + 1, LDS)
    assert form == 1 and lds >= 8192 * 12 and bound64 == bound // 2
    assert cabi.ns_homo_unique_form(6145, 1 << 41, LDS)[0] == 2
    with pytest.raises(cabi.TchGeoError, match="cap_nodes"):
        cabi.ns_homo_unique_form(-1, 1 << 24, LDS)
    with pytest.raises(cabi.TchGeoError, match="id_bound"):
        cabi.ns_homo_unique_form(64, 0, LDS)


@pytest.mark.parametrize("cap_nodes,id_bound", [(124, 34), (12289, 1 << 24), (169984, 1 << 24), (169984, 1 << 41)])
def test_workspace_sizes(cabi, cap_nodes, id_bound):
    """bytes_min is one batch's tables, slot words and tile counts; bytes is all batches at once, or 0 where an auto call
    takes the LDS form on the current device (without a device it never does)."""
    total, least = cabi.ns_homo_unique_workspace_bytes(cap_nodes, id_bound, 16)
    key = 4 if id_bound <= 1 << 31 else 8
    slots = 64
    while slots < (4 * cap_nodes + 2) // 3:
        slots *= 2
    assert least >= slots * (key + 4) + 4 * cap_nodes and least % 256 == 0
    assert least <= slots * (key + 4) + 4 * cap_nodes + 4 * (cap_nodes // 1024 + 1) + 4 * 256
    auto_form = cabi.ns_homo_unique_form(cap_nodes, id_bound, 0)[0]           # asks the same device, if any
    assert total == (0 if auto_form == 1 else least * 16)
    assert cabi.ns_homo_unique_workspace_bytes(cap_nodes, id_bound, 1)[1] == least
    if cap_nodes > 12288:
        assert total == least * 16 > 0                                        # fits no LDS anywhere
    with pytest.raises(cabi.TchGeoError, match="n_batches"):
        cabi.ns_homo_unique_workspace_bytes(cap_nodes, id_bound, -1)


def _call(cabi, src=True, dst=True, n_batches=4, n_seeds=4, n_hops=2, id_bound=1 << 20, cap_nodes=124, cap_edges=120,
          ws=None, ws_bytes=0, form=2):
    so, uo = cabi.TgNsOut(), cabi.TgNsUniqueOut()
    so.cap_nodes, so.cap_edges = cap_nodes, cap_edges
    rc = cabi.lib.tg_ns_homo_unique(C.byref(so) if src else None, C.c_int64(n_batches), C.c_int64(n_seeds), C.c_int32(n_hops),
                                    C.c_int64(id_bound), C.byref(uo) if dst else None, ws, C.c_int64(ws_bytes),
                                    C.c_int32(form), None)
    return rc, cabi.lib.tg_last_error().decode()


def _refused(cabi, word, **kw):
    rc, msg = _call(cabi, **kw)
    assert rc == 1, (rc, msg)                                                 # TG_ERR_INVALID
    assert "tg_ns_homo_unique" in msg and word in msg, msg


def test_refusals_before_any_launch(cabi):
    """Every bad argument returns TG_ERR_INVALID with a message that names it; the slab pointers are all null, so nothing
    can have been launched."""
    least = cabi.ns_homo_unique_workspace_bytes(124, 1 << 20, 4)[1]
    buf = C.create_string_buffer(least + 8)                                   # stands in for a workspace; never read
    ws = C.c_void_p((C.addressof(buf) + 7) & ~7)
    _refused(cabi, "null", src=False, ws=ws, ws_bytes=least)
    _refused(cabi, "null", dst=False, ws=ws, ws_bytes=least)
    _refused(cabi, "n_batches", n_batches=-1, ws=ws, ws_bytes=least)
    _refused(cabi, "n_seeds", n_seeds=-4, ws=ws, ws_bytes=least)
    _refused(cabi, "n_hops", n_hops=-1, ws=ws, ws_bytes=least)
    _refused(cabi, "n_hops", n_hops=9, ws=ws, ws_bytes=least)
    _refused(cabi, "cap_nodes", cap_nodes=-5, ws=ws, ws_bytes=least)
    _refused(cabi, "cap_edges", cap_edges=-5, ws=ws, ws_bytes=least)
    _refused(cabi, "id_bound", id_bound=0, ws=ws, ws_bytes=least)
    _refused(cabi, "workspace_bytes", ws=ws, ws_bytes=-1)
    _refused(cabi, "workspace too small", ws=ws, ws_bytes=least - 1)          # below bytes_min
    _refused(cabi, "workspace too small", ws=None, ws_bytes=1 << 30)          # a size without a workspace
    _refused(cabi, "form", form=3, ws=ws, ws_bytes=least)
    _refused(cabi, "form", form=-1, ws=ws, ws_bytes=least)
    _refused(cabi, "does not fit", form=1, cap_nodes=200000)                  # past any workgroup's LDS
    # well-formed sizes and a large enough workspace: the null slabs are refused, still before any launch
    _refused(cabi, "null", ws=ws, ws_bytes=least)
    assert _call(cabi, n_batches=0, ws=ws, ws_bytes=least)[0] == 0            # nothing to do


@pytest.mark.parametrize("case", ["random", "all equal", "all distinct", "duplicate seeds", "no edges", "empty"])
def test_unique_nodes_on_cpu_tensors_matches_the_rule(cabi, case):
    from tch_geometric.transforms import unique_nodes
    rs = np.random.default_rng(7)
    if case == "random":
        s = rs.integers(0, 50, 400)
    elif case == "all equal":
        s = np.full(100, 17)
    elif case == "all distinct":
        s = rs.permutation(300)
    elif case == "duplicate seeds":
        s = np.array([0, 0, 1, 0, 5, 1, 9, 0])
    elif case == "no edges":
        s = np.array([4, 4, 2])
    else:
        s = np.zeros(0, dtype=np.int64)
    s = s.astype(np.int64)
    m = 0 if case in ("no edges", "empty") else 3 * s.size
    rows, cols = rs.integers(0, max(s.size, 1), m), rs.integers(0, max(s.size, 1), m)
    nodes, inverse, rows_u, cols_u, _ = unique_rule(s, rows, cols)
    got = unique_nodes(torch.from_numpy(s), torch.from_numpy(rows.astype(np.int64)), torch.from_numpy(cols.astype(np.int64)))
    for g, w in zip(got, (nodes, rows_u, cols_u, inverse)):
        assert g.dtype == torch.int64 and np.array_equal(g.numpy(), w)
    assert np.array_equal(nodes[inverse], s) and len(set(nodes.tolist())) == nodes.size
    with pytest.raises(ValueError):
        unique_nodes(torch.from_numpy(s).to(torch.int32), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
