"""The table of tests/test_gpu_stream_order.py cannot rot: every TG_API function of include/tchgeo.h that takes a
`void *stream` and every function of tch_geometric/_cabi.py that calls stream_ptr is named by a case of CASES, with its
class, or by EXEMPT, with its reason.  A new entry point fails here until someone classifies it.  Needs no GPU."""
import ast
import os
import re

import helpers_stream as hs
import test_gpu_stream_order as table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo.h")
CABI = os.path.join(ROOT, "tch-geometric_amd", "tch_geometric", "_cabi.py")
SURFACE = ["tch_geometric.neighbor_sampling_homogenous", "tch_geometric.neighbor_sampling_heterogenous",
           "tch_geometric.hgt_sampling", "tch_geometric.budget_sampling", "tch_geometric.negative_sampling",
           "tch_geometric.random_walk", "tch_geometric.to_csc"]


def header_stream_functions(text):
    """every `TG_API <type> tg_name(... void *stream ...);` of the header"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return sorted(name for name, args in decls if re.search(r"\bvoid\s*\*\s*stream\b", args))


def header_functions(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return set(re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text))


def cabi_stream_functions(source):
    """every function or method of _cabi.py whose body calls stream_ptr, as `name` or `Class.name`"""
    found = []

    def calls_stream_ptr(fn):
        return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "stream_ptr" for n in ast.walk(fn))

    def visit(body, prefix):
        for node in body:
            if isinstance(node, ast.FunctionDef):
                if node.name != "stream_ptr" and calls_stream_ptr(node):
                    found.append(prefix + node.name)
            elif isinstance(node, ast.ClassDef):
                visit(node.body, prefix + node.name + ".")
    visit(ast.parse(source).body, "")
    return sorted(found)


def cabi_functions(source):
    names = set()

    def visit(body, prefix):
        for node in body:
            if isinstance(node, ast.FunctionDef):
                names.add(prefix + node.name)
            elif isinstance(node, ast.ClassDef):
                visit(node.body, prefix + node.name + ".")
    visit(ast.parse(source).body, "")
    return names


def _classified():
    named = {}
    for case in table.CASES:
        assert case.cls in (hs.ASYNC, hs.READS_BACK), case.id
        for name in case.names:
            named.setdefault(name, set()).add(case.cls)
    return named


def test_the_parsers_find_what_they_should():
    text = open(HEADER).read()
    fns = header_stream_functions(text)
    assert len(fns) >= 73 and "tg_ns_rows_fill" in fns and "tg_part_sample_ws" in fns and "tg_probe_ns_sol" in fns
    assert "tg_ns_homo_capacity" not in fns and "tg_ns_win_stage_times" not in fns          # no stream parameter
    assert len(fns) == len(re.findall(r"void\s*\*\s*stream\s*\)\s*;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    src = "def a(d):\n    return stream_ptr(d)\nclass K:\n    def m(self):\n        f(stream_ptr(self.d))\n    def n(self):\n        pass\n" \
          "def stream_ptr(d):\n    return d\ndef b():\n    pass\n"
    assert cabi_stream_functions(src) == ["K.m", "a"]
    wrappers = cabi_stream_functions(open(CABI).read())
    assert len(wrappers) >= 45 and "ns_hop" in wrappers and "NsInduced.count" in wrappers and "_Batched.run" in wrappers


def test_every_stream_taking_entry_point_is_classified():
    named = _classified()
    missing = [n for n in header_stream_functions(open(HEADER).read()) if n not in named and n not in table.EXEMPT]
    assert not missing, "C entry points with a stream parameter and neither a case nor an exemption in " \
        "tests/test_gpu_stream_order.py: %s" % missing
    missing = [n for n in cabi_stream_functions(open(CABI).read()) if n not in named and n not in table.EXEMPT]
    assert not missing, "_cabi.py functions that call stream_ptr and have neither a case nor an exemption: %s" % missing
    missing = [n for n in SURFACE if n not in named]
    assert not missing, "operator-surface functions without a case: %s" % missing


def test_the_table_names_only_what_exists():
    named = _classified()
    c_api, wrappers = header_functions(open(HEADER).read()), cabi_functions(open(CABI).read())
    for name in list(named) + list(table.EXEMPT):
        if name.startswith("tch_geometric."):
            assert name in SURFACE, name
        elif name.startswith("tg_"):
            assert name in c_api, "%s is not declared in include/tchgeo.h" % name
        else:
            assert name in wrappers, "%s is not a function of _cabi.py" % name
    for name, reason in table.EXEMPT.items():
        assert name not in named, "%s has a case and an exemption" % name
        assert isinstance(reason, str) and len(reason) > 10, name
    ids = [c.id for c in table.CASES]
    assert len(ids) == len(set(ids))


def test_a_deleted_case_or_exemption_is_noticed(monkeypatch):
    """the completeness test fails when the table loses an entry"""
    import pytest
    monkeypatch.setattr(table, "CASES", [c for c in table.CASES if "tg_ns_hop_labor" not in c.names])
    with pytest.raises(AssertionError, match="tg_ns_hop_labor"):
        test_every_stream_taking_entry_point_is_classified()
    monkeypatch.undo()
    monkeypatch.setattr(table, "EXEMPT", {k: v for k, v in table.EXEMPT.items() if k != "tg_probe_ns_sol"})
    with pytest.raises(AssertionError, match="tg_probe_ns_sol"):
        test_every_stream_taking_entry_point_is_classified()
