"""The table of tests/test_gpu_stream_order_lastn.py cannot rot: every TG_API function of include/tchgeo_lastn.h that takes a
`void *stream` and every function of tch_geometric/_cabi_lastn.py that calls stream_ptr is named by a case of its CASES, with
its class, or by its EXEMPT, with its reason (what tests/test_stream_contract_cpu.py does for include/tchgeo.h and _cabi.py,
with its parsers).  Needs no GPU."""
import os

import helpers_stream as hs
import test_gpu_stream_order_lastn as table
from test_stream_contract_cpu import cabi_functions, cabi_stream_functions, header_functions, header_stream_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_lastn.h")
CABI = os.path.join(ROOT, "tch-geometric_amd", "tch_geometric", "_cabi_lastn.py")
STREAM = ["tg_lastn_insert", "tg_lastn_replay", "tg_lastn_reset", "tg_lastn_sample"]


def _classified():
    named = {}
    for case in table.CASES:
        assert case.cls in (hs.ASYNC, hs.READS_BACK), case.id
        assert "tch_geometric._cabi_lastn" in case.modules, case.id      # the arena stands in for torch in the new module too
        for name in case.names:
            named.setdefault(name, set()).add(case.cls)
    return named


def test_the_parsers_find_the_new_entry_points():
    assert header_stream_functions(open(HEADER).read()) == STREAM
    assert header_functions(open(HEADER).read()) == set(STREAM) | {"tg_lastn_state_bytes", "tg_lastn_insert_workspace_bytes",
                                                                   "tg_lastn_replay_workspace_bytes"}
    assert cabi_stream_functions(open(CABI).read()) == ["LastN.insert", "LastN.replay", "LastN.reset", "LastN.sample"]


def test_every_stream_taking_entry_point_is_classified():
    named = _classified()
    for name in header_stream_functions(open(HEADER).read()) + cabi_stream_functions(open(CABI).read()):
        assert name in named or name in table.EXEMPT, "%s has neither a case nor an exemption" % name
        assert named.get(name, {hs.ASYNC}) == {hs.ASYNC}, name          # the header promises no synchronisation


def test_the_table_names_only_what_exists():
    c_api, wrappers = header_functions(open(HEADER).read()), cabi_functions(open(CABI).read())
    for name in list(_classified()) + list(table.EXEMPT):
        assert (name in c_api) if name.startswith("tg_") else (name in wrappers), name
    ids = [c.id for c in table.CASES]
    assert len(ids) == len(set(ids))


def test_a_deleted_case_is_noticed(monkeypatch):
    import pytest
    monkeypatch.setattr(table, "CASES", [])
    with pytest.raises(AssertionError, match="tg_lastn_insert"):
        test_every_stream_taking_entry_point_is_classified()
