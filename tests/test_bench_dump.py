"""`bench.py --dump-outputs DIR`: which mini-batches of the last timed step are written (fixed by the arguments alone, within
64 MB) and how they are laid out on disk.  CPU only: the slabs are host tensors filled by hand."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tch_geometric import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_arguments(bench):
    assert bench.parse_args([]).dump_outputs is None
    a = bench.parse_args(["--dump-outputs", "out_dir", "--steps", "3", "--warmup", "0"])
    assert a.dump_outputs == "out_dir" and a.steps == 3 and a.warmup == 0
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "d", "--mode", "partitioned"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_plan_is_fixed_and_fits_the_budget(bench):
    B, fanout, G = 1024, [15, 10], 16384
    cap_nodes, cap_edges = _cabi.ns_homo_capacity(B, fanout)
    ids = bench.dump_plan(G, B, cap_nodes, cap_edges, len(fanout))
    assert np.array_equal(ids, bench.dump_plan(G, B, cap_nodes, cap_edges, len(fanout)))
    assert len(ids) >= 8 and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < G
    worst = 8 * (2 * G + len(ids) * (1 + B + 2 + 3 * len(fanout) + cap_nodes + 3 * cap_edges))
    assert worst <= bench.DUMP_BUDGET
    assert np.array_equal(bench.dump_plan(4, B, cap_nodes, cap_edges, 2), np.arange(4))   # few batches: all of them
    with pytest.raises(SystemExit):
        bench.dump_plan(G, B, cap_nodes, cap_edges, 2, budget=1 << 20)


def test_dump_writes_the_sampled_batches(bench, tmp_path):
    G, B, fanout = 6, 4, [2, 2]
    out = _cabi.NsBatchedOut(G, B, fanout, torch.device("cpu"))
    for t in (out.samples, out.rows, out.cols, out.edge_index):
        t.copy_(torch.arange(t.numel(), dtype=torch.int64).view_as(t))
    out.counts.copy_(torch.tensor([[4 + b, 2 * b] for b in range(G)]))
    out.layer_offsets.copy_(torch.arange(out.layer_offsets.numel()).view_as(out.layer_offsets))
    seeds = torch.arange(G * B, dtype=torch.int64).view(G, B) + 100
    ids = np.array([1, 3, 4])
    bench.dump_outputs(str(tmp_path / "d"), out, seeds, 1000, ids, len(fanout))
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert set(got) == {"counts", "batch_ids", "call_ids", "seeds", "layer_offsets", "samples", "rows", "cols", "edge_index"}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["counts"], out.counts.numpy()) and np.array_equal(got["batch_ids"], ids)
    assert np.array_equal(got["call_ids"], ids + 1000) and np.array_equal(got["seeds"], seeds[ids].numpy())
    assert np.array_equal(got["layer_offsets"], out.layer_offsets[ids].numpy())
    for name, slab, col in (("samples", out.samples, 0), ("rows", out.rows, 1), ("cols", out.cols, 1),
                            ("edge_index", out.edge_index, 1)):
        want = np.concatenate([slab[j, :int(out.counts[j, col])].numpy() for j in ids])
        assert np.array_equal(got[name], want), name
