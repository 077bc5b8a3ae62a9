"""lp_partition end to end: equal to the restatement chained over its rounds (part and stats), a function of the seed, usable
by ClusterData / ClusterLoader, and on the planted-partition graph the cut the CPU test bounds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_lp as hl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def edges(n, e, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, n, (2, e)).astype(np.int64))


def restated(ei, n, P, slack, rounds, seed, init=None):
    ei = ei.numpy()
    ptrs, idx = hl.csr(n, np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]]))
    return hl.run(ptrs, idx, np.arange(n) * P // n if init is None else init, P, slack, rounds, seed)


def test_partition_equals_the_chained_restatement_and_depends_on_the_seed():
    from tch_geometric import lp_partition
    n, P = 700, 12
    ei = edges(n, 5000, 1)
    part, stats = lp_partition(ei, n, P, slack=1.05, rounds=5, seed=3, device=DEV, return_stats=True)
    want, wstats = restated(ei, n, P, 1.05, 5, 3)
    assert part.dtype == torch.int64 and part.device == torch.device(DEV) and part.tolist() == want.tolist()
    assert stats["cut"] == wstats["cut"] and stats["moved"] == wstats["moved"] and stats["cap"] == wstats["cap"]
    assert stats["sizes"].tolist() == wstats["sizes"].tolist() == np.bincount(want, minlength=P).tolist()
    assert max(wstats["sizes"]) <= wstats["cap"] and wstats["moved"][0] > 0
    other = lp_partition(ei, n, P, slack=1.05, rounds=5, seed=4, device=DEV)
    assert other.tolist() == restated(ei, n, P, 1.05, 5, 4)[0].tolist() != want.tolist()
    with pytest.raises(ValueError, match="init holds part ids"):
        lp_partition(ei, n, P, init=torch.full((n,), P), device=DEV)


def test_partition_feeds_cluster_data_and_loader():
    from tch_geometric import ClusterData, ClusterLoader, lp_partition
    from tch_geometric.transforms import Graph
    n, P = 700, 8
    data = Graph(edge_index=edges(n, 4000, 2).to(DEV), num_nodes=n, x=torch.arange(n, device=DEV, dtype=torch.float32)[:, None])
    part = lp_partition(data.edge_index, n, P, rounds=4, device=DEV)
    seen = 0
    for batch in ClusterLoader(ClusterData(data, part, num_parts=P, device=DEV), batch_size=2, shuffle=True, seed=1):
        assert torch.equal(data.edge_index[:, batch.e_id], batch.n_id[batch.edge_index])
        seen += batch.num_nodes
    assert seen == n


def test_planted_partition_cut_equals_the_restatement():
    from tch_geometric import lp_partition
    ptrs, idx = hl.planted()
    n, P = len(ptrs) - 1, 16
    row = np.repeat(np.arange(n), np.diff(ptrs))
    part, stats = lp_partition(torch.from_numpy(np.stack([row, idx])), n, P, rounds=40, symmetric=False, device=DEV,
                               return_stats=True)
    want, wstats = hl.run(ptrs, idx, np.arange(n) * P // n, P, 1.1, 40, 0)
    assert stats["cut"] == wstats["cut"] and part.tolist() == want.tolist()     # the number test_lp_cpu.py bounds


def test_example_with_lp_prints_a_smaller_cut():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cluster_gcn_loader.py"), "--partition", "lp"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    before, after = map(float, re.search(r"cut share before ([\d.]+), after ([\d.]+)", r.stdout).groups())
    assert after < before and "fell: True" in r.stdout
