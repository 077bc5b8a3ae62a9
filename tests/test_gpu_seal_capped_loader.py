"""SEALLoader(max_nodes_per_hop=...): every mini-batch has the nodes, link slots and labels of the restatement
(helpers_seal_capped) under the call id (epoch * L when resampled) + the link's position, and the edges of the per-subgraph
induced rule on those lists; a link's subgraph does not depend on prefetch or batch size; None changes nothing; the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_seal_capped as hc
from helpers_shadow import grouped_induced_rule
from test_gpu_seal_loader import CAP, HOPS, L, ZMAX, graph, loader  # noqa: F401  (graph: the fixture; its links sit on the hub)

pytestmark = pytest.mark.gpu
CAPS, SEED = [8, 4], 11


def per_link(g, ld, epochs=1):
    """-> {(epoch, position of the link): (n_id, z, edges)} of every link the loader serves, checked against the restatement"""
    ptrs, indices, _ = g["csc"]
    out = {}
    for epoch in range(epochs):
        at = 0
        for mb in ld:
            n_id, batch, z = mb.n_id.cpu().numpy(), mb.batch.cpu().numpy(), mb.z.cpu().numpy()
            rows, cols, _ = grouped_induced_rule(n_id, batch, ptrs, indices, n_groups=ld.batch_size)
            assert np.array_equal(mb.edge_index.cpu().numpy(), np.stack([rows, cols]))
            for slot in range(mb.batch_size):
                u, v = g["links"][:, at]
                c_i = at + (epoch * L if ld.resample else 0)
                k = (int(u), int(v), c_i)
                if k not in g["memo"]:
                    g["memo"][k] = hc.seal_capped(ptrs, indices, int(u), int(v), CAPS, CAP, SEED, c_i, ZMAX)
                st, mine = g["memo"][k], batch == slot
                assert n_id[mine].tolist() == st["nodes"] and z[mine].tolist() == st["z"], (epoch, at)
                e = mine[cols]
                out[epoch, at] = (st["nodes"], st["z"], n_id[rows[e]].tolist(), n_id[cols[e]].tolist())
                at += 1
        assert at == L
    return out


def test_two_epochs_resampled_or_not_prefetch_and_batch_size(graph):  # noqa: F811
    a = per_link(graph, loader(graph, max_nodes_per_hop=CAPS, seed=SEED), epochs=2)
    assert any(a[0, i][0] != a[1, i][0] for i in range(L))               # the hub's links draw again in epoch 1
    b = per_link(graph, loader(graph, max_nodes_per_hop=CAPS, seed=SEED, resample=False, prefetch=1, batch_size=5), epochs=2)
    assert all(b[0, i] == b[1, i] == a[0, i] for i in range(L))          # prefetch 1 against 4, batch size 5 against 16
    assert per_link(graph, loader(graph, max_nodes_per_hop=CAPS, seed=SEED, batch_size=32, prefetch=4)) == {k: w for k, w in a.items() if k[0] == 0}
    assert loader(graph, max_nodes_per_hop=CAPS).sizes.node_cap == 14 and loader(graph, max_nodes_per_hop=[8, 0]).sizes.node_cap == CAP


def test_none_is_the_loader_without_the_argument(graph):  # noqa: F811
    for x, y in zip(loader(graph), loader(graph, max_nodes_per_hop=None, resample=False)):
        assert all(torch.equal(getattr(x, n), getattr(y, n)) for n in ("n_id", "batch", "z", "edge_index", "e_id", "root_n_id"))


def test_the_example_with_a_cap_learns():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "examples", "seal_link_prediction.py"), "--max-nodes-per-hop", "16"],
                         cwd=os.path.join(root, "examples"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    auc = float(run.stdout.split("test AUC")[-1].split()[0].strip("=:"))
    assert auc > 0.5, run.stdout
