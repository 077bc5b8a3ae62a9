"""Layer-neighbor sampling (LABOR-0, Balin & Catalyurek 2023; DGL's LaborSampler): NeighborLoader(labor=True).  Every vertex
gets one random variate per mini-batch and hop, shared by all seeds of the mini-batch, and a frontier vertex keeps the
num_neighbors neighbours with the smallest ones.  Each vertex still gets a uniform subset of its neighbours, but the seeds
of a mini-batch pick the same ones, so the mini-batch lists fewer distinct nodes -- fewer feature rows to gather, fewer
rows for the model to compute.  Plain torch, no torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric.loader import NeighborLoader

data = fake_dataset(num_nodes=20000, avg_degree=20)
input_nodes = torch.arange(4096, device="cuda")

for name, kw in (("uniform", {}), ("labor", dict(labor=True)), ("labor + layer_dependency", dict(labor=True, layer_dependency=True))):
    loader = NeighborLoader(data, [10, 10], input_nodes=input_nodes, batch_size=512, prefetch=4, seed=0, unique=True, **kw)
    nodes = edges = 0
    for batch in loader:
        assert batch.x.shape[0] == batch.num_nodes           # one feature row per distinct node
        nodes += batch.num_nodes
        edges += batch.num_edges
    print("%s: %d mini-batches of %d seeds, %.1f distinct nodes and %.1f edges per mini-batch"
          % (name, len(loader), loader.batch_size, nodes / len(loader), edges / len(loader)))
