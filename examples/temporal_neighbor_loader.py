"""Node-level temporal training data (TGN / TGAT style): NeighborLoader with PyG's time_attr / input_time.  Every seed has a
time; only edges no later than it are admitted, and the whole subtree of a seed keeps the seed's time.  Both strategies
run: "uniform" draws among the admitted edges, "last" takes the most recent ones (deterministic).  Plain torch, no
torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric.loader import NeighborLoader

data = fake_dataset()
gen = torch.Generator().manual_seed(1)
data.time = torch.randint(0, 100, (data.edge_index.shape[1],), generator=gen).to("cuda")   # int64 [E], in edge_index order
input_nodes = torch.arange(data.num_nodes, device="cuda")
input_time = torch.randint(20, 100, (data.num_nodes,), generator=torch.Generator().manual_seed(3)).to("cuda")

for strategy in ("uniform", "last"):
    loader = NeighborLoader(data, [10, 5], input_nodes=input_nodes, batch_size=128, prefetch=4, seed=0, time_attr="time",
                            input_time=input_time, temporal_strategy=strategy, time_window=(0, 50))
    nodes = edges = 0
    newest = []
    for batch in loader:
        perm_time = batch.time                               # the sampled edges' times, gathered like any edge attribute
        root_time = batch.node_time[batch.edge_index[1]]     # the time the target of every edge was sampled under
        assert bool(((root_time - perm_time) >= 0).all()) and bool(((root_time - perm_time) <= 50).all())
        assert torch.equal(batch.node_time[:batch.batch_size], batch.input_time)
        nodes += batch.num_nodes
        edges += batch.num_edges
        newest.append(float((root_time - perm_time).float().mean()) if batch.num_edges else 0.0)
    print("%s: %d mini-batches of up to %d seeds, %d nodes, %d edges, every edge inside its seed's window, mean age %.2f"
          % (strategy, len(loader), loader.batch_size, nodes, edges, sum(newest) / len(newest)))
