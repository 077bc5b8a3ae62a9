"""ShaDow-GNN style training data (PyG's ShaDowKHopSampler): every seed gets its own bounded neighbourhood, and the
mini-batch holds every edge of the graph inside each neighbourhood -- a deep model over a shallow, localised subgraph.  One
untimed epoch, then one under edge times, where a subgraph only holds edges no later than its seed.  Plain torch, no
torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric import ShaDowKHopLoader

data = fake_dataset()
gen = torch.Generator().manual_seed(1)
data.time = torch.randint(0, 100, (data.edge_index.shape[1],), generator=gen).to("cuda")   # int64 [E], in edge_index order
input_nodes = torch.arange(data.num_nodes, device="cuda")
input_time = torch.randint(20, 100, (data.num_nodes,), generator=torch.Generator().manual_seed(3)).to("cuda")

for name, kw in (("untimed", {}), ("timed", dict(time_attr="time", input_time=input_time, time_window=(0, 50)))):
    loader = ShaDowKHopLoader(data, depth=2, num_neighbors=5, input_nodes=input_nodes, batch_size=128, prefetch=4, seed=0, **kw)
    nodes = edges = 0
    shared = True
    for batch in loader:
        row, col = batch.edge_index
        shared &= bool((batch.batch[row] == batch.batch[col]).all())         # an edge never leaves its seed's subgraph
        assert torch.equal(batch.batch[batch.root_n_id], torch.arange(batch.batch_size, device="cuda"))
        x_root = batch.x[batch.root_n_id]                                    # what a ShaDow model pools per subgraph, beside
        assert x_root.shape[0] == batch.batch_size                           # a readout over batch.batch
        if kw:
            age = batch.node_time[col] - batch.time                          # the edge times come like any edge attribute
            assert bool(((age >= 0) & (age <= 50)).all())
        nodes += batch.num_nodes
        edges += batch.num_edges
    print("%s: %d mini-batches of up to %d subgraphs, %d nodes, %d induced edges, both ends of every edge share batch: %s"
          % (name, len(loader), loader.batch_size, nodes, edges, shared))
