"""Temporal link prediction data (TGN / CTDNE-style evaluation: "does edge (u, v) appear at time t, given only what
happened before t"): LinkNeighborLoader with PyG's time_attr / edge_label_time.  Every label edge has a time; both of its
endpoints -- and the negatives drawn for it -- sample only edges no later than that time.  unique=True hands out PyG's
disjoint contract: one subgraph per (src, dst) pair, `batch` names every node's subgraph, edge_label_index is numbered
against n_id.  Plain torch, no torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric.loader import LinkNeighborLoader

data = fake_dataset()
n_edges = data.edge_index.shape[1]
data.time = torch.randint(0, 100, (n_edges,), generator=torch.Generator().manual_seed(1)).to("cuda")   # int64 [E]
label = torch.randperm(n_edges, generator=torch.Generator().manual_seed(2))[:2000].to("cuda")          # the edges to predict
edge_label_index, edge_label_time = data.edge_index[:, label], data.time[label]

for strategy in ("uniform", "last"):
    loader = LinkNeighborLoader(data, [10, 5], edge_label_index=edge_label_index, edge_label_time=edge_label_time,
                                time_attr="time", temporal_strategy=strategy, time_window=(0, 50), neg_sampling_ratio=1,
                                batch_size=128, prefetch=4, seed=0, shuffle=True, unique=True)
    nodes = edges = pairs = 0
    ages = []
    for batch in loader:
        src, dst = batch.edge_label_index                    # [P] each: positions in n_id, positives first
        assert torch.equal(batch.batch[src], batch.batch[dst])                      # a pair lives in ONE subgraph ...
        assert torch.equal(batch.node_time[src], batch.edge_label_time)             # ... sampled under the pair's time
        E = batch.batch_size
        assert torch.equal(batch.n_id[src[:E]], edge_label_index[0][batch.input_id])
        assert torch.equal(batch.edge_label_time[:E], edge_label_time[batch.input_id])
        age = batch.node_time[batch.edge_index[1]] - batch.time                     # batch.time: the sampled edges' times
        assert bool((age >= 0).all()) and bool((age <= 50).all())                   # nothing from the future of its pair
        assert torch.equal(batch.batch[batch.edge_index[0]], batch.batch[batch.edge_index[1]])
        nodes += batch.num_nodes
        edges += batch.num_edges
        pairs += src.numel()
        ages.append(float(age.float().mean()) if batch.num_edges else 0.0)
    print("%s: %d mini-batches, %d pairs in disjoint subgraphs, %d nodes, %d edges, every edge before its pair's time, "
          "mean age %.2f" % (strategy, len(loader), pairs, nodes, edges, sum(ages) / len(ages)))
