"""ShaDow-GNN with its PPR sampler (also PPRGo's neighbourhoods): every seed gets the k vertices of largest approximate
personalised PageRank from it -- a forward push on the device, in integers -- and the mini-batch holds every edge of the
graph inside each neighbourhood.  `ppr` carries every node's estimate from its own seed: PPRGo's aggregation weights.  Plain
torch, no torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric import PPRLoader

data = fake_dataset()
input_nodes = torch.arange(data.num_nodes, device="cuda")
loader = PPRLoader(data, k=16, alpha=0.15, eps=1e-4, input_nodes=input_nodes, batch_size=128, prefetch=4)
nodes = edges = seen = 0
shared = True
for batch in loader:
    row, col = batch.edge_index
    shared &= bool((batch.batch[row] == batch.batch[col]).all())             # an edge never leaves its seed's subgraph
    assert torch.equal(batch.batch[batch.root_n_id], torch.arange(batch.batch_size, device="cuda"))
    assert torch.equal(batch.n_id[batch.root_n_id], input_nodes[seen:seen + batch.batch_size])   # every seed's own entry
    seen += batch.batch_size
    pooled = torch.zeros(batch.batch_size, batch.x.shape[1], device="cuda")
    pooled.index_add_(0, batch.batch, batch.ppr[:, None] * batch.x)           # PPRGo: the ppr-weighted sum per seed
    assert pooled.shape[0] == batch.batch_size and bool((batch.ppr >= 0).all()) and bool((batch.ppr <= 1).all())
    nodes += batch.num_nodes
    edges += batch.num_edges
print("ppr: %d mini-batches of up to %d subgraphs of at most %d nodes, %d nodes, %d induced edges, both ends of every edge share "
      "batch: %s" % (len(loader), loader.batch_size, loader.k, nodes, edges, shared))
