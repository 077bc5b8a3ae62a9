"""GraphSAINT's node and edge samplers (PyG's GraphSAINTNodeSampler / GraphSAINTEdgeSampler) beside the random-walk one of
graphsaint_loader.py: the same subgraph mini-batches and the same two normalisation vectors, from a node list that is drawn
differently -- nodes by out-degree, or the ends of edges drawn with probability ~ 1/deg(u) + 1/deg(v) (the sampler the
paper recommends).  One epoch each on the synthetic graph, with the norms applied as a trainer would."""
import torch

from _data import fake_dataset
from tch_geometric import GraphSAINTEdgeLoader, GraphSAINTNodeLoader

data = fake_dataset()
for name, loader in (
        ("node", GraphSAINTNodeLoader(data, batch_size=200, num_steps=6, sample_coverage=20, prefetch=4, seed=0)),
        ("edge", GraphSAINTEdgeLoader(data, batch_size=120, num_steps=6, sample_coverage=20, prefetch=4, seed=0))):
    nodes = edges = 0
    weight = 0.0
    for batch in loader:
        assert batch.x.shape[0] == batch.num_nodes == batch.node_norm.numel()
        assert batch.edge_index.shape[1] == batch.num_edges == batch.edge_norm.numel()
        src, dst = batch.n_id[batch.edge_index]                         # the induced edges are edges of the graph
        assert torch.equal(torch.stack([src, dst]), data.edge_index[:, batch.e_id])
        nodes += batch.num_nodes
        edges += batch.num_edges
        weight += float(batch.node_norm.sum())                         # an unbiased estimate of 1 per mini-batch
    print("%s sampler: %d draws -> %d nodes and %d edges per mini-batch; pre-sample of %d mini-batches, "
          "sum of node_norm per mini-batch %.3f"
          % (name, loader.batch_size, nodes // len(loader), edges // len(loader), loader.presampled_batches,
             weight / len(loader)))
