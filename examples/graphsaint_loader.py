"""GraphSAINT-style training (PyG's GraphSAINTRandomWalkSampler): every step trains on a SUBGRAPH -- the nodes that short
random walks from random roots visit, with every edge of the graph between them -- and corrects the sampler's bias with
the two normalisation vectors a pre-sample estimates: edge_norm weighs the messages, node_norm the loss.  A two-layer GCN
in plain torch, no torch_geometric."""
import torch
import torch.nn.functional as F

from _data import fake_dataset
from tch_geometric import GraphSAINTRandomWalkLoader

data = fake_dataset()
data.y = data.x[:, :10].argmax(1)            # labels a model can learn (the synthetic ones are noise)
loader = GraphSAINTRandomWalkLoader(data, batch_size=64, walk_length=2, num_steps=8, sample_coverage=20, prefetch=4, seed=0)
print("pre-sample: %d mini-batches in %d launches cover every node %d times on average; node_norm in [%.3g, %.3g]"
      % (loader.presampled_batches, loader.presampled_launches, loader.sample_coverage, float(loader.node_norm.min()),
         float(loader.node_norm.max())))

torch.manual_seed(0)
w1 = torch.nn.Parameter(torch.randn(data.x.shape[1], 32, device="cuda") * 0.1)
w2 = torch.nn.Parameter(torch.randn(32, 10, device="cuda") * 0.1)
opt = torch.optim.Adam([w1, w2], lr=0.02)


def conv(h, edge_index, weight):
    """the node itself plus the weighted mean of its in-neighbours inside the subgraph"""
    row, col = edge_index
    total = torch.zeros(h.shape[0], device=h.device).index_add(0, col, weight)
    mean = torch.zeros_like(h).index_add(0, col, h[row] * weight[:, None]) / total.clamp(min=1e-6)[:, None]
    return h + mean


losses = []
for epoch in range(8):
    total = nodes = 0
    for batch in loader:
        h = F.relu(conv(batch.x @ w1, batch.edge_index, batch.edge_norm))
        out = conv(h @ w2, batch.edge_index, batch.edge_norm)
        loss = (F.cross_entropy(out, batch.y, reduction="none") * batch.node_norm).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        total += loss.item()
        nodes += batch.num_nodes
    losses.append(total / len(loader))
print("trained: %d epochs of %d subgraphs of about %d nodes, normalised loss %.4f -> %.4f, fell: %s"
      % (len(losses), len(loader), nodes // len(loader), losses[0], losses[-1], losses[-1] < losses[0]))
