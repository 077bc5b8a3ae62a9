"""Cluster-GCN-style training (PyG's ClusterData / ClusterLoader): the nodes are partitioned once, every step trains on the
union of a few clusters with every edge of the graph between its nodes.  The partition here is range_partition, a stand-in
that knows nothing about the edges: with a real partitioner (METIS through pymetis or torch-sparse, or a saved file) pass its
cluster vector as `part` instead.  A two-layer GCN in plain torch, no torch_geometric."""
import torch
import torch.nn.functional as F

from _data import fake_dataset
from tch_geometric import ClusterData, ClusterLoader, range_partition

data = fake_dataset()
data.y = data.x[:, :10].argmax(1)            # labels a model can learn (the synthetic ones are noise)
N, E = data.num_nodes, data.edge_index.shape[1]
cluster_data = ClusterData(data, range_partition(N, 32), num_parts=32)
loader = ClusterLoader(cluster_data, batch_size=4, shuffle=True, prefetch=4, seed=0)
kept = sum(batch.num_edges for batch in loader)
print("partition: %d clusters of about %d nodes, %d per mini-batch; an epoch keeps %d of %d edges (%.0f%%)"
      % (len(cluster_data), N // len(cluster_data), loader.batch_size, kept, E, 100.0 * kept / E))

torch.manual_seed(0)
w1 = torch.nn.Parameter(torch.randn(data.x.shape[1], 32, device="cuda") * 0.1)
w2 = torch.nn.Parameter(torch.randn(32, 10, device="cuda") * 0.1)
opt = torch.optim.Adam([w1, w2], lr=0.02)


def conv(h, edge_index):
    """the node itself plus the mean of its in-neighbours inside the subgraph"""
    row, col = edge_index
    deg = torch.zeros(h.shape[0], device=h.device).index_add(0, col, torch.ones(col.numel(), device=h.device))
    return h + torch.zeros_like(h).index_add(0, col, h[row]) / deg.clamp(min=1)[:, None]


losses = []
for epoch in range(8):
    total = nodes = 0
    for batch in loader:
        out = conv(F.relu(conv(batch.x @ w1, batch.edge_index)) @ w2, batch.edge_index)
        loss = F.cross_entropy(out, batch.y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        total += loss.item()
        nodes += batch.num_nodes
    assert nodes == N                         # an epoch visits every cluster, so every node, once
    losses.append(total / len(loader))
print("trained: %d epochs of %d subgraphs of about %d nodes, loss %.4f -> %.4f, fell: %s"
      % (len(losses), len(loader), N // len(loader), losses[0], losses[-1], losses[-1] < losses[0]))
