"""Link prediction over LinkNeighborLoader: a mini-batch is 256 positive edges, one checked negative each, and the two-hop
neighbourhood of all their endpoints; a mean-aggregating encoder embeds the mini-batch's nodes from their features and a
dot product scores the (source, destination) pairs named by edge_label_index.  Plain torch, no torch_geometric."""
import torch
import torch.nn.functional as F

from _data import fake_dataset
from tch_geometric import LinkNeighborLoader

data = fake_dataset()
loader = LinkNeighborLoader(data, [10, 5], neg_sampling_ratio=1, neg_sampling="binary", try_count=8, batch_size=256,
                            prefetch=8, shuffle=True, unique=True, seed=0)


class Encoder(torch.nn.Module):
    """two rounds of h[v] = W_self x[v] + W_nbr mean(x[u] for sampled edges u -> v)"""

    def __init__(self, channels, hidden):
        super().__init__()
        self.self1, self.nbr1 = torch.nn.Linear(channels, hidden), torch.nn.Linear(channels, hidden)
        self.self2, self.nbr2 = torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, hidden)

    @staticmethod
    def mean_of_neighbours(h, edge_index):
        src, dst = edge_index
        total = torch.zeros_like(h).index_add_(0, dst, h[src])
        degree = torch.zeros(h.shape[0], device=h.device).index_add_(0, dst, torch.ones_like(dst, dtype=h.dtype))
        return total / degree.clamp(min=1).unsqueeze(1)

    def forward(self, x, edge_index):
        h = F.relu(self.self1(x) + self.nbr1(self.mean_of_neighbours(x, edge_index)))
        return self.self2(h) + self.nbr2(self.mean_of_neighbours(h, edge_index))


model = Encoder(data.x.shape[1], 32).to("cuda")
optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
for epoch in range(2):
    total, unverified = 0.0, torch.zeros((), dtype=torch.int64, device="cuda")
    for batch in loader:
        optimizer.zero_grad()
        h = model(batch.x, batch.edge_index)
        src, dst = batch.edge_label_index                 # numbered against batch.n_id, like batch.edge_index
        loss = F.binary_cross_entropy_with_logits((h[src] * h[dst]).sum(-1), batch.edge_label)
        loss.backward()
        optimizer.step()
        total += float(loss)
        unverified += batch.neg_unverified
    print("epoch %d: %d mini-batches of up to %d positive edges, last one %d nodes / %d sampled edges, call id %d, "
          "%d unverified negatives, loss %.4f" % (epoch, len(loader), loader.batch_size, batch.num_nodes, batch.num_edges,
                                                 batch.call_id, int(unverified), total / len(loader)))
