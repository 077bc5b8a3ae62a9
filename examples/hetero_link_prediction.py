"""Link prediction on a typed graph over HeteroLinkNeighborLoader: the labelled relation (v0, e0, v1) joins two node types;
a mini-batch is 256 of its edges, one checked negative each (a random v0 with a random v1), and the two-hop typed
neighbourhood of all their endpoints.  A mean-aggregating encoder with one weight per node type and per relation embeds
the mini-batch's nodes and a dot product scores the (v0, v1) pairs named by edge_label_index, whose two rows are numbered
against the n_id of v0 and of v1.  Plain torch, no torch_geometric."""
import torch
import torch.nn.functional as F

from _data import fake_hetero_dataset
from tch_geometric import HeteroLinkNeighborLoader

data = fake_hetero_dataset()
REL = ("v0", "e0", "v1")
loader = HeteroLinkNeighborLoader(data, [10, 5], REL, neg_sampling_ratio=1, neg_sampling="binary", try_count=8,
                                  batch_size=256, prefetch=8, shuffle=True, unique=True, seed=0)


class Layer(torch.nn.Module):
    """h'[t][v] = W_t h[t][v] + sum over relations (s, r, t) of W_r mean(h[s][u] for sampled edges u -> v)"""

    def __init__(self, node_types, edge_types, channels, hidden):
        super().__init__()
        self.own = torch.nn.ModuleDict({t: torch.nn.Linear(channels, hidden) for t in node_types})
        self.rel = torch.nn.ModuleDict({"__".join(et): torch.nn.Linear(channels, hidden) for et in edge_types})

    def forward(self, h, edges):
        out = {t: lin(h[t]) for t, lin in self.own.items()}
        for et, (src, dst) in edges.items():
            total = torch.zeros_like(h[et[2]]).index_add_(0, dst, h[et[0]][src])
            degree = torch.zeros(h[et[2]].shape[0], device=dst.device).index_add_(0, dst, torch.ones_like(dst, dtype=total.dtype))
            out[et[2]] = out[et[2]] + self.rel["__".join(et)](total / degree.clamp(min=1).unsqueeze(1))
        return out


class Encoder(torch.nn.Module):
    def __init__(self, node_types, edge_types, channels, hidden):
        super().__init__()
        self.l1, self.l2 = Layer(node_types, edge_types, channels, hidden), Layer(node_types, edge_types, hidden, hidden)

    def forward(self, x, edges):
        return self.l2({t: F.relu(v) for t, v in self.l1(x, edges).items()}, edges)


model = Encoder(data.node_types, data.edge_types, data["v0"].x.shape[1], 32).to("cuda")
optimizer = torch.optim.Adam(model.parameters(), lr=0.01)
for epoch in range(2):
    total, unverified = 0.0, torch.zeros((), dtype=torch.int64, device="cuda")
    for batch in loader:
        optimizer.zero_grad()
        h = model({t: batch[t].x for t in data.node_types}, {et: batch[et].edge_index for et in data.edge_types})
        src, dst = batch[REL].edge_label_index            # row 0 indexes batch["v0"].n_id, row 1 batch["v1"].n_id
        loss = F.binary_cross_entropy_with_logits((h["v0"][src] * h["v1"][dst]).sum(-1), batch[REL].edge_label)
        loss.backward()
        optimizer.step()
        total += float(loss)
        unverified += batch.neg_unverified
    print("epoch %d: %d mini-batches of up to %d positive edges, last one %s nodes, %d + %d unique seeds, call id %d, "
          "%d unverified negatives, loss %.4f" % (epoch, len(loader), loader.batch_size,
                                                 {t: batch[t].num_nodes for t in data.node_types}, batch["v0"].batch_size,
                                                 batch["v1"].batch_size, batch.call_id, int(unverified), total / len(loader)))
