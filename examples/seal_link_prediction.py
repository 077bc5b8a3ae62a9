"""SEAL link prediction (Zhang and Chen 2018; PyG's examples/seal_link_pred.py): every candidate link gets its 1-hop enclosing
subgraph with double-radius node labels from the device, one epoch of positive and random negative links trains a small GCN
over label embeddings + features, pooled at the two roots.  `target_edge` masks the link itself out of the positive
subgraphs, so the model cannot read the answer off the graph.  Plain torch, no torch_geometric.

--max-nodes-per-hop K (SEAL-OGB's cap; 0 = the exhaustive default run): two-hop subgraphs whose hops keep K random new
vertices at most; three quarters of the links train for EPOCHS epochs, the rest are scored for a test AUC on a second line."""
import argparse

import torch
import torch.nn.functional as F

from _data import fake_dataset
from tch_geometric import SEALLoader

parser = argparse.ArgumentParser()
parser.add_argument("--max-nodes-per-hop", type=int, default=0)
K = parser.parse_args().max_nodes_per_hop
Z_MAX, HIDDEN, EPOCHS = 8, 32, 8 if K else 1
data = fake_dataset(avg_degree=3)
data.edge_index = torch.cat([data.edge_index, data.edge_index.flip(0)], 1)   # symmetric: SEAL's undirected subgraphs
gen = torch.Generator().manual_seed(1)
E = data.edge_index.shape[1]
pos = data.edge_index[:, torch.randperm(E // 2, generator=gen)[:512].to("cuda")]
pos = pos[:, pos[0] != pos[1]]
neg = torch.randint(0, data.num_nodes, (2, pos.shape[1]), generator=gen).to("cuda")   # negative links are the caller's
neg = neg[:, neg[0] != neg[1]]
links = torch.cat([pos, neg], 1)
labels = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to("cuda")
loader = SEALLoader(data, links, labels, num_hops=1, node_cap=256, z_max=Z_MAX, batch_size=64, prefetch=4, shuffle=True)
held, scores = [], []
if K:
    order = torch.randperm(links.shape[1], generator=gen).to("cuda")
    test, train = order[:links.shape[1] // 4], order[links.shape[1] // 4:]
    capped = dict(num_hops=2, node_cap=256, z_max=Z_MAX, batch_size=64, max_nodes_per_hop=K)
    held = SEALLoader(data, links[:, test].contiguous(), labels[test], resample=False, **capped)
    links = links[:, train].contiguous()
    loader = SEALLoader(data, links, labels[train], shuffle=True, **capped)

torch.manual_seed(0)
embed = torch.nn.Embedding(Z_MAX + 1, HIDDEN).to("cuda")
lin_x = torch.nn.Linear(data.x.shape[1], HIDDEN).to("cuda")
conv = torch.nn.Linear(HIDDEN, HIDDEN).to("cuda")
head = torch.nn.Linear(2 * HIDDEN, 1).to("cuda")
params = [p for mod in (embed, lin_x, conv, head) for p in mod.parameters()]
opt = torch.optim.Adam(params, lr=0.01)

hist = torch.zeros(Z_MAX + 1, dtype=torch.int64, device="cuda")
nodes = edges = masked = 0
loss_sum = 0.0
for step, batch in enumerate(b for part in [loader] * EPOCHS + [held] for b in part):
    row, col = batch.edge_index
    keep = ~(batch.target_edge & (batch.edge_label[batch.batch[col]] > 0))     # a positive link's own edges are masked
    row, col = row[keep], col[keep]
    h = embed(batch.z) + lin_x(batch.x)
    deg = torch.zeros(batch.num_nodes, device="cuda").index_add_(0, col, torch.ones(col.numel(), device="cuda")) + 1.0
    agg = torch.zeros_like(h).index_add_(0, col, h[row])
    h = F.relu(conv((h + agg) / deg[:, None]))
    logit = head(h[batch.root_n_id].reshape(batch.batch_size, -1)).squeeze(1)  # the two roots of every link
    if step >= EPOCHS * len(loader):           # a held-out mini-batch is scored, not trained on
        scores.append((logit.detach(), batch.edge_label > 0))
        continue
    loss = F.binary_cross_entropy_with_logits(logit, batch.edge_label)
    opt.zero_grad()
    loss.backward()
    opt.step()
    hist += torch.bincount(batch.z, minlength=Z_MAX + 1)
    nodes, edges, masked = nodes + batch.num_nodes, edges + batch.num_edges, masked + int((~keep).sum())
    loss_sum += float(loss)
print("seal: %d links in %d mini-batches, %d nodes, %d induced edges, %d target edges masked, mean loss %.4f, z histogram %s"
      % (links.shape[1], EPOCHS * len(loader), nodes, edges, masked, loss_sum / (EPOCHS * len(loader)), hist.tolist()))
if K:
    score, truth = (torch.cat(t) for t in zip(*scores))
    wins = (score[truth][:, None] > score[~truth][None, :]).float() + 0.5 * (score[truth][:, None] == score[~truth][None, :])
    print("seal: max_nodes_per_hop %d, %d held-out links, test AUC %.4f" % (K, truth.numel(), float(wins.mean())))
