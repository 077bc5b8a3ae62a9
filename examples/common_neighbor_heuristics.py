"""The classical link heuristics -- common neighbours, Jaccard, Adamic-Adar, resource allocation -- as link predictors: held-out
edges of a synthetic graph with planted communities are scored against random non-links from the per-link common neighbours
the device finds (CommonNeighborLoader over tg_cn_links), and each heuristic's AUC is printed.  There is no training.  Plain
torch, no torch_geometric."""
import torch

from _data import fake_community_dataset
from tch_geometric import CommonNeighborLoader

data = fake_community_dataset()
gen = torch.Generator().manual_seed(1)
E = data.edge_index.shape[1]
held = torch.zeros(E, dtype=torch.bool, device="cuda")
held[torch.randperm(E, generator=gen)[:512].to("cuda")] = True
pos = data.edge_index[:, held]
pos = pos[:, pos[0] != pos[1]]
kept = data.edge_index[:, ~held]
data.edge_index = torch.cat([kept, kept.flip(0)], 1)                        # symmetric: the undirected notion
neg = torch.randint(0, data.num_nodes, (2, pos.shape[1]), generator=gen).to("cuda")
links = torch.cat([pos, neg], 1)
labels = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to("cuda")
loader = CommonNeighborLoader(data, links, labels, cn_cap=64, batch_size=128, prefetch=4, truncate=True)

scores, listed = {name: [] for name in loader.scores}, 0
for batch in loader:
    for name, s in batch.scores.items():
        scores[name].append(s)
    listed += batch.cn_index.numel()
    assert batch.x.shape[0] == batch.cn_index.numel()                       # the common neighbours' features ride along


def auc(s, y):
    """the probability that a positive link outscores a negative one, ties counting half"""
    p, n = s[y > 0].double(), s[y == 0].double()
    return float(((p[:, None] > n[None, :]).double().mean() + 0.5 * (p[:, None] == n[None, :]).double().mean()))


print("common neighbours: %d links, %d listed neighbours, " % (links.shape[1], listed)
      + ", ".join("AUC %s %.4f" % (name, auc(torch.cat(parts), labels)) for name, parts in scores.items()))
