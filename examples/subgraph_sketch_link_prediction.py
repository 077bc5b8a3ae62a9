"""ELPH / BUDDY's structure features as a link predictor: held-out edges of a synthetic graph with planted communities are
scored against random non-links by a logistic regression on `structure` alone -- the estimated numbers of vertices at every
pair of distances from the two ends, from MinHash / HyperLogLog sketches (SketchData, SubgraphSketchLoader over
tg_sketch_links) -- beside the exact common-neighbour count of CommonNeighborLoader; the mean relative error of the
intersection estimates I[a][b] against exact ball intersections on 256 links is printed too.  Plain torch, no
torch_geometric."""
import torch

from _data import fake_community_dataset
from tch_geometric import CommonNeighborLoader, SketchData, SubgraphSketchLoader

H = 2
data = fake_community_dataset()
gen = torch.Generator().manual_seed(1)
E, N = data.edge_index.shape[1], data.num_nodes
held = torch.zeros(E, dtype=torch.bool, device="cuda")
held[torch.randperm(E, generator=gen)[:1024].to("cuda")] = True
pos = data.edge_index[:, held]
pos = pos[:, pos[0] != pos[1]]
kept = data.edge_index[:, ~held]
data.edge_index = torch.cat([kept, kept.flip(0)], 1)                        # symmetric: the undirected notion
neg = torch.randint(0, N, (2, pos.shape[1]), generator=gen).to("cuda")
links = torch.cat([pos, neg], 1)
labels = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to("cuda")

sketches = SketchData(data, hops=H)
batches = list(SubgraphSketchLoader(sketches, links, labels, batch_size=256, prefetch=4))
x = torch.log1p(torch.cat([b.structure for b in batches]).clamp(min=0))
cn = torch.cat([b.scores["cn"] for b in CommonNeighborLoader(data, links, labels, scores=("cn",), batch_size=256, truncate=True)])


def auc(s, y):
    """the probability that a positive link outscores a negative one, ties counting half"""
    p, n = s[y > 0].double(), s[y == 0].double()
    return float(((p[:, None] > n[None, :]).double().mean() + 0.5 * (p[:, None] == n[None, :]).double().mean()))


train = torch.rand(links.shape[1], generator=gen).to("cuda") < 0.5          # fit on one half of the links, score the other
w = torch.zeros(x.shape[1] + 1, device="cuda", requires_grad=True)
opt = torch.optim.Adam([w], lr=0.05)
for _ in range(300):
    opt.zero_grad()
    torch.nn.functional.binary_cross_entropy_with_logits(x[train] @ w[:-1] + w[-1], labels[train]).backward()
    opt.step()
score = (x @ w[:-1] + w[-1]).detach()

# exact closed balls by boolean matrix powers (1 000 vertices), against I[a][b] = match / n_perm x card(usum, uzero)
from tch_geometric._cabi_sketch import cardinality  # noqa: E402
adj = torch.eye(N, device="cuda")
adj[data.edge_index[1], data.edge_index[0]] = 1.0
balls = [adj]
for _ in range(H - 1):
    balls.append(((balls[-1] @ adj) > 0).float())
u, v = links[0, :256], links[1, :256]
raw = batches[0]
est = raw.match.float() / sketches.n_perm * cardinality(raw.usum, raw.uzero, sketches.sizes.m_reg)
exact = torch.stack([torch.stack([(balls[a][u] * balls[b][v]).sum(1) for b in range(H)], 1) for a in range(H)], 1)
err = ((est - exact).abs() / exact.clamp(min=1)).mean()

print("subgraph sketches: %d links, AUC structure %.4f, AUC cn %.4f, mean relative error of I %.4f"
      % (links.shape[1], auc(score[~train], labels[~train]), auc(cn[~train], labels[~train]), float(err)))
