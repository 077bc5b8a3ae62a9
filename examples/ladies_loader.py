"""Layer-wise importance sampling (FastGCN / LADIES): a two-layer model trained on LADIESLoader's blocks.  Every layer draws
ONE budget of nodes for the whole mini-batch, so a block has at most n_dst + budget sources however deep the model is; the
kept edges carry the rescaled adjacency entry, so the weighted sum over a destination's edges is an unbiased estimate of
the mean over all its in-neighbours.  Plain torch, no torch_geometric."""
import torch
import torch.nn.functional as F

from _data import fake_dataset
from tch_geometric import LADIESLoader

data = fake_dataset()
data.y = data.x[:, :10].argmax(1)            # labels a model can learn (the synthetic ones are noise)
N, C = data.num_nodes, data.x.shape[1]
BUDGETS = [256, 256]

torch.manual_seed(0)
shapes = ((C, 32), (C, 32), (32, 10), (32, 10))          # per layer: the node's own weights, its neighbours' weights
w = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.1) for s in shapes]
opt = torch.optim.Adam(w, lr=0.02)


def conv(h_src, block, w_self, w_nbr):
    """the first n_dst rows of h_src are the destinations: their own row plus the estimated mean of their in-neighbours"""
    row, col = block.edge_index
    est = torch.zeros((block.n_dst, h_src.shape[1]), device=h_src.device).index_add(0, col, h_src[row] * block.edge_weight[:, None])
    return h_src[:block.n_dst] @ w_self + est @ w_nbr


loader = LADIESLoader(data, BUDGETS, batch_size=250, prefetch=4, shuffle=True, seed=0)
losses, bounded, consistent, most = [], True, True, 0
for epoch in range(8):
    total = 0.0
    for batch in loader:                     # blocks come outermost first: blocks[0] reads batch.x
        outer, inner = batch.blocks
        h = F.relu(conv(batch.x, outer, w[0], w[1]))
        out = conv(h, inner, w[2], w[3])
        loss = F.cross_entropy(out, batch.y[:batch.batch_size])
        opt.zero_grad()
        loss.backward()
        opt.step()
        total += loss.item()
        for block, s in zip((inner, outer), BUDGETS):
            bounded &= block.num_src_nodes <= block.n_dst + s
            consistent &= bool((data.edge_index[:, block.e_id] == block.n_id[block.edge_index]).all())
        most = max(most, batch.num_nodes)
    losses.append(total / len(loader))
print("trained: %d epochs of %d layer-wise mini-batches, loss %.4f -> %.4f, fell: %s"
      % (len(losses), len(loader), losses[0], losses[-1], losses[-1] < losses[0]))
print("blocks: at most %d nodes per mini-batch of 250 seeds, bounded by the budgets: %s, e_id names the edges: %s"
      % (most, bounded, consistent))
