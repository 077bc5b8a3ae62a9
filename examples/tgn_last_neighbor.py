"""The train loop of the memory-based temporal GNNs (TGN, Rossi et al. 2020) without the memory: for every mini-batch of a
chronological event list, look up the most recent interactions of its nodes in the state BEFORE the batch, score the events
against negatives with one attention layer over (n_id, edge_index, t[e_id]), then insert the batch.  TemporalEventLoader does
the lookups and inserts of `prefetch` mini-batches in one launch chain.  Plain torch, no torch_geometric."""
import math

import torch
import torch.nn.functional as F

import _data  # noqa: F401  (puts the package on the path)
from tch_geometric import TemporalEventLoader

N, E, D, SIZE, GROUPS = 600, 6000, 32, 10, 6
g = torch.Generator().manual_seed(0)
src = torch.randint(0, N, (E,), generator=g)
dst = (src % GROUPS + GROUPS * torch.randint(0, N // GROUPS, (E,), generator=g)) % N    # events stay inside a group of nodes
t = torch.sort(torch.randint(0, 10000, (E,), generator=g)).values

torch.manual_seed(0)
emb = torch.nn.Parameter(torch.randn(N, D, device="cuda") * 0.1)
wq, wk, wv = (torch.nn.Parameter(torch.randn(D, D, device="cuda") / math.sqrt(D)) for _ in range(3))
freq = torch.nn.Parameter(torch.logspace(0, -4, D, device="cuda"))
opt = torch.optim.Adam([emb, wq, wk, wv, freq], lr=0.01)
t_dev = t.cuda()


def embed(batch):
    """one attention layer: a node attends over its last interactions, keyed by the neighbour and the time since"""
    z0 = emb[batch.n_id]
    nbr, query = batch.edge_index
    since = (batch.t[0] - t_dev[batch.e_id]).float()
    msg = z0[nbr] + torch.cos(since[:, None] * freq[None, :])
    score = ((msg @ wk) * (z0[query] @ wq)).sum(-1) / math.sqrt(D)
    a = torch.exp(score - score.max()) if score.numel() else score
    denom = torch.zeros(z0.shape[0], device=a.device).index_add(0, query, a)
    att = a / denom[query]
    return z0 + torch.zeros_like(z0).index_add(0, query, att[:, None] * (msg @ wv))


loader = TemporalEventLoader(src, dst, t, N, SIZE, batch_size=200, prefetch=8, seed=0)
losses, causal, edges = [], True, 0
for epoch in range(4):
    total = 0.0
    for batch in loader:
        z = embed(batch)
        pos = (z[batch.src_index] * z[batch.dst_index]).sum(-1)
        neg = (z[batch.src_index] * z[batch.neg_index]).sum(-1)
        loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
        opt.zero_grad()
        loss.backward()
        opt.step()
        total += loss.item()
        causal &= batch.e_id.numel() == 0 or int(batch.e_id.max()) < int(batch.input_id[0])
        edges += batch.e_id.numel()
    losses.append(total / len(loader))
print("trained: %d epochs of %d event mini-batches, loss %.4f -> %.4f, fell: %s"
      % (len(losses), len(loader), losses[0], losses[-1], losses[-1] < losses[0]))
print("lookups: %d neighbour entries, none from the mini-batch itself or later: %s" % (edges, causal))
