"""Node2Vec training as the reference's examples/random_walk.py sets it up (positive walks, negative rows, the skip-gram
loss over context windows), with the sampling done by Node2VecLoader: one launch walks `prefetch` mini-batches, cuts the
walks into context windows and draws the negatives.  Plain torch, no torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric import Node2VecLoader

EPS = 1e-15
walk_length, context_size, walks_per_node, num_negative_samples, p, q = 20, 10, 4, 1, 1.0, 1.5
data = fake_dataset()
loader = Node2VecLoader(data, walk_length - 1, context_size, walks_per_node=walks_per_node,
                        num_negative_samples=num_negative_samples, p=p, q=q, batch_size=128, prefetch=4, seed=0)
embedding = torch.nn.Embedding(data.num_nodes, 32, sparse=True).to("cuda")
optimizer = torch.optim.SparseAdam(list(embedding.parameters()), lr=0.01)


def scores(rw):
    """dot products of every window's first node with the rest of the window"""
    start, rest = rw[:, 0], rw[:, 1:]
    h = embedding(start).unsqueeze(1) * embedding(rest)
    return h.sum(-1).reshape(-1)


def skip_gram_loss(pos_rw, neg_rw):
    pos_rw = pos_rw[(pos_rw >= 0).all(1)]                # windows of a walk that met a dead end carry its -1 padding
    pos = -torch.log(torch.sigmoid(scores(pos_rw)) + EPS).mean()
    neg = -torch.log(1 - torch.sigmoid(scores(neg_rw)) + EPS).mean()
    return pos + neg


for epoch in range(2):
    total = 0.0
    for batch in loader:
        optimizer.zero_grad()
        loss = skip_gram_loss(batch.pos_rw, batch.neg_rw)
        loss.backward()
        optimizer.step()
        total += float(loss)
    print("epoch %d: %d mini-batches of up to %d seeds, windows %s + %s, last call id %d, loss %.4f" % (
        epoch, len(loader), loader.batch_size, tuple(batch.pos_rw.shape), tuple(batch.neg_rw.shape), batch.call_id,
        total / len(loader)))
