"""MetaPath2Vec training as PyG's MetaPath2Vec sets it up (walks along a metapath of a typed graph, negative rows per column
type, the skip-gram loss over context windows, ONE embedding table for all node types), with the sampling done by
MetaPath2VecLoader: one launch walks `prefetch` mini-batches, cuts the walks into context windows, draws the negatives and
adds every column's type offset.  Plain torch, no torch_geometric."""
import torch

from _data import fake_hetero_dataset
from tch_geometric import MetaPath2VecLoader

EPS = 1e-15
walk_length, context_size, walks_per_node, num_negative_samples = 20, 10, 4, 1
data = fake_hetero_dataset()
metapath = [("v0", "e0", "v1"), ("v1", "e1", "v0")]      # v0 -> v1 -> v0: a closed path, repeated along the walk
loader = MetaPath2VecLoader(data, metapath, walk_length - 1, context_size, walks_per_node=walks_per_node,
                            num_negative_samples=num_negative_samples, batch_size=128, prefetch=4, seed=0)
# rows [start[t], end[t]) of the table belong to node type t; row dummy_idx stands for "the walk had ended"
embedding = torch.nn.Embedding(loader.num_embeddings, 32, sparse=True).to("cuda")
optimizer = torch.optim.SparseAdam(list(embedding.parameters()), lr=0.01)


def scores(rw):
    """dot products of every window's first node with the rest of the window"""
    start, rest = rw[:, 0], rw[:, 1:]
    h = embedding(start).unsqueeze(1) * embedding(rest)
    return h.sum(-1).reshape(-1)


def skip_gram_loss(pos_rw, neg_rw):
    pos_rw = pos_rw[(pos_rw != loader.dummy_idx).all(1)]   # windows of a walk that had ended carry dummy_idx
    pos = -torch.log(torch.sigmoid(scores(pos_rw)) + EPS).mean()
    neg = -torch.log(1 - torch.sigmoid(scores(neg_rw)) + EPS).mean()
    return pos + neg


for epoch in range(3):
    total = 0.0
    for batch in loader:
        optimizer.zero_grad()
        loss = skip_gram_loss(batch.pos_rw, batch.neg_rw)
        loss.backward()
        optimizer.step()
        total += float(loss)
    print("epoch %d: %d mini-batches of up to %d seeds, windows %s + %s, %d table rows, last call id %d, loss %.4f" % (
        epoch, len(loader), loader.batch_size, tuple(batch.pos_rw.shape), tuple(batch.neg_rw.shape), loader.num_embeddings,
        batch.call_id, total / len(loader)))
