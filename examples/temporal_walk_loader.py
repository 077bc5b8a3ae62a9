"""CTDNE-style embedding training: skip-gram over TEMPORAL walks (every step stays inside a time window that opens at the
walker's start time), with the sampling done by TemporalWalkLoader: one launch walks `prefetch` mini-batches, cuts the
walks into context windows, hands out the timestamp of every word beside it and draws the negatives.  Plain torch, no
torch_geometric."""
import torch

from _data import fake_temporal_dataset
from tch_geometric import TemporalWalkLoader

EPS = 1e-15
walk_length, context_size, walks_per_node, num_negative_samples = 20, 10, 4, 1    # walk_length counts columns here
window, max_gap = (0, 40), 25
data = fake_temporal_dataset()
# every node starts its walks when it was first seen; edges in [start, start + 40) are admissible
loader = TemporalWalkLoader(data, walk_length, context_size, window, walks_per_node=walks_per_node,
                            num_negative_samples=num_negative_samples, input_timestamps=data.node_time, batch_size=128,
                            prefetch=4, seed=0)
embedding = torch.nn.Embedding(data.num_nodes, 32, sparse=True).to("cuda")
optimizer = torch.optim.SparseAdam(list(embedding.parameters()), lr=0.01)


def scores(rw):
    """dot products of every window's first node with the rest of the window"""
    start, rest = rw[:, 0], rw[:, 1:]
    h = embedding(start).unsqueeze(1) * embedding(rest)
    return h.sum(-1).reshape(-1)


def skip_gram_loss(pos_rw, pos_ts, neg_rw):
    # keep the windows whose words lie close in time: from the first edge taken to the last one no more than max_gap
    # (column 0 of window 0 carries the walker's start time, the others the time of the edge that led to the word)
    ts = pos_ts[:, 1:]
    latest = ts.amax(1, keepdim=True)
    earliest = torch.where(ts >= 0, ts, latest).amin(1, keepdim=True)        # -1 = a word without a timestamp: ignored
    keep = (latest - earliest).squeeze(1) <= max_gap
    pos = -torch.log(torch.sigmoid(scores(pos_rw[keep])) + EPS).mean()
    neg = -torch.log(1 - torch.sigmoid(scores(neg_rw)) + EPS).mean()
    return pos + neg, float(keep.float().mean())


for epoch in range(2):
    total = kept = 0.0
    for batch in loader:
        optimizer.zero_grad()
        loss, frac = skip_gram_loss(batch.pos_rw, batch.pos_ts, batch.neg_rw)
        loss.backward()
        optimizer.step()
        total += float(loss)
        kept += frac
    print("epoch %d: %d mini-batches of up to %d seeds, windows %s (+ timestamps) + %s, %.0f%% of the windows span <= %d, "
          "last call id %d, loss %.4f" % (epoch, len(loader), loader.batch_size, tuple(batch.pos_rw.shape),
                                          tuple(batch.neg_rw.shape), 100 * kept / len(loader), max_gap, batch.call_id,
                                          total / len(loader)))
