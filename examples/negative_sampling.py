"""The reference's examples/negative_sampling.py on this backend: negatives for every node through
NegativeSamplerTransform (one call), then the same stream of mini-batches through NegativeLoader (many mini-batches per
launch), homogeneous and heterogeneous."""
import torch

from _data import fake_dataset, fake_hetero_dataset
import tch_geometric as thg
from tch_geometric.loader import NegativeLoader
from tch_geometric.transforms import NegativeSamplerTransform

num_neg, try_count = 5, 5
data = fake_dataset()
inputs = torch.arange(data.num_nodes, device="cuda")

thg.seed(0)
transform = NegativeSamplerTransform(data, num_neg, try_count, inbound=False)
batch = transform(inputs)
print("transform: %d nodes, %d negative edges, x %s" % (batch.num_nodes, batch.neg_edge_index.shape[1], tuple(batch.x.shape)))

loader = NegativeLoader(data, num_neg, try_count, input_nodes=inputs, batch_size=128, prefetch=4, seed=0)
edges = 0
for mini in loader:
    src, dst = mini.n_id[mini.neg_edge_index[0]], mini.n_id[mini.neg_edge_index[1]]
    assert bool((src != dst).all()) and mini.x.shape[0] == mini.num_nodes
    edges += int(src.numel())
print("loader: %d mini-batches of up to %d inputs, %d negative edges, call ids %d..%d" % (
    len(loader), loader.batch_size, edges, loader.call_id0, mini.call_id))

# the first mini-batch again through the transform, at the loader's (seed, call id): the same draw
thg.set_rng_state(0, loader.call_id0)
again = transform(inputs[:128])
first = next(iter(NegativeLoader(data, num_neg, try_count, input_nodes=inputs, batch_size=128, prefetch=4, seed=0)))
print("loader mini-batch 0 == transform at its call id:", bool(torch.equal(first.neg_edge_index, again.neg_edge_index)))

hetero = fake_hetero_dataset()
nt = hetero.node_types[0]
hloader = NegativeLoader(hetero, num_neg, try_count, input_type=nt, batch_size=128, prefetch=4, seed=0)
mini = next(iter(hloader))
print("hetero loader: %d mini-batches of type %s; first: %s" % (
    len(hloader), nt, {"__".join(et): int(mini[et].neg_edge_index.shape[1]) for et in hetero.edge_types}))
