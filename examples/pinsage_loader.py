"""PinSAGE-style importance sampling (DGL's PinSAGESampler): PinSAGELoader.  A node's neighbours are not drawn from its
own column: they are the few nodes that short random walks with termination from it visit most often, and the visit counts
weigh the messages.  A mini-batch is a list of blocks, outermost first; a layer aggregates a block's source rows into its
destination rows, which are the first n_dst rows of the source.  Plain torch, no torch_geometric."""
import torch

from _data import fake_dataset
from tch_geometric import PinSAGELoader

data = fake_dataset(num_nodes=20000, avg_degree=20)
loader = PinSAGELoader(data, [5, 5], input_nodes=torch.arange(2048), batch_size=512, n_walks=10, walk_length=2,
                       termination=0.5, prefetch=4, seed=0)


def layer(h, block):
    """a destination row plus the visit-count weighted mean of its sampled neighbours"""
    row, col = block.edge_index
    w = block.edge_weight.to(h.dtype)
    total = torch.zeros(block.n_dst, device=h.device).index_add(0, col, w)
    mean = torch.zeros(block.n_dst, h.shape[1], device=h.device).index_add(0, col, h[row] * w[:, None])
    return h[:block.n_dst] + mean / total.clamp(min=1)[:, None]


nodes = edges = 0
for batch in loader:
    h = batch.x                                              # one feature row per node of the outermost block
    assert h.shape[0] == batch.n_id.numel() == batch.blocks[0].num_src_nodes
    for block in batch.blocks:
        h = layer(h, block)
    assert h.shape[0] == batch.batch_size and bool(torch.isfinite(h).all())
    assert torch.equal(batch.n_id[:batch.batch_size], batch.input_nodes)
    nodes += batch.n_id.numel()
    edges += sum(b.num_edges for b in batch.blocks)
print("pinsage: %d mini-batches of %d seeds, %.1f distinct nodes and %.1f weighted edges per mini-batch, heaviest edge %d visits"
      % (len(loader), loader.batch_size, nodes / len(loader), edges / len(loader),
         max(int(b.edge_weight.max()) for b in batch.blocks)))
