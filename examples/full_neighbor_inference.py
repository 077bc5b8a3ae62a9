"""Train on samples, infer on everything (the end of every PyG / DGL node-classification script): a two-layer
mean-aggregation model is trained with NeighborLoader on sampled neighbourhoods, then evaluated layer by layer over ALL nodes
with ALL their neighbours through FullNeighborLoader(num_layers=1) -- PyG's model.inference(x_all, subgraph_loader) with
NeighborLoader(num_neighbors=[-1]), DGL's MultiLayerFullNeighborSampler(1).  Plain torch, no torch_geometric."""
import torch
import torch.nn.functional as F

from _data import fake_dataset
from tch_geometric import FullNeighborLoader
from tch_geometric.loader import NeighborLoader

data = fake_dataset()
data.y = data.x[:, :10].argmax(1)            # labels a model can learn (the synthetic ones are noise)
N, C = data.num_nodes, data.x.shape[1]

torch.manual_seed(0)
shapes = ((C, 32), (C, 32), (32, 10), (32, 10))          # per layer: the node's own weights, its neighbours' weights
w = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.1) for s in shapes]
opt = torch.optim.Adam(w, lr=0.02)


def conv(h_src, edge_index, n_dst, w_self, w_nbr):
    """the first n_dst rows of h_src are the destinations: their own row plus the mean of their in-neighbours' rows"""
    row, col = edge_index
    ones = torch.ones(col.numel(), device=h_src.device)
    deg = torch.zeros(n_dst, device=h_src.device).index_add(0, col, ones)
    mean = torch.zeros((n_dst, h_src.shape[1]), device=h_src.device).index_add(0, col, h_src[row]) / deg.clamp(min=1)[:, None]
    return h_src[:n_dst] @ w_self + mean @ w_nbr


train = NeighborLoader(data, [10, 10], batch_size=250, prefetch=4, shuffle=True, seed=0, unique=True)
losses = []
for epoch in range(8):
    total = 0.0
    for batch in train:                      # the seeds lead n_id; both layers run over the sampled subgraph
        n = batch.num_nodes
        h = F.relu(conv(batch.x, batch.edge_index, n, w[0], w[1]))
        out = conv(h, batch.edge_index, n, w[2], w[3])[:batch.batch_size]
        loss = F.cross_entropy(out, batch.y[:batch.batch_size])
        opt.zero_grad()
        loss.backward()
        opt.step()
        total += loss.item()
    losses.append(total / len(train))
print("trained: %d epochs of %d sampled mini-batches, loss %.4f -> %.4f, fell: %s"
      % (len(losses), len(train), losses[0], losses[-1], losses[-1] < losses[0]))

# layer-wise inference: layer l of ALL nodes before layer l + 1 of any, every node with its full neighbourhood
loader = FullNeighborLoader(data, num_layers=1, batch_size=128, prefetch=4)
seen = torch.zeros(N, dtype=torch.int64, device="cuda")
with torch.no_grad():
    h_all = data.x
    for layer in range(2):
        nxt = torch.empty((N, shapes[2 * layer][1]), device="cuda")
        for batch in loader:
            block = batch.blocks[0]
            h_src = batch.x if layer == 0 else h_all[batch.n_id]
            out = conv(h_src, block.edge_index, block.n_dst, w[2 * layer], w[2 * layer + 1])
            nxt[batch.input_nodes] = F.relu(out) if layer == 0 else out
            if layer == 0:                   # the integer check: every node is handed its whole in-degree, once per epoch
                seen.index_add_(0, batch.input_nodes[block.edge_index[1]], torch.ones_like(block.edge_index[1]))
        h_all = nxt
    # the same model over the whole graph at once
    full = conv(F.relu(conv(data.x, data.edge_index, N, w[0], w[1])), data.edge_index, N, w[2], w[3])
in_degree = torch.bincount(data.edge_index[1], minlength=N)
accuracy = (h_all.argmax(1) == data.y).float().mean().item()
print("inference: %d nodes in %d mini-batches per layer, accuracy %.3f, equals the whole-graph forward: %s, "
      "block edges per node equal the in-degree: %s"
      % (N, len(loader), accuracy, torch.allclose(h_all, full, atol=1e-4), bool((seen == in_degree).all())))
