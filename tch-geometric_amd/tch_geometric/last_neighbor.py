"""The memory-based temporal GNNs' sampler (TGN, Rossi et al. 2020) on the streaming last-k neighbour state of
include/tchgeo_lastn.h: `LastNeighborLoader` with the shape of PyG's torch_geometric.nn.models.tgn.LastNeighborLoader, and
`TemporalEventLoader`, which walks a chronological event list in mini-batches, looking every batch's neighbourhood up BEFORE
the batch is inserted (tg_lastn_replay: `prefetch` such steps per launch)."""
from typing import List, Optional

import torch
from torch import Tensor

from . import _cabi
from ._cabi_lastn import LastN, _fanout, _sizes
from .loader import _Loader, _at_least_1, _epoch_plan


def _device(device):
    return torch.device("cuda" if device is None else device)


def _trim(out, uniq, g: int, counts):
    """mini-batch g of a launch -> (n_id, edge_index, e_id), trimmed by the read-back counts"""
    n_nodes, n_edges = int(counts[g, 0]), int(counts[g, 1])
    edge_index = torch.stack([uniq.rows[g, :n_edges], uniq.cols[g, :n_edges]])
    return uniq.nodes[g, :n_nodes], edge_index, out.edge_index[g, :n_edges]


class LastNeighborLoader:
    """PyG's LastNeighborLoader on the device-resident ring: `insert(src, dst)` appends a batch of interactions (both
    directions, with ids from the running counter `cur_e_id`), `loader(n_id)` returns (n_id, edge_index, e_id): for every
    input node its `size` most recent interactions, newest first; edge_index[0] = the neighbour, edge_index[1] = the query
    node, both numbered against the returned n_id; e_id = the interactions' ids.

    Two differences from PyG's.  The returned n_id holds the inputs first (repeats of an input collapse onto its first
    occurrence), then the new neighbours in order of first occurrence -- tg_ns_homo_unique's order -- where PyG returns them
    sorted.  And a node with more than `size` interactions in ONE insert keeps exactly its newest `size`; PyG numbers a
    batch's interactions of a node with `arange % size`, which collides there.

    num_hops > 1 expands the neighbours again at the same state (fan-out `size` per hop); edge_index[1] is then the
    expanded node's number in n_id.  A lookup synchronises twice (status, then sizes); an insert does not."""

    def __init__(self, num_nodes: int, size: int, device=None, num_hops: int = 1):
        self.num_nodes, self.size = _sizes("LastNeighborLoader", num_nodes, size)
        self.fanout = _fanout("LastNeighborLoader", [self.size] * int(num_hops), self.size)
        _at_least_1("num_hops", num_hops)
        self.device = _device(device)
        self.lastn = LastN(self.num_nodes, self.size, self.device)
        self.cur_e_id = 0

    def reset_state(self):
        self.lastn.reset()
        self.cur_e_id = 0

    def insert(self, src: Tensor, dst: Tensor):
        src = src.to(self.device, torch.int64).reshape(-1).contiguous()
        dst = dst.to(self.device, torch.int64).reshape(-1).contiguous()
        self.lastn.insert(src, dst, e_base=self.cur_e_id, symmetric=True)
        self.cur_e_id += src.numel()

    def __call__(self, n_id: Tensor, num_hops: Optional[int] = None):
        fanout = self.fanout if num_hops is None else _fanout("LastNeighborLoader", [self.size] * int(num_hops), self.size)
        seeds = n_id.to(self.device, torch.int64).reshape(1, -1).contiguous()
        out = self.lastn.sample(seeds, fanout)
        self.lastn.status_check("LastNeighborLoader")      # every id the dedup sees is inside [0, num_nodes)
        uniq = _cabi.ns_homo_unique(out, 1, self.num_nodes, in_place=True, with_inverse=False)
        return _trim(out, uniq, 0, uniq.counts.cpu())

    def state_dict(self):
        d = self.lastn.state_dict()
        d["cur_e_id"] = self.cur_e_id
        return d

    def load_state_dict(self, d):
        self.lastn.load_state_dict(d)
        self.cur_e_id = int(d["cur_e_id"])


class TemporalEventBatch:
    """One mini-batch of TemporalEventLoader: the events `src`, `dst`, `t` with their numbers `input_id`, the negatives
    `neg_dst` [len(src) * neg_sampling_ratio], and the neighbourhood of src ++ dst ++ neg_dst in the state BEFORE these events:
    `n_id`, `edge_index` (neighbour, query position; numbered against n_id), `e_id` (event numbers: gather t[e_id] or
    messages with them); n_id[src_index] == src, n_id[dst_index] == dst, n_id[neg_index] == neg_dst."""
    __slots__ = ("src", "dst", "t", "neg_dst", "n_id", "edge_index", "e_id", "src_index", "dst_index", "neg_index", "input_id")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class TemporalEventLoader(_Loader):
    """A chronological event list (src, dst, t; t ascending) in mini-batches of `batch_size` events, in order (no shuffle):
    mini-batch j carries its events, `neg_sampling_ratio` negative destinations per event (drawn unchecked and uniformly from
    neg_range = [lo, hi), default all nodes, by a device generator keyed by (seed, epoch, launch)), and the `size` most
    recent interactions (num_neighbors: fan-out per hop, default [size]) of all of these nodes among the events of the
    mini-batches before j.  One launch (tg_lastn_replay) serves `prefetch` mini-batches; the ragged last one is a launch of
    its own.  The state is reset when an epoch starts.  The loader holds ONE state: starting a second iterator refuses the
    first, which raises RuntimeError at its next launch."""

    def __init__(self, src: Tensor, dst: Tensor, t: Tensor, num_nodes: int, size: int, batch_size: int,
                 num_neighbors: Optional[List[int]] = None, neg_sampling_ratio: int = 1, neg_range=None, prefetch: int = 16,
                 seed: int = 0, device=None):
        self.num_nodes, self.size = _sizes("TemporalEventLoader", num_nodes, size)
        self.fanout = _fanout("TemporalEventLoader", [self.size] if num_neighbors is None else num_neighbors, self.size)
        _at_least_1("batch_size", batch_size)
        _at_least_1("prefetch", prefetch)
        if int(neg_sampling_ratio) < 0:
            raise ValueError("neg_sampling_ratio must be at least 0, got %r" % (neg_sampling_ratio,))
        lo, hi = (0, self.num_nodes) if neg_range is None else (int(neg_range[0]), int(neg_range[1]))
        if not 0 <= lo < hi <= self.num_nodes:
            raise ValueError("neg_range = [%d, %d) is empty or outside [0, %d)" % (lo, hi, self.num_nodes))
        src, dst, t = (x.reshape(-1).to(torch.int64) for x in (src, dst, t))
        if not src.numel() == dst.numel() == t.numel():
            raise ValueError("src, dst and t differ in length: %d, %d, %d" % (src.numel(), dst.numel(), t.numel()))
        if t.numel() > 1 and bool((t[1:] < t[:-1]).any()):
            raise ValueError("t is not ascending: the events must be in chronological order")
        for name, x in (("src", src), ("dst", dst)):
            if x.numel() and (int(x.min()) < 0 or int(x.max()) >= self.num_nodes):
                raise IndexError("%s outside [0, %d)" % (name, self.num_nodes))
        self.batch_size, self.prefetch, self.ratio, self.neg_range = int(batch_size), int(prefetch), int(neg_sampling_ratio), (lo, hi)
        self.seed, self.epoch, self.drop_last = int(seed), 0, False
        self.device = _device(device)
        self.src, self.dst, self.t = (x.to(self.device).contiguous() for x in (src, dst, t))
        self.lastn = LastN(self.num_nodes, self.size, self.device)
        self._live = None

    def __len__(self) -> int:
        return (self.src.numel() + self.batch_size - 1) // self.batch_size

    def _negatives(self, epoch: int, launch: int, G: int, width: int) -> Tensor:
        gen = torch.Generator(device=self.device)
        gen.manual_seed((self.seed * 1000003 + epoch) * 1000003 + launch)
        return torch.randint(self.neg_range[0], self.neg_range[1], (G, width * self.ratio), device=self.device, generator=gen)

    def _launch(self, epoch: int, launch: int, start: int, G: int, width: int):
        """mini-batches start // batch_size ... of the epoch -> their TemporalEventBatch list; one read-back"""
        stop = start + G * width
        src, dst = self.src[start:stop], self.dst[start:stop]
        neg = self._negatives(epoch, launch, G, width)
        seeds = torch.cat([src.view(G, width), dst.view(G, width), neg], dim=1).contiguous()
        out = self.lastn.replay(src, dst, seeds, self.fanout, width, e_base=start)
        uniq = _cabi.ns_homo_unique(out, G, self.num_nodes, in_place=True)
        counts = uniq.counts.cpu()
        batches = []
        for g in range(G):
            a, b = start + g * width, start + (g + 1) * width
            n_id, edge_index, e_id = _trim(out, uniq, g, counts)
            inv = uniq.inverse[g]
            batches.append(TemporalEventBatch(
                src=self.src[a:b], dst=self.dst[a:b], t=self.t[a:b], neg_dst=neg[g], n_id=n_id, edge_index=edge_index, e_id=e_id,
                src_index=inv[:width], dst_index=inv[width:2 * width], neg_index=inv[2 * width:(2 + self.ratio) * width],
                input_id=torch.arange(a, b, device=self.device)))
        return batches

    def __iter__(self):
        epoch, token = self.epoch, object()
        self.epoch += 1
        self._live = token
        self.lastn.reset()
        for launch, (start, G, width) in enumerate(_epoch_plan(self.src.numel(), self.batch_size, self.prefetch, False)):
            if self._live is not token:
                raise RuntimeError("TemporalEventLoader: a newer iterator owns the state; this one is refused")
            yield from self._launch(epoch, launch, start, G, width)
