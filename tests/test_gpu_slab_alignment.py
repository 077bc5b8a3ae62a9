"""Output slabs at independent alignments.

tg_ns_out takes four independent int64 pointers: a caller slicing one big buffer may pass slabs whose bases differ modulo
16 and 64 bytes.  The emit passes store 16-byte pairs from each stream's own 64-byte (or 16-byte) boundary on, so any
8-byte aligned views give the same outputs.  Here the four slabs are views into ONE flat poisoned buffer, each at its own
element offset ((0, 1, 3, 6) and its rotations: every pair of streams differs modulo 2 and modulo 8 elements), filled
by every launch form and compared word for word with a normal NsBatchedOut filled by the fused kernel (used prefixes equal,
everything past them and every element between the views still poison), and by the CPU oracle.  Batch 0 samples no edge
at all and batch 1 four, fewer than the scalar prologue of at least one edge stream stores (asserted), so that prologue
alone writes the batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from test_gpu_windowed_timed_scale import POISON, _poisoned, assert_equal_on_device, assert_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOWED, FUSED, WINDOWED_WIDE = 1, 2, 3
OFFSETS = (0, 1, 3, 6)
ROTATIONS = [OFFSETS[i:] + OFFSETS[:i] for i in range(4)]
GAP = 40                                                     # poison elements at least between two views


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


class FlatOut:
    """NsBatchedOut-shaped: samples / rows / cols / edge_index are [n_batches, pitch] views into one flat buffer, view i
    starting `offsets[i]` elements past a 64-byte boundary.  NsBatchedOut.struct / batch read only these attributes."""

    def __init__(self, cabi, nb, B, fan, offsets):
        self.n_batches, self.n_seeds, self.n_hops = nb, B, len(fan)
        self.cap_nodes, self.cap_edges = cabi.ns_homo_capacity(B, fan)
        pitches = (max(self.cap_nodes, 1),) + (max(self.cap_edges, 1),) * 3
        at, self.spans = GAP, []
        for off, pitch in zip(offsets, pitches):
            at = (at + 7) // 8 * 8 + off
            self.spans.append((at, at + nb * pitch))
            at += nb * pitch + GAP
        self.flat = torch.full((at + 8,), POISON, dtype=torch.int64, device=DEV)
        assert self.flat.data_ptr() % 64 == 0
        views = [self.flat[a:e].view(nb, p) for (a, e), p in zip(self.spans, pitches)]
        self.samples, self.rows, self.cols, self.edge_index = views
        for v, off in zip(views, offsets):
            assert v.data_ptr() % 64 == off * 8
        self.layer_offsets = torch.zeros((nb, max(self.n_hops, 1), 3), dtype=torch.int64, device=DEV)
        self.counts = torch.zeros((nb, 2), dtype=torch.int64, device=DEV)
        self.states = None

    def struct(self):
        from tch_geometric._cabi import NsBatchedOut
        return NsBatchedOut.struct(self)

    def batch(self, b, counts=None):
        from tch_geometric._cabi import NsBatchedOut
        return NsBatchedOut.batch(self, b, counts)

    def assert_gaps_poison(self):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for a, e in self.spans:
            keep[a:e] = False
        assert bool((self.flat[keep] == POISON).all()), "a store landed between the views"


def _head(t, b, pitch, am=7):
    """elements of batch b's stream that an emit pass stores alone before the stream's next 64-byte boundary"""
    return (am + 1 - ((t.data_ptr() // 8 + b * pitch) & am)) & am


def _graph(cabi):
    """RMAT-14 plus 4 096 isolated vertices and a little tree: V <- {U1, U2}, U1 <- W1, U2 <- W2 (W isolated), so that a
    batch seeded on V and isolated vertices samples exactly four edges"""
    dev = torch.device(DEV)
    n0 = 1 << 14
    row, col = cabi.rmat_edges(14, n0 * 16, 0x5EED0A11, dev)
    V, U1, U2, W1, W2 = n0, n0 + 1, n0 + 2, n0 + 3, n0 + 4
    iso0, n = n0 + 8, n0 + 8 + 4096
    extra = torch.tensor([[U1, U2, W1, W2], [V, V, U1, U2]], dtype=torch.int64, device=dev)   # (source row, column)
    row, col = torch.cat([row, extra[0]]), torch.cat([col, extra[1]])
    ptrs, idx, _ = cabi.coo_to_csx(row, col, n, n, True)
    g = cabi.graph_view(ptrs, idx, indices32=idx.to(torch.int32), ptrs32=ptrs.to(torch.int32), max_degree="auto")
    return n0, V, iso0, ptrs, idx, g


def _seeds(n0, V, iso0, nb, B):
    gen = torch.Generator(device=DEV).manual_seed(B)
    seeds = torch.randint(0, n0, (nb, B), device=DEV, generator=gen)
    seeds[0] = torch.arange(iso0, iso0 + B, device=DEV)           # no edge at all
    seeds[1] = torch.arange(iso0, iso0 + B, device=DEV)
    seeds[1, B // 2] = V                                            # four edges
    return seeds.contiguous()


# (label, tuning, form): the fused kernel, the push windowed form with narrow and wide items, the staged pipeline with
# 64- and 16-byte store alignment, and with its emit pass split from the gather
FORMS = [("fused", {}, FUSED),
         ("push", dict(staged=0), WINDOWED),
         ("push_wide", dict(staged=0), WINDOWED_WIDE),
         ("staged_a64", dict(staged=1, store_align64=1), WINDOWED),
         ("staged_a16", dict(staged=1, store_align64=0), WINDOWED),
         ("staged_split", dict(staged=1, stage_split=1), WINDOWED)]


@pytest.mark.parametrize("B", [1024, 1023])
def test_every_launch_form_on_independently_aligned_slabs(cabi, B):
    dev = torch.device(DEV)
    n0, V, iso0, ptrs, idx, g = _graph(cabi)
    nb, fan, seed, call0 = 6, [15, 10], 17, 300
    seeds = _seeds(n0, V, iso0, nb, B)
    ref = _poisoned(cabi, nb, B, fan)
    cabi.ns_homo_batched(g, seeds, fan, seed, call0, ref, form=FUSED)
    torch.cuda.synchronize()
    assert int(ref.counts[0, 1]) == 0 and int(ref.counts[1, 1]) == 4 and int(ref.counts[2:, 1].min()) > 1000
    for label, tuning, form in FORMS:
        before = cabi.ns_win_tuning_set(window_bytes=1 << 14, **tuning)
        try:
            for offsets in ROTATIONS:
                out = FlatOut(cabi, nb, B, fan, offsets)
                # batch 1's four edges: fewer than the scalar prologue of at least one edge stream (offsets 1 / 3 -> 7 / 5)
                assert max(_head(t, 1, out.cap_edges) for t in (out.rows, out.cols, out.edge_index)) > 4
                ws = None
                if form != FUSED:
                    ws = cabi.ns_homo_workspace(nb, B, fan, dev, staged=tuning.get("staged") == 1, graph=g)
                    assert cabi.ns_homo_batched_form(g, out, nb, B, fan, ws=ws, form=form)[0] == form
                    assert cabi.ns_homo_batched_staged(g, out, nb, B, fan, ws=ws, form=form) == (tuning["staged"] == 1)
                cabi.ns_homo_batched(g, seeds, fan, seed, call0, out, ws=ws, form=form)
                torch.cuda.synchronize()
                assert_equal_on_device(out, ref)
                out.assert_gaps_poison()
                assert_oracle(cabi, out, ptrs, idx, seeds, fan, seed, call0, (0, 1, nb - 1))
                del out, ws
        finally:
            cabi.ns_win_tuning_set(**before)


@pytest.mark.parametrize("world", [1, 3])
def test_mode2_slot_replies_on_independently_aligned_slabs(cabi, world):
    """range-partitioned sampling, fixed-size slot replies (tg_part_emit_slots), the all-to-alls emulated in one process"""
    from helpers_part import emulated_world_sample
    from tch_geometric import partitioned
    dev = torch.device(DEV)
    n0, V, iso0, ptrs, idx, g = _graph(cabi)
    fan, seed, call0 = [7, 5], 23, 900
    for B in (64, 63):
        nb = 5
        seeds = _seeds(n0, V, iso0, nb, B)
        ref = _poisoned(cabi, nb, B, fan)
        cabi.ns_homo_batched(g, seeds, fan, seed, call0, ref, form=FUSED)
        shards = [partitioned.CscShard.from_full(ptrs, idx, r, world) for r in range(world)]
        for offsets in ROTATIONS:
            out = FlatOut(cabi, nb, B, fan, offsets)
            got, _ = emulated_world_sample(cabi, shards, seeds, fan, seed, call0, slots=True, out=out)
            assert got is out
            assert_equal_on_device(out, ref)
            out.assert_gaps_poison()
            assert_oracle(cabi, out, ptrs, idx, seeds, fan, seed, call0, (0, 1, nb - 1))


def test_compact_from_and_into_misaligned_buffers(cabi):
    """tg_ns_homo_compact: misaligned slabs in, four flat outputs that are views of one buffer at offsets 1, 3, 6, 0 out"""
    dev = torch.device(DEV)
    n0, V, iso0, ptrs, idx, g = _graph(cabi)
    nb, B, fan = 6, 1023, [15, 10]
    seeds = _seeds(n0, V, iso0, nb, B)
    out = FlatOut(cabi, nb, B, fan, ROTATIONS[1])
    cabi.ns_homo_batched(g, seeds, fan, 5, 60, out, form=FUSED)
    counts = out.counts.cpu()
    tn, te = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    off = torch.zeros((2, nb + 1), dtype=torch.int64, device=dev)
    off[:, 1:] = torch.cumsum(out.counts.t(), dim=1)
    sizes, at, spans = (tn, te, te, te), GAP, []
    for o, size in zip((1, 3, 6, 0), sizes):
        at = (at + 7) // 8 * 8 + o
        spans.append((at, at + size))
        at += size + GAP
    flat = torch.full((at + 8,), POISON, dtype=torch.int64, device=dev)
    fs, fr, fc, fe = (flat[a:e] for a, e in spans)
    so = out.struct()
    cabi.check(cabi.lib.tg_ns_homo_compact(C.byref(so), C.c_int64(nb), cabi.ptr(off[0]), cabi.ptr(off[1]), cabi.ptr(fs),
                                           cabi.ptr(fr), cabi.ptr(fc), cabi.ptr(fe), cabi.stream_ptr(dev)))
    torch.cuda.synchronize()
    hp, hi = ptrs.cpu().numpy(), idx.cpu().numpy()
    want = [[], [], [], []]
    for b in range(nb):
        o = orc.ns_homo(hp, hi, seeds[b].cpu().numpy(), fan, orc.rng_philox(5, 60 + b))
        for w, x in zip(want, o[:4]):
            w.append(np.asarray(x, dtype=np.int64))
    for got, w in zip((fs, fr, fc, fe), want):
        assert np.array_equal(got.cpu().numpy(), np.concatenate(w))
    keep = torch.ones_like(flat, dtype=torch.bool)
    for a, e in spans:
        keep[a:e] = False
    assert bool((flat[keep] == POISON).all())
