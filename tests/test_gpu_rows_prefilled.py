"""tg_ns_out.rows_prefilled: rows[e] = n_seeds + e whatever is sampled, so a slab that holds the arange (NsBatchedOut
fills it once, tg_ns_rows_fill) need not be written again -- the fused kernel and both pipelines of the window-ordered form
skip that stream for a matching slab, and only for one.

Graph and seeds are test_gpu_slab_alignment's: RMAT-14 plus isolated vertices and the little tree; batch 0 samples no
edge, batch 1 four (the store prologue alone writes such a batch).  Every launch form runs at nb = 6, B in {1 024, 1 023}
(odd pitch), fan-out [15, 10], 16 KiB windows."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from test_gpu_slab_alignment import FORMS, FUSED, _graph, _seeds
from test_gpu_windowed_timed_scale import POISON, _poisoned, assert_equal_on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB, FAN, SEED, CALL0 = 6, [15, 10], 17, 300
ORACLE_BATCHES = (0, 1, 5)


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def world(cabi):
    """graph, and per B: seeds, the fused reference on normal (poisoned, so: written) slabs, the oracle's batches"""
    n0, V, iso0, ptrs, idx, g = _graph(cabi)
    hp, hi = ptrs.cpu().numpy(), idx.cpu().numpy()
    per_b = {}
    for B in (1024, 1023):
        seeds = _seeds(n0, V, iso0, NB, B)
        ref = _poisoned(cabi, NB, B, FAN)
        assert ref.struct().rows_prefilled == 0
        cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0, ref, form=FUSED)
        torch.cuda.synchronize()
        assert int(ref.counts[0, 1]) == 0 and int(ref.counts[1, 1]) == 4 and int(ref.counts[2:, 1].min()) > 1000
        want = {j: orc.ns_homo(hp, hi, seeds[j].cpu().numpy(), FAN, orc.rng_philox(SEED, CALL0 + j)) for j in ORACLE_BATCHES}
        per_b[B] = (seeds, ref, want)
    return dict(g=g, ptrs=ptrs, idx=idx, n_nodes=int(ptrs.numel()) - 1, per_b=per_b)


def _arange_slab(out, B):
    return (torch.arange(out.rows.shape[1], device=out.rows.device) + B)[None, :].expand_as(out.rows)


def _each_form(cabi, g, B):
    """-> (label, form, workspace) under that form's tuning, one at a time"""
    dev = torch.device(DEV)
    for label, tuning, form in FORMS:
        before = cabi.ns_win_tuning_set(window_bytes=1 << 14, **tuning)
        try:
            ws = None
            if form != FUSED:
                ws = cabi.ns_homo_workspace(NB, B, FAN, dev, staged=tuning.get("staged") == 1, graph=g)
            yield label, tuning, form, ws
        finally:
            cabi.ns_win_tuning_set(**before)


def _launch_struct(cabi, g, seeds, so, ws, form):
    """the C entry points with a hand-built tg_ns_out"""
    fan = (C.c_int64 * len(FAN))(*FAN)
    cfg, rng = cabi.TgNsConfig(), cabi.TgRng(SEED, CALL0)
    cfg.sampler, cfg.filter_mode = cabi.SAMPLER_UNIFORM, cabi.FILTER_NONE
    args = (C.byref(g), cabi.ptr(seeds), C.c_int64(seeds.shape[0]), C.c_int64(seeds.shape[1]), fan, C.c_int32(len(FAN)),
            C.byref(cfg), C.byref(rng), C.byref(so))
    if ws is not None:
        cabi.check(cabi.lib.tg_ns_homo_batched_ws(*args, cabi.ptr(ws), C.c_int64(ws.numel() * 8), C.c_int32(form),
                                                  cabi.stream_ptr(seeds.device)))
    else:
        cabi.check(cabi.lib.tg_ns_homo_batched(*args, cabi.stream_ptr(seeds.device)))
    torch.cuda.synchronize()


def _assert_form_taken(cabi, g, out, B, ws, tuning, form):
    if form != FUSED:
        assert cabi.ns_homo_batched_form(g, out, NB, B, FAN, ws=ws, form=form)[0] == form
        assert cabi.ns_homo_batched_staged(g, out, NB, B, FAN, ws=ws, form=form) == (tuning["staged"] == 1)


def _assert_all_but_rows(out, ref, want):
    """counts, layer offsets and the used prefixes of samples / cols / edge_index equal the reference's (poison beyond),
    and the oracle's for its batches"""
    assert torch.equal(out.counts, ref.counts) and torch.equal(out.layer_offsets, ref.layer_offsets)
    for name, col in (("samples", 0), ("cols", 1), ("edge_index", 1)):
        x, y = getattr(out, name), getattr(ref, name)
        used = torch.arange(x.shape[1], device=x.device)[None, :] < out.counts[:, col:col + 1]
        assert bool(((x == y) | ~used).all()), name
        assert bool(((x == POISON) | used).all()), "%s written beyond its used prefix" % name
    for j, o in want.items():
        s, _r, c, e, lo = out.batch(j)
        assert lo == o[4]
        for got, w in ((s, o[0]), (c, o[2]), (e, o[3])):
            assert np.array_equal(got.cpu().numpy(), w), j


def _assert_oracle(out, want):
    for j, o in want.items():
        x = out.batch(j)
        assert x[4] == o[4]
        for u, v in zip(x[:4], o[:4]):
            assert np.array_equal(u.cpu().numpy(), v), j


@pytest.mark.parametrize("B", [1024, 1023])
def test_fresh_slab_holds_the_arange_and_says_so(cabi, B):
    out = cabi.NsBatchedOut(NB, B, FAN, torch.device(DEV))
    torch.cuda.synchronize()
    assert torch.equal(out.rows, _arange_slab(out, B))
    assert out.struct().rows_prefilled == B + 1
    assert out.rows._version == 0                                   # the fill went through the raw pointer


@pytest.mark.parametrize("B", [1024, 1023])
def test_matching_field_skips_the_rows_stream_and_nothing_else(cabi, world, B):
    """poisoned slabs + a hand-set rows_prefilled = B + 1: `rows` is never touched, everything else is what it was"""
    g = world["g"]
    seeds, ref, want = world["per_b"][B]
    seen = []
    for label, tuning, form, ws in _each_form(cabi, g, B):
        seen.append(label)
        out = _poisoned(cabi, NB, B, FAN)
        _assert_form_taken(cabi, g, out, B, ws, tuning, form)
        so = out.struct()
        assert so.rows_prefilled == 0
        so.rows_prefilled = B + 1
        _launch_struct(cabi, g, seeds, so, ws, form)
        assert bool((out.rows == POISON).all()), "%s stored into a slab it was told holds its rows" % label
        _assert_all_but_rows(out, ref, want)
    assert seen == ["fused", "push", "push_wide", "staged_a64", "staged_a16", "staged_split"]


@pytest.mark.parametrize("B", [1024, 1023])
def test_default_path_every_form(cabi, world, B):
    """a fresh NsBatchedOut: all four arrays are the oracle's, and `rows` is still the arange over the whole slab"""
    g = world["g"]
    seeds, ref, want = world["per_b"][B]
    for label, tuning, form, ws in _each_form(cabi, g, B):
        out = cabi.NsBatchedOut(NB, B, FAN, torch.device(DEV))
        for t in (out.samples, out.cols, out.edge_index):
            t.fill_(POISON)
        _assert_form_taken(cabi, g, out, B, ws, tuning, form)
        assert out.struct().rows_prefilled == B + 1
        cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0, out, ws=ws, form=form)
        torch.cuda.synchronize()
        _assert_oracle(out, want)
        _assert_all_but_rows(out, ref, want)
        used = torch.arange(out.rows.shape[1], device=DEV)[None, :] < out.counts[:, 1:2]
        assert bool(((out.rows == ref.rows) | ~used).all()), label
        assert torch.equal(out.rows, _arange_slab(out, B)), label
        assert out.struct().rows_prefilled == B + 1                  # and the next launch skips again


@pytest.mark.parametrize("B", [1024, 1023])
def test_guards_torch_write_and_other_n_seeds(cabi, world, B):
    g = world["g"]
    seeds, ref, want = world["per_b"][B]
    for label, tuning, form, ws in _each_form(cabi, g, B):
        # an in-place torch write ends the mark: the launch writes the used prefix and leaves the rest alone
        out = cabi.NsBatchedOut(NB, B, FAN, torch.device(DEV))
        for t in (out.samples, out.rows, out.cols, out.edge_index):
            t.fill_(POISON)
        assert out.struct().rows_prefilled == 0
        cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0, out, ws=ws, form=form)
        torch.cuda.synchronize()
        assert_equal_on_device(out, ref)
        _assert_oracle(out, want)
        # a field that names another n_seeds makes the launch write as well
        out2 = _poisoned(cabi, NB, B, FAN)
        so = out2.struct()
        so.rows_prefilled = B + 2
        _launch_struct(cabi, g, seeds, so, ws, form)
        assert_equal_on_device(out2, ref)


def test_the_mark_follows_the_tensor(cabi):
    dev, B = torch.device(DEV), 1024
    first, second = cabi.NsBatchedOut(NB, B, FAN, dev), cabi.NsBatchedOut(NB, B, FAN, dev)
    mix = copy.copy(second)
    mix.samples = second.samples
    mix.rows, mix.cols, mix.edge_index = first.rows, first.cols, first.edge_index
    assert mix.struct().rows_prefilled == B + 1 and mix.struct().rows == first.rows.data_ptr()
    view = copy.copy(first)
    view.rows = first.rows[:]
    assert view.rows.data_ptr() == first.rows.data_ptr() and view.struct().rows_prefilled == 0      # a view carries none
    other = copy.copy(first)
    other.n_seeds = B - 1                                             # slab filled for B, object says B - 1
    assert other.struct().rows_prefilled == 0
    with torch.inference_mode():
        inf = cabi.NsBatchedOut(2, 8, [2], dev)                       # inference tensors keep no version
    assert inf.struct().rows_prefilled == 0
    torch.cuda.synchronize()
    assert torch.equal(inf.rows, _arange_slab(inf, 8))
    first.rows[0, 0] = 5                                              # any in-place write: the mark is void everywhere
    assert first.struct().rows_prefilled == 0 and mix.struct().rows_prefilled == 0


@pytest.mark.parametrize("label", ["fused", "staged_a64"])
def test_in_place_unique_ends_the_mark(cabi, world, label):
    B = 1023
    g = world["g"]
    seeds, ref, want = world["per_b"][B]
    for lab, tuning, form, ws in _each_form(cabi, g, B):
        if lab != label:
            continue
        out = cabi.NsBatchedOut(NB, B, FAN, torch.device(DEV))
        cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0, out, ws=ws, form=form)
        assert out.struct().rows_prefilled == B + 1
        u = cabi.ns_homo_unique(out, NB, world["n_nodes"], in_place=True)
        assert u.rows is out.rows and out.struct().rows_prefilled == 0
        torch.cuda.synchronize()
        assert not torch.equal(out.rows, _arange_slab(out, B))       # relabelled rows lie in the slab now
        cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0, out, ws=ws, form=form)
        torch.cuda.synchronize()
        _assert_oracle(out, want)
        used = torch.arange(out.rows.shape[1], device=DEV)[None, :] < out.counts[:, 1:2]
        assert bool(((out.rows == ref.rows) | ~used).all())
        # a reused result object writes through the raw pointer at every call: still no mark
        cabi.ns_homo_unique(out, NB, world["n_nodes"], result=u)
        assert out.struct().rows_prefilled == 0


def test_launch_with_fewer_seeds_into_the_same_slabs_ends_the_mark(cabi, world):
    """a launch with another n_seeds writes ITS rows (n_seeds' + e); the slab no longer holds what the mark says"""
    B = 1024
    g = world["g"]
    seeds, ref, want = world["per_b"][B]
    out = cabi.NsBatchedOut(NB, B, FAN, torch.device(DEV))
    half = seeds[:, :B // 2].contiguous()
    cabi.ns_homo_batched(g, half, FAN, SEED, CALL0, out, form=FUSED)
    torch.cuda.synchronize()
    ne = int(out.counts[5, 1])
    assert ne > 0 and torch.equal(out.rows[5, :ne], torch.arange(ne, device=DEV) + B // 2)
    assert out.struct().rows_prefilled == 0
    cabi.ns_homo_batched(g, seeds, FAN, SEED, CALL0, out, form=FUSED)
    torch.cuda.synchronize()
    _assert_oracle(out, want)


def test_rows_fill_misaligned_odd_pitch_and_more_than_one_sweep(cabi):
    """a slab that starts 8 bytes past a 16-byte boundary with an odd pitch (pairs straddle batches), and one longer than
    the grid covers in one sweep; nothing lands outside the slab"""
    dev = torch.device(DEV)
    for nb, pitch, n_seeds, off in ((5, 7, 3, 1), (3, 1, 9, 1), (2, 8, 0, 0), (1, 1, 4, 1), (67, 131075, 1024, 1)):
        flat = torch.full((nb * pitch + 16,), POISON, dtype=torch.int64, device=dev)
        assert flat.data_ptr() % 16 == 0
        slab = flat[off:off + nb * pitch].view(nb, pitch)
        cabi.ns_rows_fill(slab, n_seeds)
        torch.cuda.synchronize()
        assert torch.equal(slab, (torch.arange(pitch, device=dev) + n_seeds)[None, :].expand(nb, pitch))
        assert bool((flat[:off] == POISON).all()) and bool((flat[off + nb * pitch:] == POISON).all())
