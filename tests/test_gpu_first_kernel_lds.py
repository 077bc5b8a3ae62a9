"""The staged pipeline's first kernel (win_stage_first_kernel) after its LDS diet: column starts held as u32 in LDS when the
graph brings the `ptrs32` shadow (i64 otherwise), hop 0 reading the seeds themselves instead of the copy it has just stored
(and the barrier of that round trip gone), the lean ticket chain, and as many persistent workgroups as stay resident
(tg_ns_win_tuning.stage_sort_blocks = auto) -- none of which may change an output word.

Graph and seeds are test_gpu_slab_alignment's (RMAT-14 plus isolated vertices and the little tree: batch 0's seeds all have
empty columns, batch 1 samples four edges or fewer), 16 KiB windows, the staged form forced, slabs poisoned.  Every case is
compared word for word with the fused kernel (form = 2) and, for three batches, with the CPU oracle in philox-mode.
n_seeds 1 / 63 / 65 / 1 023 / 1 025: below, around and beyond a 64-lane chunk and the 1 024 slots of a round (1 025 makes a
second round); fan-outs [15, 10], [16, 4], [32, 4]: the KFIRST = 16 and 32 instantiations; with and without replacement;
with and without `ptrs32` (narrow / wide column starts); 6 batches and 1; rows forced to 1, to 5 (fewer rows than batches:
the persistent loop revisits its LDS) and auto; rows_prefilled on and off."""
import numpy as np
import pytest
import torch

from test_gpu_slab_alignment import FUSED, WINDOWED, _graph, _seeds
from test_gpu_windowed_timed_scale import POISON, _poisoned, assert_oracle

DEV = "cuda:0"
NB, SEED, CALL0 = 6, 17, 300
ORACLE_BATCHES = (0, 1, 5)
SIZES = [1, 63, 65, 1023, 1025]
# (fan-out, sampler): KFIRST = 16 twice (15 and the full 16), KFIRST = 32, and sampling with replacement
LAWS = [([15, 10], 0), ([16, 4], 0), ([32, 4], 0), ([15, 10], 1)]
AUTO_ROWS = -1
# (ptrs32 shadow, stage_sort_blocks, first batch, batches, rows_prefilled)
VARIANTS = [(True, AUTO_ROWS, 0, NB, False),
            (True, 5, 0, NB, True),
            (True, 1, 0, NB, False),
            (False, AUTO_ROWS, 0, NB, False),
            (False, 5, 0, NB, True),
            (True, AUTO_ROWS, 5, 1, False),      # one persistent workgroup, the rest of the device idle
            (False, 1, 5, 1, True),
            (True, 5, 0, 1, False)]              # the one batch is the one whose seeds all have empty columns


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def world(cabi):
    n0, V, iso0, ptrs, idx, g = _graph(cabi)
    i32 = idx.to(torch.int32)
    wide = cabi.graph_view(ptrs, idx, indices32=i32, ptrs32=None, max_degree=g.max_degree)   # no u32 shadow of `ptrs`
    assert g.ptrs32 and not wide.ptrs32
    return dict(n0=n0, V=V, iso0=iso0, ptrs=ptrs, idx=idx, g=g, wide=wide, refs={})


def _reference(cabi, world, B, fan, sampler):
    """seeds and the fused kernel's output on poisoned slabs, once per (B, law), checked against the oracle"""
    key = (B, tuple(fan), sampler)
    if key not in world["refs"]:
        seeds = _seeds(world["n0"], world["V"], world["iso0"], NB, B)
        ref = _poisoned(cabi, NB, B, fan)
        cabi.ns_homo_batched(world["g"], seeds, fan, SEED, CALL0, ref, sampler=sampler, form=FUSED)
        torch.cuda.synchronize()
        assert int(ref.counts[0, 1]) == 0                        # batch 0: every seed's column is empty
        assert_oracle(cabi, ref, world["ptrs"], world["idx"], seeds, fan, SEED, CALL0, ORACLE_BATCHES, sampler=sampler)
        world["refs"][key] = (seeds, ref)
    return world["refs"][key]


def _assert_equals_reference(out, ref, b0, nb, prefilled, B):
    """batches [b0, b0 + nb) of the reference: counts, layer offsets, the used prefixes word for word, poison beyond"""
    sl = slice(b0, b0 + nb)
    assert torch.equal(out.counts, ref.counts[sl]) and torch.equal(out.layer_offsets, ref.layer_offsets[sl])
    for name, col in (("samples", 0), ("rows", 1), ("cols", 1), ("edge_index", 1)):
        x, y = getattr(out, name), getattr(ref, name)[sl]
        used = torch.arange(x.shape[1], device=x.device)[None, :] < out.counts[:, col:col + 1]
        assert bool(((x == y) | ~used).all()), name
        if name == "rows" and prefilled:                          # never stored: still the arange over the whole slab
            assert torch.equal(x, (torch.arange(x.shape[1], device=x.device) + B)[None, :].expand_as(x))
        else:
            assert bool(((x == POISON) | used).all()), "%s written beyond its used prefix" % name


@pytest.mark.gpu
@pytest.mark.parametrize("fan,sampler", LAWS, ids=["15x10", "16x4", "32x4", "15x10repl"])
@pytest.mark.parametrize("B", SIZES)
def test_staged_first_kernel_equals_fused_and_oracle(cabi, world, B, fan, sampler):
    dev = torch.device(DEV)
    seeds, ref = _reference(cabi, world, B, fan, sampler)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for shadow, rows, b0, nb, prefilled in VARIANTS:
        g = world["g"] if shadow else world["wide"]
        before = cabi.ns_win_tuning_set(window_bytes=1 << 14, staged=1, stage_sort_blocks=rows)
        try:
            assert cabi.ns_win_tuning()["stage_sort_blocks"] == rows
            sub = seeds[b0:b0 + nb].contiguous()
            ws = cabi.ns_homo_workspace(nb, B, fan, dev, staged=True, graph=g)
            if prefilled:
                out = cabi.NsBatchedOut(nb, B, fan, dev)
                for t in (out.samples, out.cols, out.edge_index):
                    t.fill_(POISON)
                assert out.struct().rows_prefilled == B + 1
            else:
                out = _poisoned(cabi, nb, B, fan)
                assert out.struct().rows_prefilled == 0
            assert cabi.ns_homo_batched_form(g, out, nb, B, fan, ws=ws, form=WINDOWED, sampler=sampler)[0] == WINDOWED
            assert cabi.ns_homo_batched_staged(g, out, nb, B, fan, ws=ws, form=WINDOWED, sampler=sampler) is True
            cabi.ns_homo_batched(g, sub, fan, SEED, CALL0 + b0, out, sampler=sampler, ws=ws, form=WINDOWED)
            torch.cuda.synchronize()
            first = cabi.ns_win_first_launch()
            assert first["narrow"] == shadow
            if rows == AUTO_ROWS:
                assert first["workgroups_per_cu"] >= 1
                assert first["rows"] == min(nb, 1024, first["workgroups_per_cu"] * cus)
            else:
                assert first["rows"] == min(nb, rows) and first["workgroups_per_cu"] == 0
            _assert_equals_reference(out, ref, b0, nb, prefilled, B)
            if nb == NB and rows == AUTO_ROWS:
                assert_oracle(cabi, out, world["ptrs"], world["idx"], seeds, fan, SEED, CALL0, ORACLE_BATCHES, sampler=sampler)
        finally:
            cabi.ns_win_tuning_set(**before)
    assert cabi.ns_win_tuning()["stage_sort_blocks"] == AUTO_ROWS     # the default, restored


def test_first_kernel_lds_request():
    """The first kernel's LDS arithmetic (no device needed).  bench.py's shape -- 256 threads, kmax 16, 264 coarse buckets,
    2 049 windows: with u32 column starts four workgroups fit a CU's 160 KB (<= 40 960 bytes each); with i64 ones the request
    is what it was before the narrow form existed, 42 376 bytes."""
    from tch_geometric import _cabi
    wave = 64 * 16 * 4 + 64 * 16 + 64                                    # staged positions u32, lanes u8, drawing lanes
    tables = (264 + 2049 + 1) * 4                                       # coarse counters, vertex table
    head_wide = 80 + 16 + 16 * 64 * (8 + 4)                              # chunk offsets, fbase, column starts i64, degrees
    head_narrow = 80 + 16 + 16 * 64 * (4 + 4)
    assert head_wide + 4 * wave + tables == 42376
    assert _cabi.ns_win_first_lds_bytes(256, 16, 264, 2049, False) == (256, 42376)
    assert _cabi.ns_win_first_lds_bytes(256, 16, 264, 2049, True) == (256, head_narrow + 4 * wave + tables)
    assert _cabi.ns_win_first_lds_bytes(256, 16, 264, 2049, True)[1] <= 40960
    # the launch bound caps the workgroup at 512 threads, and it halves until the request fits 64 KB
    assert _cabi.ns_win_first_lds_bytes(1024, 16, 264, 2049, False) == (512, head_wide + 8 * wave + tables)
    wave32 = 64 * 32 * 4 + 64 * 32 + 64
    assert head_wide + 8 * wave32 + tables > 65536
    assert _cabi.ns_win_first_lds_bytes(512, 32, 264, 2049, False) == (256, head_wide + 4 * wave32 + tables)
    assert _cabi.ns_win_first_lds_bytes(512, 32, 264, 2049, True) == (256, head_narrow + 4 * wave32 + tables)
