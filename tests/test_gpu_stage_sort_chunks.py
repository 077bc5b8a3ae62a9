"""The staged sort's level 1 writes whole aligned 64-byte chunks (win_scatter8_carry_kernel): per coarse bucket the items
behind the last 64-byte boundary of the destination address wait in an LDS carry for the workgroup's next tile, and the
carries are flushed after the row's last batch.  Nothing of that may change an output word.

Graph: test_gpu_slab_alignment's (RMAT-14 plus 4 096 isolated vertices), 16-KiB windows (hundreds of windows, dozens of
coarse buckets), the staged form forced, slabs poisoned.  Every case is compared word for word with the fused kernel
(form = 2) on the same seeds and call ids, and a few batches with the CPU oracle in philox-mode.

Frontier sizes are made exact: without replacement a seed of degree d hands min(d, 15) items to hop 1, so a batch seeded with
m vertices of degree >= 15, one vertex of degree r < 15 and isolated vertices has a hop-1 frontier of exactly 15 m + r items.
The tile is WIN_SC_CARRY_TILE = 4 096 items (2 048 was measured as well): both sizes, each - 1 / exact / + 1; 1, 7 and 8 items
(nothing but carries, one whole chunk); 0; three batches of 8 192 in all (the step of the second sort level)."""
import pytest
import torch

from test_gpu_slab_alignment import FUSED, WINDOWED, _graph
from test_gpu_windowed_timed_scale import _poisoned, _rmat, assert_equal_on_device, assert_oracle

DEV = "cuda:0"
SEED, CALL0 = 23, 4100
K0 = 15
B = 281                                    # odd, and 281 * 15 >= 4 097: with K0 odd the item pitch of a batch is odd
# hop-1 frontier per batch.  Three rows (stage_sort_blocks = 3) walk batches r, r + 3, r + 6, r + 9: row 0 ends on an empty
# frontier (batch 9) with its carries full of batch 6's tail; 2 047 + 2 049 + 4 096 = 8 192 = the second level's step
TARGETS = [2047, 2048, 2049, 4095, 4096, 4097, 1, 7, 8, 0]


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def world(cabi):
    n0, V, iso0, ptrs, idx, g = _graph(cabi)
    deg = (ptrs[1:] - ptrs[:-1])[:n0]
    heavy = torch.nonzero(deg >= K0).flatten()
    assert heavy.numel() >= B
    gen = torch.Generator(device=DEV).manual_seed(91)
    seeds = torch.empty((len(TARGETS), B), dtype=torch.int64, device=DEV)
    for j, t in enumerate(TARGETS):
        m, r = divmod(t, K0)
        row = torch.arange(iso0, iso0 + B, device=DEV)                    # isolated: no item
        row[:m] = heavy[torch.randperm(heavy.numel(), device=DEV, generator=gen)[:m]]
        if r:
            exact = torch.nonzero(deg == r).flatten()
            assert exact.numel() > 0
            row[m] = exact[j % exact.numel()]
        seeds[j] = row[torch.randperm(B, device=DEV, generator=gen)]      # the degree-r and isolated seeds anywhere
    seeds = seeds.contiguous()
    refs = {}

    def reference(fan):
        """the fused kernel's output, once per fan-out, checked against the oracle"""
        key = tuple(fan)
        if key not in refs:
            ref = _poisoned(cabi, len(TARGETS), B, fan)
            cabi.ns_homo_batched(g, seeds, fan, SEED, CALL0, ref, form=FUSED)
            torch.cuda.synchronize()
            assert_oracle(cabi, ref, ptrs, idx, seeds, fan, SEED, CALL0, (0, 5, 9))
            refs[key] = ref
        return refs[key]

    return dict(n0=n0, ptrs=ptrs, idx=idx, g=g, seeds=seeds, reference=reference)


def _staged(cabi, g, seeds, fan, call0, **knobs):
    nb, n_seeds = seeds.shape
    dev = torch.device(DEV)
    before = cabi.ns_win_tuning_set(window_bytes=1 << 14, staged=1, **knobs)
    try:
        ws = cabi.ns_homo_workspace(nb, n_seeds, fan, dev, staged=True, graph=g)
        out = _poisoned(cabi, nb, n_seeds, fan)
        assert cabi.ns_homo_batched_staged(g, out, nb, n_seeds, fan, ws=ws, form=WINDOWED) is True
        cabi.ns_homo_batched(g, seeds, fan, SEED, call0, out, ws=ws, form=WINDOWED)
        torch.cuda.synchronize()
    finally:
        cabi.ns_win_tuning_set(**before)
    return out


@pytest.mark.gpu
def test_frontiers_are_what_the_cases_need(cabi, world):
    ref = world["reference"]([K0, 10])
    assert (ref.layer_offsets[:, 1, 0] - B).tolist() == TARGETS
    assert sum(TARGETS[i] for i in (0, 2, 4)) == 8192


# rows: 3 = fewer rows than batches (the carries live across batches; row 0 ends on the empty frontier), 1 = one row takes
# every batch (18 448 items = two steps of the second level and a rest), 64 = asked for more rows than batches, -1 = auto;
# stage_fine = 0: the gather reads the level-1 output itself; stage_fine_blocks = 1: one workgroup loops over all steps
@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(stage_sort_blocks=3), dict(stage_sort_blocks=1), dict(stage_sort_blocks=64),
                                   dict(stage_sort_blocks=-1), dict(stage_sort_blocks=3, stage_fine=0),
                                   dict(stage_sort_blocks=3, stage_fine_blocks=1),
                                   dict(stage_sort_blocks=3, stage_split=1),
                                   dict(stage_sort_blocks=3, stage_parts=2, stage_part_min_batches=1, stage_concurrent=1)],
                         ids=["rows3", "rows1", "rows64", "auto", "nofine", "fine1block", "split", "concurrent"])
def test_tile_edges_equal_fused(cabi, world, knobs):
    fan = [K0, 10]
    ref = world["reference"](fan)
    out = _staged(cabi, world["g"], world["seeds"], fan, CALL0, **knobs)
    assert_equal_on_device(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [3, -1])
def test_second_part_starts_on_an_odd_element(cabi, world, rows):
    """two parts: the second part's level-1 output starts at item 5 * 281 * 15 of the array -- 8-byte but not 64-byte
    aligned, so its chunk boundaries are not the index's multiples of 8"""
    fan = [K0, 10]
    assert (len(TARGETS) // 2 * B * K0) % 8 != 0
    ref = world["reference"](fan)
    out = _staged(cabi, world["g"], world["seeds"], fan, CALL0, stage_sort_blocks=rows, stage_parts=2, stage_part_min_batches=1,
                  stage_concurrent=0)
    assert_equal_on_device(out, ref)
    assert_oracle(cabi, out, world["ptrs"], world["idx"], world["seeds"], fan, SEED, CALL0, (4, 5, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("fan", [[K0, 3, 2], [K0, 10, 2]], ids=["15x3x2", "15x10x2"])
def test_three_hops_feed_level_one_through_the_histogram_pass(cabi, world, fan):
    """hops beyond the second count their items in win_hist8_kernel; [15, 10, 2]: third frontiers of up to 40 970 items"""
    ref = world["reference"](fan)
    for rows in (3, -1):
        out = _staged(cabi, world["g"], world["seeds"], fan, CALL0, stage_sort_blocks=rows)
        assert_equal_on_device(out, ref)


@pytest.mark.gpu
def test_one_batch_and_batches_of_isolated_seeds(cabi, world):
    fan = [K0, 10]
    ref = world["reference"](fan)
    for j in (5, 9):                                                     # 4 097 items; none at all
        out = _staged(cabi, world["g"], world["seeds"][j:j + 1].contiguous(), fan, CALL0 + j)
        sub = _poisoned(cabi, 1, B, fan)
        cabi.ns_homo_batched(world["g"], world["seeds"][j:j + 1].contiguous(), fan, SEED, CALL0 + j, sub, form=FUSED)
        torch.cuda.synchronize()
        assert torch.equal(sub.counts, ref.counts[j:j + 1])
        assert_equal_on_device(out, sub)


@pytest.mark.gpu
def test_many_small_batches_take_the_staged_pipeline_by_default(cabi):
    """2 048 batches of 8 seeds under the default tuning (staged = 2: the staged pipeline from 2 048 batches on): every row
    of the sort walks two or more batches of ~100 items, most buckets of a tile hold nothing or one item"""
    dev = torch.device(DEV)
    n, ptrs, idx, g = _rmat(cabi, 12)
    nb, n_seeds, fan = 2048 + 5, 8, [K0, 10]
    assert cabi.ns_win_tuning()["staged"] == 2
    seeds = cabi.seed_batches(0xBA7C4, 0, nb, n_seeds, n, dev)
    before = cabi.ns_win_tuning_set(window_bytes=1 << 14)
    try:
        ws = cabi.ns_homo_workspace(nb, n_seeds, fan, dev, graph=g)
        a, b = _poisoned(cabi, nb, n_seeds, fan), _poisoned(cabi, nb, n_seeds, fan)
        assert cabi.ns_homo_batched_staged(g, a, nb, n_seeds, fan, ws=ws, form=WINDOWED) is True
        cabi.ns_homo_batched(g, seeds, fan, SEED, CALL0, a, ws=ws, form=WINDOWED)
        cabi.ns_homo_batched(g, seeds, fan, SEED, CALL0, b, form=FUSED)
        torch.cuda.synchronize()
    finally:
        cabi.ns_win_tuning_set(**before)
    assert_equal_on_device(a, b)
    assert_oracle(cabi, a, ptrs, idx, seeds, fan, SEED, CALL0, (0, 1024, nb - 1))
