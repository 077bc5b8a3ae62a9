"""The walks (csrc/random_walk.hip) at the sizes where their launches change shape, on guarded, sentinel-filled buffers.

tg_tempo_random_walk picks 4, 2 or 1 wavefronts per workgroup from the column count L (4 up to 768, 2 up to 1 536) and
asks for up to 64 KiB of dynamic LDS (more than 48 KiB from L = 3 073); each wavefront keeps its walk at a pitch of 2 L
words, and a restart reads a random earlier column from there.  rw_node2vec_kernel stages 16 columns per walker and lets
the whole wavefront flush them.  edge_set_insert_kernel cuts the edge array into segments of 2 048 edges and finds an
edge's row by search between the rows of the segment's ends.  Walks compare word for word with the CPU oracle, the edge
set with NumPy.  Each case names, in its comment, the defect it would catch."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from helpers import has_edge, load_karate
from helpers_negative import GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu
SEED = 0xA11CE
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


def _to(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in arrs]


def _csr_rmat(scale, seed):
    n = 1 << scale
    row, col = orc.rmat_edges(scale, n * 16, seed)
    ptrs, idx, _ = orc.to_csr(np.stack([row, col]), n)
    return ptrs, idx, n


# ------------------------------------------------------------------------------------------------ tg_tempo_random_walk
def _tempo(cabi, dev_arrays, n, L, window, call_id, expect_rc=0):
    """The C call on two guarded [n, L] buffers -> (walks, walks_ts) as NumPy; a refused call must leave both untouched."""
    p_d, i_d, nt_d, et_d, s_d, st_d = dev_arrays
    walks, wts = Guarded(torch, DEV, n * L), Guarded(torch, DEV, n * L)
    rc = cabi.lib.tg_tempo_random_walk(C.byref(cabi.graph_view(p_d, i_d)), cabi.ptr(nt_d), cabi.ptr(et_d), cabi.ptr(s_d),
                                       cabi.ptr(st_d), C.c_int64(n), C.c_int64(L), C.c_int64(window[0]), C.c_int64(window[1]),
                                       C.byref(cabi.TgRng(SEED, call_id)), C.c_void_p(walks.ptr()), C.c_void_p(wts.ptr()),
                                       cabi.stream_ptr(torch.device(DEV)))
    torch.cuda.current_stream().synchronize()
    if expect_rc:
        assert rc == expect_rc
        assert (walks.numpy() == SENTINEL).all() and (wts.numpy() == SENTINEL).all(), "a refused call wrote its outputs"
        with pytest.raises(cabi.TchGeoError, match="exceeds the LDS walk buffer"):
            cabi.check(rc)
        return None
    cabi.check(rc)
    return walks.split("walks").reshape(n, L), wts.split("walks_ts").reshape(n, L)


@pytest.fixture(scope="module")
def karate_tempo():
    """Karate with the timestamps of test_gpu_walks.test_tempo_random_walk_karate and nine walkers: 9 is no multiple of 4
    or 2, so the last workgroup of either shape is short (its idle wavefronts must leave, not walk)."""
    ei, n = load_karate()
    ptrs, idx, _ = orc.to_csr(ei, n)
    g = np.random.default_rng(7)
    node_ts, edge_ts = g.integers(-1, 4, n), g.integers(-1, 4, len(idx))
    start = np.array([0, 1, 2, 3, 33, 5, 6, 8, 9], dtype=np.int64)
    start_ts = np.array([0, -1, 2, 3, 1, 0, 9, 1, 2], dtype=np.int64)
    host = (ptrs, idx, node_ts, edge_ts, start, start_ts)
    return host, _to(*host)


TEMPO_L = [768,    # the last L on 4 wavefronts: 48 KiB exactly, wave 3's walk ends at the last LDS word
           769,    # the first on 2 wavefronts: a pitch still computed for 4 puts wave 1 on top of wave 0's timestamps
           1536,   # the last on 2 wavefronts
           1537,   # the first on 1
           3072,   # 48 KiB for one wavefront: the most a launch gets without asking for more
           3073,   # the first launch above 48 KiB of dynamic LDS
           4096]   # 64 KiB, the largest walk the buffer holds


@pytest.mark.parametrize("L", TEMPO_L)
def test_tempo_walk_at_the_workgroup_shapes(cabi, karate_tempo, L):
    host, dev = karate_tempo
    ptrs, idx = host[0], host[1]
    rw, rwt = orc.tempo_random_walk(*host, L, (0, 2), orc.rng_philox(SEED, 3))
    # a restart copies (node, time) of a random earlier column: with a wrong pitch, or the start time in place of the
    # stored one, it differs only if restarts happen late, where that column is far from column 0
    late = [i for i in range(len(host[4]))
            if any(not has_edge(ptrs, idx, rw[i, c - 1], rw[i, c]) for c in range(3 * L // 4 + 1, L))]
    assert len(late) >= 3, late
    w, wt = _tempo(cabi, dev, 9, L, (0, 2), 3)
    assert np.array_equal(w, rw), "walks differ in rows %s" % np.flatnonzero((w != rw).any(1)).tolist()
    assert np.array_equal(wt, rwt), "timestamps differ"


def test_tempo_walk_of_4097_columns_is_refused(cabi, karate_tempo):
    """65 552 bytes for one wavefront: no launch, TG_ERR_UNSUPPORTED, both buffers as they were."""
    _tempo(cabi, karate_tempo[1], 9, 4097, (0, 2), 3, expect_rc=3)


def test_tempo_walk_rmat_full_and_short_workgroups_of_two_wavefronts(cabi):
    """701 walkers at L = 769: 350 full workgroups of 2 wavefronts and one with a single walker; hub rows stream in two
    chunks a round."""
    ptrs, idx, n = _csr_rmat(12, 5)
    g = np.random.default_rng(1)
    node_ts, edge_ts = g.integers(-1, 50, n), g.integers(-1, 50, len(idx))
    start = orc.seed_batches(1, 0, 1, 701, n)[0]
    start_ts = g.integers(-1, 40, 701)
    host = (ptrs, idx, node_ts, edge_ts, start, start_ts)
    rw, rwt = orc.tempo_random_walk(*host, 769, (0, 15), orc.rng_philox(SEED, 4))
    w, wt = _tempo(cabi, _to(*host), 701, 769, (0, 15), 4)
    assert np.array_equal(w, rw) and np.array_equal(wt, rwt)


# ------------------------------------------------------------------------------------------------ tg_random_walk(_es)
WALK_LENGTHS = [14,   # 15 columns: one ragged stage
                15,   # 16 columns: exactly one stage, no ragged one behind it
                16,   # 17: a second stage of a single column
                31,   # 32: two whole stages
                32]   # 33
WALKERS = [1, 63, 64, 65, 255, 256, 257]   # a wavefront and a workgroup, one short, exact, one over: the flush's tw < n


@pytest.fixture(scope="module")
def rmat13_host():
    ptrs, idx, n = _csr_rmat(13, 99)                     # test_gpu_walks.test_random_walk_rmat_with_dead_ends: many dead ends
    return ptrs, idx, orc.seed_batches(0x57A27, 0, 1, 257, n)[0]


@pytest.fixture(scope="module")
def rmat13(cabi, rmat13_host):
    ptrs, idx, start = rmat13_host
    p_d, i_d, s_d = _to(ptrs, idx, start)
    views = {"plain": cabi.graph_view(p_d, i_d),
             "u32 shadows": cabi.graph_view(p_d, i_d, indices32=i_d.to(torch.int32), ptrs32=p_d.to(torch.int32))}
    return ptrs, idx, start, s_d, views


def _walk(cabi, g, s_d, n, walk_length, pq, call_id, edge_set=None):
    L = walk_length + 1
    walks = Guarded(torch, DEV, n * L)
    rng, stream = cabi.TgRng(SEED, call_id), cabi.stream_ptr(torch.device(DEV))
    if edge_set is None:
        rc = cabi.lib.tg_random_walk(C.byref(g), cabi.ptr(s_d), C.c_int64(n), C.c_int64(walk_length), C.c_float(pq[0]),
                                     C.c_float(pq[1]), C.byref(rng), C.c_void_p(walks.ptr()), stream)
    else:
        rc = cabi.lib.tg_random_walk_es(C.byref(g), cabi.ptr(edge_set), C.c_int64(edge_set.numel() * 8), cabi.ptr(s_d),
                                        C.c_int64(n), C.c_int64(walk_length), C.c_float(pq[0]), C.c_float(pq[1]),
                                        C.byref(rng), C.c_void_p(walks.ptr()), stream)
    cabi.check(rc)
    torch.cuda.current_stream().synchronize()
    return walks.split("walks").reshape(n, L)


def _first_dead(w):
    """Per row the first column holding -1, or the row length."""
    dead = w == -1
    return np.where(dead.any(1), dead.argmax(1), w.shape[1])


def test_the_walk_cases_exercise_what_they_claim(rmat13_host):
    """On the oracle alone: -1 stands in a column that is a multiple of 16 and in the last column of some row; a walker
    dies exactly where a stage begins (column 16 or 32: the stage is all -1, and a u32 stage word of all ones must come out
    as -1, not 4 294 967 295) and one dies in the last column."""
    ptrs, idx, start = rmat13_host
    at_stage = at_last = in_stage_col = 0
    for wl in WALK_LENGTHS:
        for pq in ((1.0, 1.0), (2.0, 0.5)):
            ref = orc.random_walk(ptrs, idx, start, wl, pq[0], pq[1], orc.rng_philox(SEED, wl))
            first = _first_dead(ref)
            at_stage += int(((first % 16 == 0) & (first <= wl)).sum())
            at_last += int((first == wl).sum())
            in_stage_col += int((ref[:, 16::16] == -1).sum())
            assert (ref[:, -1] == -1).any() and (ref[:, -1] >= 0).any()
    assert in_stage_col > 0 and at_stage > 0 and at_last > 0


@pytest.mark.parametrize("pq", [(1.0, 1.0),    # every candidate accepted: int64 staging
                                (2.0, 0.5)])   # has_edge decides: u32 staging, where -1 is the all-ones word
@pytest.mark.parametrize("walk_length", WALK_LENGTHS)
def test_node2vec_walk_at_stage_wavefront_and_workgroup_edges(cabi, rmat13, walk_length, pq):
    ptrs, idx, start, s_d, views = rmat13
    es = cabi.edge_set(views["plain"], torch.device(DEV))
    for n in WALKERS:
        ref = orc.random_walk(ptrs, idx, start[:n], walk_length, pq[0], pq[1], orc.rng_philox(SEED, walk_length))
        for how in ("plain", "u32 shadows", "edge set"):
            g = views["plain" if how == "edge set" else how]
            w = _walk(cabi, g, s_d, n, walk_length, pq, walk_length, edge_set=es if how == "edge set" else None)
            assert np.array_equal(w, ref), (n, how)


# ------------------------------------------------------------------------------------------------ tg_edge_set_build
N_SET = 461


def _csr_of_degrees(deg, rng, n_cols=N_SET):
    """A CSR with these row lengths, random columns sorted inside each row (multi-edges allowed)."""
    deg = np.asarray(deg, dtype=np.int64)
    ptrs = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rows = np.repeat(np.arange(deg.size, dtype=np.int64), deg)
    cols = rng.integers(0, n_cols, rows.size)
    order = np.lexsort((cols, rows))
    return ptrs, cols[order].astype(np.int64)


def _spread(n_edges, rng):
    """n_edges over N_SET rows, the last row taking the remainder."""
    deg = rng.multinomial(n_edges, np.full(N_SET, 1.0 / N_SET))
    return _csr_of_degrees(deg, rng)


def _set_graph(name):
    rng = np.random.default_rng([0xED6E, sum(name.encode())])
    if name.startswith("edges="):                        # 1: one lane of one wavefront works; 2 047 / 2 048 / 2 049 / 4 097:
        return _spread(int(name[6:]), rng)               # a segment one short, exact, and a last segment of a single edge
    if name == "hub":
        # 10 rows of 30, 70 empty, a row of 5 000 (edges 300 .. 5 299: segments 0, 1 and 2, the middle one all hub, so
        # r0 == r1 there), 70 empty, 10 rows of 30, 300 empty: r0 / r1 must skip empty rows on either side of a cut, and
        # the search for the last edge must not run into the trailing empty rows, whose ptrs all equal n_edges
        deg = [30] * 10 + [0] * 70 + [5000] + [0] * 70 + [30] * 10 + [0] * 300
        assert len(deg) == N_SET
        return _csr_of_degrees(deg, rng)
    if name == "one edge across a cut":
        # row 0 holds 2 040 edges, row 1 the edge (1, 7) twenty times, over the cut at 2 048: both segments insert the
        # same key, and the set must hold it once
        ptrs, idx = _csr_of_degrees([2040, 20] + [3] * (N_SET - 2), rng)
        idx[2040:2060] = 7
        return ptrs, idx
    if name == "a row ends on a cut":
        # rows 0 .. 7 hold 256 edges each: edge 2 047 is the last of row 7, edge 2 048 the first of row 9 (row 8 is empty):
        # ptrs[r] <= e must send edge 2 048 past both
        return _csr_of_degrees([256] * 8 + [0] + [40] * 60 + [0] * (N_SET - 69), rng)
    raise KeyError(name)


SET_GRAPHS = ["edges=1", "edges=2047", "edges=2048", "edges=2049", "edges=4097", "hub", "one edge across a cut",
              "a row ends on a cut"]


def _build_set(cabi, ptrs, idx):
    """tg_edge_set_bytes + tg_edge_set_build on a guarded buffer of exactly that size -> (slots as uint64, device tensor)."""
    p_d, i_d = _to(ptrs, idx)
    g = cabi.graph_view(p_d, i_d)
    nbytes = C.c_int64(-1)
    cabi.check(cabi.lib.tg_edge_set_bytes(C.byref(g), C.byref(nbytes)))
    want = 64
    while want < 2 * idx.size:
        want *= 2
    assert nbytes.value == 8 * want
    buf = Guarded(torch, DEV, want)
    cabi.check(cabi.lib.tg_edge_set_build(C.byref(g), C.c_void_p(buf.ptr()), nbytes, cabi.stream_ptr(torch.device(DEV))))
    torch.cuda.current_stream().synchronize()
    slots = buf.split("the edge set").copy()
    return slots.view(np.uint64), buf.buf[GUARD:GUARD + want], g, (p_d, i_d)


@pytest.mark.parametrize("name", SET_GRAPHS)
def test_edge_set_holds_exactly_the_distinct_edges(cabi, name):
    ptrs, idx = _set_graph(name)
    slots, es, g, keep = _build_set(cabi, ptrs, idx)
    rows = np.repeat(np.arange(ptrs.size - 1), np.diff(ptrs)).astype(np.uint64)
    keys = np.unique((rows << np.uint64(32)) | idx.astype(np.uint64))
    empty = slots == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert np.array_equal(np.sort(slots[~empty]), keys)   # each key once, none under a wrong row, none missing
    if idx.size > 1:
        # has_edge answered from this set walks as has_edge by binary search does
        start = np.arange(ptrs.size - 1, dtype=np.int64)
        ref = orc.random_walk(ptrs, idx, start, 10, 2.0, 0.5, orc.rng_philox(SEED, 9))
        w = _walk(cabi, g, _to(start)[0], start.size, 10, (2.0, 0.5), 9, edge_set=es)
        assert np.array_equal(w, ref)


def test_edge_set_of_no_edges(cabi):
    """n_edges = 0 with n_major = 5: 64 slots, all empty, nothing inserted, nothing read through the null indices."""
    slots, _, _, _ = _build_set(cabi, np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert slots.size == 64 and (slots == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
