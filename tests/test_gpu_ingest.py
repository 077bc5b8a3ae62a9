"""Device ingest (tg_coo_to_csx, csrc/ingest.hip) at the C ABI, word for word against tests/helpers_ingest.py.

Every other GPU test builds its graph with this call and most hand the result to the oracle as well, so a wrong ingest
feeds the device and its yardstick the same wrong graph.  Here the test owns every buffer: `ptrs`, `indices` and `perm`
sit between 16 guard words in front and behind, pre-filled with a value that is no valid output, the workspace is exactly
the number of bytes the query returns with guard bytes behind it, and all three outputs must equal the restatement
(proven on the CPU in tests/test_ingest_cpu.py) exactly.  Each case names, in its comment, the defect it would catch.
Out-of-range ids never reach tg_coo_to_csx (its contract leaves them unchecked); they go to the surface, which refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_ingest as hi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16
SENTINEL = -0x5A5A5A5A5A5A5A5B          # negative: no pointer, index or edge position


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


@pytest.fixture(scope="module")
def tg():
    import tch_geometric
    return tch_geometric


class Guarded:
    """n int64 words between GUARD sentinel words on either side; the payload starts as sentinels too, so a word the call
    leaves unwritten cannot equal the restatement."""

    def __init__(self, n, fill=SENTINEL, dtype=torch.int64):
        self.fill = fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def assert_guards(self):
        assert bool((self.buf[:GUARD] == self.fill).all()), "words in front of the output were written"
        assert bool((self.buf[GUARD + self.view.numel():] == self.fill).all()), "words behind the output were written"

    def numpy(self):
        return self.view.cpu().numpy()


def device_csx(cabi, row, col, size0, size1, csc, null_inputs=False):
    """tg_coo_to_csx on guarded outputs and a workspace of exactly the queried size -> (ptrs, indices, perm) as NumPy."""
    dev = torch.device(DEV)
    nnz, m = int(row.numel()), size1 if csc else size0
    ptrs, indices, perm = Guarded(m + 1), Guarded(nnz), Guarded(nnz)
    nbytes = C.c_int64(-1)
    cabi.check(cabi.lib.tg_coo_to_csx_workspace_bytes(C.c_int64(nnz), C.c_int64(size0), C.c_int64(size1), C.byref(nbytes)))
    assert nbytes.value >= 24 * nnz
    ws = torch.full((nbytes.value + 128,), 0xA5, dtype=torch.uint8, device=dev)
    null = C.c_void_p(0)
    if null_inputs:
        assert nnz == 0
        args = (null, null, ptrs.ptr(), null, null, null, C.c_int64(0))
    else:
        assert row.dtype == col.dtype == torch.int64 and row.is_contiguous() and col.is_contiguous() and nnz > 0
        args = (cabi.ptr(row), cabi.ptr(col), ptrs.ptr(), indices.ptr(), perm.ptr(), cabi.ptr(ws), C.c_int64(nbytes.value))
    rc = cabi.lib.tg_coo_to_csx(args[0], args[1], C.c_int64(nnz), C.c_int64(size0), C.c_int64(size1), C.c_int32(int(csc)),
                                args[2], args[3], args[4], args[5], args[6], cabi.stream_ptr(dev))
    cabi.check(rc)
    torch.cuda.current_stream(dev).synchronize()
    for g in (ptrs, indices, perm):
        g.assert_guards()
    assert bool((ws[nbytes.value:] == 0xA5).all()), "bytes behind the workspace were written"
    return ptrs.numpy(), indices.numpy(), perm.numpy()


def assert_ingest(cabi, row, col, size0, size1, csc):
    """row, col: NumPy int64, every id inside the graph (asserted: the C call does not check)."""
    row, col = np.ascontiguousarray(row, dtype=np.int64), np.ascontiguousarray(col, dtype=np.int64)
    assert row.size == col.size and row.size > 0
    assert 0 <= int(row.min()) and int(row.max()) < size0 and 0 <= int(col.min()) and int(col.max()) < size1
    got = device_csx(cabi, torch.from_numpy(row).to(DEV), torch.from_numpy(col).to(DEV), size0, size1, csc)
    want = hi.to_csx(row, col, size0, size1, csc)
    for name, g, w in zip(("ptrs", "indices", "perm"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), "%s differs from the restatement" % name
    return want


def _rng(*key):
    return np.random.default_rng([0x1A9E57] + [int(k) for k in key])


# ------------------------------------------------------------------ sort paths
# rocPRIM picks its algorithm by size: one block sort, merge sort up to 1 048 576 items, onesweep above.
SORT_NNZ = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097,     # block sort at its wavefront / tile edges: a ragged tail dropped
            65537,                                                  # merge sort over many blocks: a last block of one item lost
            1048575, 1048576, 1048577,                              # the last merge sort, the first onesweep: scratch sized for
                                                                    # one algorithm and used by the other, an unstable merge
            3000001]                                                # onesweep over several blocks, ragged last one: its tail
                                                                    # scattered with a stale digit offset, ties reordered


@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("nnz", SORT_NNZ)
def test_sort_paths(cabi, nnz, csc):
    rng = _rng(1, nnz)
    assert_ingest(cabi, rng.integers(0, 1000, nnz), rng.integers(0, 1000, nnz), 1000, 1000, csc)


# ------------------------------------------------------------------ rectangular graphs
@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("size0,size1", [(1000, 7), (7, 1000),   # size_minor / size_major swapped in the indices or ptrs kernel
                                         (1, 5000), (5000, 1),   # ... where one side has a single id: `% size` gives all zeros
                                         (1025, 1023)])          # col * size1 + row for col * size0 + row: off by little
def test_rectangular(cabi, size0, size1, csc):
    rng = _rng(2, size0, size1)
    row, col = rng.integers(0, size0, 50000), rng.integers(0, size1, 50000)
    longer = row if size0 > size1 else col
    assert int(longer.max()) >= min(size0, size1)                   # an id only the longer side can hold: a swap cannot pass
    ptrs, _, _ = assert_ingest(cabi, row, col, size0, size1, csc)
    assert ptrs.size == (size1 if csc else size0) + 1


@pytest.mark.parametrize("csc", [True, False])
def test_rectangular_rmat_generator_as_input(cabi, csc):
    """2^20 x 2^9 R-MAT edges made on the device (what the typed benchmarks ingest), 2^21 + 3 of them: onesweep on a
    rectangle.  The oracle has no twin of the rectangular generator, so the restatement is the only yardstick."""
    row, col = cabi.rmat_edges_rect(20, 9, (1 << 21) + 3, 0x5EED, torch.device(DEV))
    hrow, hcol = row.cpu().numpy(), col.cpu().numpy()
    assert 0 <= hrow.min() and hrow.max() < (1 << 20) and 0 <= hcol.min() and hcol.max() < (1 << 9)
    assert hrow.max() >= (1 << 9)                                   # a size swap cannot pass
    got = device_csx(cabi, row, col, 1 << 20, 1 << 9, csc)
    want = hi.to_csx(hrow, hcol, 1 << 20, 1 << 9, csc)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------ key width
def _top_bit(product):
    return max((product - 1).bit_length(), 1) - 1


@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("size0,size1,product", [
    (1 << 10, 1 << 10, 1 << 20),          # a power of two: 20 bits exactly; one bit fewer leaves the upper half unsorted
    (1024, 1025, (1 << 20) + 1024),       # just above: the 21st bit is needed for 1 024 keys only
    (1023, 1025, (1 << 20) - 1),          # just below: 20 bits, every one of them used
    (3, 5, 15)])                          # 4 bits: a minimum key width of the sort larger than the keys
def test_key_width(cabi, size0, size1, product, csc):
    assert size0 * size1 == product
    rng = _rng(3, size0, size1)
    row, col = rng.integers(0, size0, 30000), rng.integers(0, size1, 30000)
    row[7], col[7] = size0 - 1, size1 - 1                           # the largest key of the graph
    keys = hi.keys_of(row, col, size0, size1, csc)
    assert int(keys.max()) == product - 1 and (int(keys.max()) >> _top_bit(product)) == 1
    assert int((keys >> _top_bit(product) == 0).sum()) > 0          # and keys without it: dropping the bit reorders
    assert_ingest(cabi, row, col, size0, size1, csc)


@pytest.mark.parametrize("csc", [True, False])
def test_key_width_one_by_one(cabi, csc):
    """1 x 1 with 100 self loops: zero key bits are needed (the sort is asked for one); perm is the identity"""
    z = np.zeros(100, dtype=np.int64)
    ptrs, indices, perm = assert_ingest(cabi, z, z, 1, 1, csc)
    assert ptrs.tolist() == [0, 100] and perm.tolist() == list(range(100)) and not indices.any()


def _wide_ids(rng, n, long_side):
    """ids over [0, long_side): the low end, the high end and everything between, the last id among them"""
    ids = np.concatenate([rng.integers(0, 1000, n // 3), long_side - 1 - rng.integers(0, 1000, n // 3),
                          rng.integers(0, long_side, n - 2 * (n // 3))])
    ids[0] = long_side - 1
    return rng.permutation(ids)


@pytest.mark.parametrize("size0,size1,csc,nnz,product,bits", [
    (1 << 40, 1000, True, 50000, 1000 << 40, 50),    # 50-bit keys: a key built or compared in 32 bits, passes past bit 32 lost
    (1000, 1 << 40, False, 50000, 1000 << 40, 50),   # the same through the CSR branch (row * size1 + col)
    (1 << 52, 1024, True, 100000, 1 << 62, 62)])     # 62-bit keys, the widest whose ptrs fit: `j * size_minor` near 2^63
def test_wide_keys(cabi, size0, size1, csc, nnz, product, bits):
    """one orientation each: the other one's ptrs would have 2^40 words"""
    assert size0 * size1 == product and _top_bit(product) == bits - 1
    rng = _rng(4, bits, csc)
    minor = _wide_ids(rng, nnz, max(size0, size1))
    major = rng.integers(0, min(size0, size1), nnz)
    major[int(np.argmax(minor))] = min(size0, size1) - 1            # the graph's largest key: top valid bit set
    row, col = (minor, major) if csc else (major, minor)
    keys = hi.keys_of(row, col, size0, size1, csc)
    assert int(keys.max()) == product - 1 and (int(keys.max()) >> (bits - 1)) == 1
    assert int(minor.min()) < 1000 and int(minor.max()) == max(size0, size1) - 1
    ptrs, indices, _ = assert_ingest(cabi, row, col, size0, size1, csc)
    assert ptrs.size == min(size0, size1) + 1 and int(indices.max()) == max(size0, size1) - 1


# ------------------------------------------------------------------ stability
@pytest.mark.parametrize("csc", [True, False])
def test_stability_one_edge_many_times(cabi, csc):
    """200 000 copies of one edge: only a stable sort returns the identity (merge-sort path)"""
    n = 200000
    _, _, perm = assert_ingest(cabi, np.full(n, 3), np.full(n, 5), 9, 7, csc)
    assert np.array_equal(perm, np.arange(n))


@pytest.mark.parametrize("csc", [True, False])
def test_stability_on_onesweep(cabi, csc):
    """1 500 000 edges over 1 000 distinct pairs: the only case where stability decides perm on the onesweep path"""
    rng = _rng(5)
    prow, pcol = rng.integers(0, 300, 1000), rng.integers(0, 200, 1000)
    pick = rng.integers(0, 1000, 1500000)
    row, col = prow[pick], pcol[pick]
    assert np.unique(hi.keys_of(row, col, 300, 200, csc)).size <= 1000
    _, _, perm = assert_ingest(cabi, row, col, 300, 200, csc)
    keys = hi.keys_of(row, col, 300, 200, csc)[perm]
    assert bool(np.all((np.diff(keys) > 0) | (np.diff(perm) > 0)))  # inside a run of equal keys positions ascend


@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("order", ["sorted", "reversed"])
def test_presorted_inputs(cabi, order, csc):
    """already sorted: perm is the identity; reversed, with parallel edges: equal keys must NOT be reversed back"""
    rng = _rng(6)
    row, col = rng.integers(0, 211, 70000), rng.integers(0, 97, 70000)
    by_key = np.argsort(hi.keys_of(row, col, 211, 97, csc), kind="stable")
    if order == "reversed":
        by_key = by_key[::-1]
    row, col = row[by_key], col[by_key]
    assert np.unique(hi.keys_of(row, col, 211, 97, csc)).size < 70000          # there are parallel edges
    _, _, perm = assert_ingest(cabi, row, col, 211, 97, csc)
    if order == "sorted":
        assert np.array_equal(perm, np.arange(70000))


# ------------------------------------------------------------------ column structure
def _by_orientation(major, minor, csc):
    return (minor, major) if csc else (major, minor)


@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("shape", ["first", "last", "gap70", "hub", "m1"])
def test_column_structure(cabi, shape, csc):
    rng = _rng(7, ["first", "last", "gap70", "hub", "m1"].index(shape))
    m, size_minor, n = 1000, 613, 40000
    if shape == "first":       # every edge in column 0: the lower bound of every later column must run to nnz
        major = np.zeros(n, dtype=np.int64)
    elif shape == "last":      # every edge in the last column: ptrs[0..m-1] all 0, a search that never returns 0 fails
        major = np.full(n, m - 1)
    elif shape == "gap70":     # 70 empty columns in a row: their ptrs repeat one value
        major = rng.integers(0, m - 70, n)
        major = np.where(major >= 400, major + 70, major)
    elif shape == "hub":       # a hub of 300 000 edges beside columns of one edge: a search window sized by an average
        major = np.concatenate([np.full(300000, 500), np.arange(m)])
        major = rng.permutation(major)
        n = major.size
    else:                      # m = 1: ptrs is [0, nnz]; the ptrs grid has two live threads
        m, major = 1, np.zeros(n, dtype=np.int64)
    minor = rng.integers(0, size_minor, n)
    row, col = _by_orientation(major, minor, csc)
    size0, size1 = _by_orientation(m, size_minor, csc)
    ptrs, _, _ = assert_ingest(cabi, row, col, size0, size1, csc)
    deg = np.diff(ptrs)
    if shape == "gap70":
        assert not deg[400:470].any() and deg[399] > 0 and deg[470] > 0
    if shape == "hub":
        assert deg[500] == 300001 and np.all(np.delete(deg, 500) == 1)
    if shape == "m1":
        assert ptrs.tolist() == [0, n]


# ------------------------------------------------------------------ nnz = 0
@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 100000])
def test_no_edges(cabi, m, csc):
    """ptrs is m + 1 zeros (a memset of m words, or of m + 1 ints, shows); every other pointer is null and not needed"""
    size0, size1 = _by_orientation(m, 3, csc)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    ptrs, indices, perm = device_csx(cabi, empty, empty, size0, size1, csc, null_inputs=True)
    assert ptrs.shape == (m + 1,) and not ptrs.any() and indices.size == 0 and perm.size == 0


# ------------------------------------------------------------------ stream
@pytest.mark.parametrize("csc", [True, False])
def test_non_default_stream(cabi, csc):
    """every launch and the sort take the caller's stream: one left on the null stream races the others"""
    rng = _rng(8)
    row, col = rng.integers(0, 1000, 1200000), rng.integers(0, 7, 1200000)
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        assert cabi.stream_ptr(torch.device(DEV)).value == stream.cuda_stream != 0
        assert_ingest(cabi, row, col, 1000, 7, csc)
    stream.synchronize()


# ------------------------------------------------------------------ the surface: tch_geometric.to_csc / to_csr
def _surface(tg, csc):
    return tg.to_csc if csc else tg.to_csr


@pytest.mark.parametrize("where", ["cpu", "cuda:0"])
@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("size", [(1000, 7), (7, 1000)])
def test_surface_tuple_size(tg, size, csc, where):
    """a tuple size reaches the kernels in the right order, from a CPU and from a device tensor, results on its device"""
    rng = _rng(9, *size)
    row, col = rng.integers(0, size[0], 20000), rng.integers(0, size[1], 20000)
    assert max(int(row.max()), int(col.max())) >= min(size)
    got = _surface(tg, csc)(torch.from_numpy(np.stack([row, col])).to(where), size)
    for g, w in zip(got, hi.to_csx(row, col, size[0], size[1], csc)):
        assert str(g.device) == where and g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("where", ["cpu", "cuda:0"])
@pytest.mark.parametrize("csc", [True, False])
def test_surface_no_edges(tg, csc, where):
    ptrs, indices, perm = _surface(tg, csc)(torch.zeros((2, 0), dtype=torch.int64, device=where), (5, 9))
    assert ptrs.cpu().tolist() == [0] * ((9 if csc else 5) + 1) and indices.numel() == 0 and perm.numel() == 0
    assert str(ptrs.device) == str(indices.device) == str(perm.device) == where


BAD_IDS = [("row_is_size0", 0, 1000), ("col_is_size1", 1, 7), ("negative_row", 0, -1), ("negative_col", 1, -1)]


@pytest.mark.parametrize("csc", [True, False])
@pytest.mark.parametrize("name,side,value", BAD_IDS)
def test_surface_refuses_ids_outside_the_graph(tg, name, side, value, csc):
    """the range check stands between a bad id and the sort: `>` for `>=`, a check against the other side's size, a first
    or last element skipped"""
    rng = _rng(10)
    for where in ("cpu", "cuda:0"):
        for at in (0, 4999):
            rc = np.stack([rng.integers(0, 1000, 5000), rng.integers(0, 7, 5000)])
            rc[side, at] = value
            with pytest.raises(IndexError, match="outside the graph"):
                _surface(tg, csc)(torch.from_numpy(rc).to(where), (1000, 7))
    # the largest valid ids on both sides, in the same places, are accepted
    rc = np.stack([rng.integers(0, 1000, 5000), rng.integers(0, 7, 5000)])
    rc[0, [0, 4999]], rc[1, [0, 4999]] = 999, 6
    ptrs, _, _ = _surface(tg, csc)(torch.from_numpy(rc).to(DEV), (1000, 7))
    assert int(ptrs[-1]) == 5000


@pytest.mark.parametrize("name,side,value", BAD_IDS)
def test_surface_refuses_one_bad_id_among_three_million(tg, name, side, value):
    """3 000 000 ids are more than the check's 8 192 x 256 threads: the bad one sits in the grid-stride tail"""
    n = 3000000
    rc = torch.zeros((2, n), dtype=torch.int64, device=DEV)
    rc[0] = torch.arange(n, device=DEV) % 1000
    rc[1] = torch.arange(n, device=DEV) % 7
    at = n - 12345
    assert at > 8192 * 256
    rc[side, at] = value
    with pytest.raises(IndexError, match="outside the graph"):
        tg.to_csc(rc, (1000, 7))


@pytest.mark.parametrize("csc", [True, False])
def test_surface_value_errors(tg, csc):
    good = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        _surface(tg, csc)(torch.zeros((3, 4), dtype=torch.int64, device=DEV), 5)
    with pytest.raises(ValueError):
        _surface(tg, csc)(good, 0)
    with pytest.raises(ValueError):
        _surface(tg, csc)(good, (5, 0))
    with pytest.raises(ValueError):
        _surface(tg, csc)(good, (0, 5))
