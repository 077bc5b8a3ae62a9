"""The yardstick of tests/test_gpu_ingest.py and tests/test_gpu_index_plumbing.py, proven without a device: the NumPy
restatements of tests/helpers_ingest.py against brute force written from the header's sentences and against the oracle,
and every refusal of the ingest / index entry points that is decided before a launch (fake or null pointers only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers_ingest as hi
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")
TG_OK, TG_ERR_INVALID = 0, 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    so = C.CDLL(LIB)
    so.tg_last_error.restype = C.c_char_p
    return so


def i64(v):
    return C.c_int64(v)


# ------------------------------------------------------------------ restatement against brute force and the oracle
def _cases():
    """200 small COO graphs: (name, row, col, size0, size1).  The named ones first, then random rectangles."""
    rng = np.random.default_rng(0x1A9E57)
    z = np.zeros(0, dtype=np.int64)
    out = [("nnz0", z, z, 5, 3), ("nnz0_1x1", z, z, 1, 1),
           ("nnz1", np.array([2]), np.array([1]), 4, 3),
           ("nnz1_corner", np.array([3]), np.array([2]), 4, 3),                 # the largest key of the rectangle
           ("all_equal", np.full(17, 2), np.full(17, 4), 3, 6),                 # stability alone decides perm
           ("size0_is_1", np.zeros(9, dtype=np.int64), rng.integers(0, 7, 9), 1, 7),
           ("size1_is_1", rng.integers(0, 7, 9), np.zeros(9, dtype=np.int64), 7, 1),
           ("empty_first_last_col", rng.integers(0, 6, 30), rng.integers(1, 8, 30), 6, 9),
           ("empty_first_last_row", rng.integers(1, 5, 30), rng.integers(0, 9, 30), 6, 9),
           ("self_loops_1x1", np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64), 1, 1)]
    while len(out) < 200:
        size0, size1 = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        nnz = int(rng.integers(0, 40))
        row, col = rng.integers(0, size0, nnz), rng.integers(0, size1, nnz)
        if len(out) % 3 == 0 and nnz:                                           # duplicate-free: the oracle's perm is defined
            flat = rng.permutation(size0 * size1)[:min(nnz, size0 * size1)]
            row, col = flat % size0, flat // size0
        out.append(("random%d" % len(out), row, col, size0, size1))
    return [(n, np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64), s0, s1) for n, r, c, s0, s1 in out]


CASES = _cases()


def brute_to_csx(row, col, size0, size1, csc):
    """Python ints only: sort (key, position) tuples, then count the entries of every major id below j."""
    row, col = [int(x) for x in row], [int(x) for x in col]
    major, minor, m = (col, row, size1) if csc else (row, col, size0)
    size_minor = size0 if csc else size1
    pairs = sorted((major[e] * size_minor + minor[e], e) for e in range(len(row)))
    perm = [e for _, e in pairs]
    indices = [minor[e] for e in perm]
    ptrs = []
    for j in range(m + 1):
        n = 0
        for e in range(len(row)):
            n += major[e] < j
        ptrs.append(n)
    return ptrs, indices, perm


def test_case_list_covers_what_it_claims():
    assert len(CASES) == 200
    assert any(s0 != s1 for _, _, _, s0, s1 in CASES) and any(s0 > s1 for _, _, _, s0, s1 in CASES)
    assert any(s0 < s1 for _, _, _, s0, s1 in CASES)
    assert any(r.size == 0 for _, r, _, _, _ in CASES) and any(r.size == 1 for _, r, _, _, _ in CASES)
    assert sum(1 for _, r, c, s0, _ in CASES if r.size > 1 and np.unique(c * s0 + r).size == r.size) >= 30
    assert sum(1 for _, r, c, s0, _ in CASES if np.unique(c * s0 + r).size < r.size) >= 30


@pytest.mark.parametrize("csc", [True, False])
def test_to_csx_restatement_against_brute_force(csc):
    for name, row, col, size0, size1 in CASES:
        ptrs, indices, perm = hi.to_csx(row, col, size0, size1, csc)
        bp, bi, bperm = brute_to_csx(row, col, size0, size1, csc)
        assert ptrs.dtype == indices.dtype == perm.dtype == np.int64, name
        assert ptrs.tolist() == bp and indices.tolist() == bi and perm.tolist() == bperm, name


@pytest.mark.parametrize("csc", [True, False])
def test_to_csx_restatement_against_the_oracle(csc):
    compared_perm = 0
    for name, row, col, size0, size1 in CASES:
        ptrs, indices, perm = hi.to_csx(row, col, size0, size1, csc)
        op, oi, operm = orc.to_csx(np.stack([row, col]), (size0, size1), csc)
        assert np.array_equal(ptrs, op) and np.array_equal(indices, oi), name
        keys = hi.keys_of(row, col, size0, size1, csc)
        if np.unique(keys).size == keys.size:      # the reference's argsort is not stable: perm is defined without ties only
            assert np.array_equal(perm, operm), name
            compared_perm += 1
    assert compared_perm >= 30


def test_to_csx_restatement_refuses_a_key_past_int64():
    with pytest.raises(AssertionError):
        hi.to_csx(np.array([0]), np.array([1]), 1 << 62, 2, True)     # size0 * size1 = 2^63


def test_ind2ptr_restatement():
    rng = np.random.default_rng(7)
    assert hi.ind2ptr([3, 3, 3, 4, 4, 7, 7, 8, 8], 10).tolist() == [0, 0, 0, 0, 3, 5, 5, 5, 7, 9, 9]   # storage.rs:152-163
    for t in range(100):
        m = int(rng.integers(0, 20))
        ind = np.sort(rng.integers(0, max(m, 1), int(rng.integers(0, 50)))).astype(np.int64) if m else np.zeros(0, np.int64)
        want = [sum(1 for x in ind.tolist() if x < j) for j in range(m + 1)]
        assert hi.ind2ptr(ind, m).tolist() == want
        assert np.array_equal(hi.ind2ptr(ind, m), orc.ind2ptr(ind, m))
    # entries >= m (the oracle, like the reference, would write out of bounds there): the counting rule still holds
    ind = np.array([0, 2, 2, 5, 9, 9], dtype=np.int64)
    assert hi.ind2ptr(ind, 4).tolist() == [sum(1 for x in ind.tolist() if x < j) for j in range(5)] == [0, 1, 1, 3, 3]


def test_small_restatements_against_loops():
    rng = np.random.default_rng(11)
    assert hi.max_degree([0]) == 0 and hi.max_degree([0, 0, 0]) == 0 and hi.max_degree([0, 2, 2, 9, 10]) == 7
    for lo, hi_ in ((0, 10), (5, 6), (-3, 3)):
        for v in ([lo], [hi_ - 1], [lo - 1], [hi_], [hi.I64_MIN], [hi.I64_MAX], [lo, hi_ - 1], [lo, hi_, lo], []):
            bad = [not (lo <= x < hi_) for x in v]
            assert hi.check_range(v, lo, hi_) == any(bad)
            out, flag = hi.sanitize_range(v, lo, hi_)
            assert out.tolist() == [lo if b else x for x, b in zip(v, bad)] and flag == any(bad)
    slab = rng.integers(0, 1 << 40, (5, 7))
    lens = np.array([0, 7, 3, 0, 1])
    assert hi.compact_rows(slab, lens).tolist() == [int(slab[r, i]) for r in range(5) for i in range(int(lens[r]))]
    assert hi.compact_rows(np.zeros((0, 4), dtype=np.int64), np.zeros(0, dtype=np.int64)).size == 0
    src = rng.integers(0, 256, 6 * 11 + 3).astype(np.uint8)             # 6 rows of 9 bytes, 11 apart
    index = np.array([5, -1, 0, 6, 3, hi.I64_MIN, 3])
    dst, status = hi.gather_rows(src, 6, 9, 11, index)
    want = []
    for f in index.tolist():
        want += [int(src[f * 11 + k]) for k in range(9)] if 0 <= f < 6 else [0] * 9
    assert dst.tolist() == want and status == 1
    assert hi.gather_rows(src, 6, 9, 11, np.array([0, 5]))[1] == 0
    dst, status = hi.gather_rows(np.zeros(0, dtype=np.uint8), 0, 4, 4, np.arange(5))
    assert dst.tolist() == [0] * 20 and status == 1


# ------------------------------------------------------------------ refusals decided before any launch
def _refused(lib, rc, word):
    assert rc == TG_ERR_INVALID
    assert word in lib.tg_last_error(), lib.tg_last_error()


def test_workspace_query_refuses_keys_past_int64(lib):
    nbytes = C.c_int64(-1)
    for size0, size1 in ((1 << 32, 1 << 31), (1 << 62, 2), (2, 1 << 62), ((1 << 63) - 1, (1 << 63) - 1)):
        _refused(lib, lib.tg_coo_to_csx_workspace_bytes(i64(10), i64(size0), i64(size1), C.byref(nbytes)), b"overflows")
        assert nbytes.value == -1                                       # a refused call writes nothing
    # ... and tg_coo_to_csx itself refuses the same sizes before it looks at a buffer
    fake = C.c_void_p(4096)
    _refused(lib, lib.tg_coo_to_csx(fake, fake, i64(10), i64(1 << 32), i64(1 << 31), C.c_int32(1), fake, fake, fake, fake,
                                    i64(1 << 40), None), b"overflows")


def test_workspace_query_accepts_sizes_just_below_the_bound(lib):
    nbytes = C.c_int64(-1)
    for size0, size1 in ((1 << 31, (1 << 32) - 1), ((1 << 62) - 1, 2), ((1 << 63) - 1, 1), (1, (1 << 63) - 1)):
        assert size0 * size1 < (1 << 63)
        assert lib.tg_coo_to_csx_workspace_bytes(i64(10), i64(size0), i64(size1), C.byref(nbytes)) == TG_OK
        assert nbytes.value >= 24 * 10


def test_workspace_query_is_monotone_and_holds_three_arrays(lib):
    """keys, edge positions and sorted keys live in the workspace: 24 bytes an edge before the sort's own scratch"""
    nbytes, last = C.c_int64(-1), 0
    for nnz in (0, 1, 2, 63, 64, 65, 4096, 4097, 65537, 1048575, 1048576, 1048577, 3000001, 1 << 24, 1 << 28):
        assert lib.tg_coo_to_csx_workspace_bytes(i64(nnz), i64(1000), i64(1000), C.byref(nbytes)) == TG_OK
        assert nbytes.value >= 24 * nnz and nbytes.value >= last, nnz
        last = nbytes.value


def test_coo_to_csx_refuses_a_workspace_one_byte_short(lib):
    fake, nbytes = C.c_void_p(4096), C.c_int64(-1)
    for nnz in (1, 1000, 1048577):
        assert lib.tg_coo_to_csx_workspace_bytes(i64(nnz), i64(1000), i64(7), C.byref(nbytes)) == TG_OK
        _refused(lib, lib.tg_coo_to_csx(fake, fake, i64(nnz), i64(1000), i64(7), C.c_int32(1), fake, fake, fake, fake,
                                        i64(nbytes.value - 1), None), b"workspace too small")
        for which in range(5):                                          # a null row / col / indices / perm / workspace
            args = [fake] * 5
            args[which] = None
            _refused(lib, lib.tg_coo_to_csx(args[0], args[1], i64(nnz), i64(1000), i64(7), C.c_int32(1), fake, args[2],
                                            args[3], args[4], i64(nbytes.value), None), b"null buffers")


def test_workspace_query_refuses_bad_arguments(lib):
    nbytes = C.c_int64(-1)
    for nnz, size0, size1 in ((10, 0, 5), (10, 5, 0), (10, -1, 5), (-1, 5, 5)):
        _refused(lib, lib.tg_coo_to_csx_workspace_bytes(i64(nnz), i64(size0), i64(size1), C.byref(nbytes)), b"bad arguments")
    _refused(lib, lib.tg_coo_to_csx_workspace_bytes(i64(10), i64(5), i64(5), None), b"bad arguments")
    assert nbytes.value == -1


def test_coo_to_csx_refuses_bad_arguments(lib):
    fake = C.c_void_p(4096)

    def call(nnz=10, size0=5, size1=5, ptrs=fake, row=fake, ws=fake, ws_bytes=1 << 40):
        return lib.tg_coo_to_csx(row, fake, i64(nnz), i64(size0), i64(size1), C.c_int32(1), ptrs, fake, fake, ws,
                                 i64(ws_bytes), None)
    _refused(lib, call(ptrs=None), b"bad arguments")
    _refused(lib, call(nnz=-1), b"bad arguments")
    _refused(lib, call(size0=0), b"bad arguments")
    _refused(lib, call(size1=-3), b"bad arguments")


def test_other_entry_points_refuse_bad_arguments(lib):
    fake = C.c_void_p(4096)
    for lo, hi_ in ((3, 3), (4, 3), (0, 0), (0, -1)):                   # lo >= hi: no value to replace a bad one with
        _refused(lib, lib.tg_sanitize_range(fake, i64(4), i64(lo), i64(hi_), fake, fake, None), b"tg_sanitize_range")
    _refused(lib, lib.tg_sanitize_range(fake, i64(-1), i64(0), i64(3), fake, fake, None), b"tg_sanitize_range")
    _refused(lib, lib.tg_sanitize_range(fake, i64(4), i64(0), i64(3), fake, None, None), b"tg_sanitize_range")
    _refused(lib, lib.tg_sanitize_range(None, i64(4), i64(0), i64(3), fake, fake, None), b"tg_sanitize_range")
    _refused(lib, lib.tg_check_range(fake, i64(-1), i64(0), i64(3), fake, None), b"tg_check_range")
    _refused(lib, lib.tg_check_range(fake, i64(4), i64(0), i64(3), None, None), b"tg_check_range")
    _refused(lib, lib.tg_check_range(None, i64(4), i64(0), i64(3), fake, None), b"tg_check_range")
    for stride, pitch, n_rows in ((0, 8, 4), (-1, 8, 4), (1, -1, 4), (1, 8, -1), (1, 8, 1 << 31)):
        _refused(lib, lib.tg_compact_rows(fake, i64(pitch), fake, i64(stride), fake, i64(n_rows), fake, None), b"bad sizes")
    _refused(lib, lib.tg_compact_rows(fake, i64(8), fake, i64(1), fake, i64(4), None, None), b"null buffers")
    st = C.c_int32(0)
    _refused(lib, lib.tg_gather_rows(fake, i64(4), i64(16), i64(15), fake, i64(1), fake, C.byref(st), None), b"stride")
    for n_src, row_bytes, n in ((-1, 16, 1), (4, -1, 1), (4, 16, -1)):
        _refused(lib, lib.tg_gather_rows(fake, i64(n_src), i64(row_bytes), i64(16), fake, i64(n), fake, None, None),
                 b"negative size")
    _refused(lib, lib.tg_gather_rows(None, i64(4), i64(16), i64(16), fake, i64(1), fake, None, None), b"null buffer")
    _refused(lib, lib.tg_gather_rows(fake, i64(4), i64(16), i64(16), None, i64(1), fake, None, None), b"null buffer")
    _refused(lib, lib.tg_gather_rows(fake, i64(4), i64(16), i64(16), fake, i64(1), None, None, None), b"null buffer")
    assert st.value == 0
    _refused(lib, lib.tg_ind2ptr(fake, i64(3), i64(-1), fake, None), b"tg_ind2ptr")
    _refused(lib, lib.tg_ind2ptr(fake, i64(-1), i64(3), fake, None), b"tg_ind2ptr")
    _refused(lib, lib.tg_ind2ptr(None, i64(3), i64(3), fake, None), b"tg_ind2ptr")
    _refused(lib, lib.tg_ind2ptr(fake, i64(3), i64(3), None, None), b"tg_ind2ptr")
    _refused(lib, lib.tg_graph_max_degree(None, fake, None), b"tg_graph_max_degree")
    # empty calls are accepted with null pointers: nothing is launched
    assert lib.tg_check_range(None, i64(0), i64(0), i64(3), fake, None) == TG_OK
    assert lib.tg_sanitize_range(None, i64(0), i64(0), i64(3), None, fake, None) == TG_OK
    assert lib.tg_compact_rows(None, i64(0), None, i64(1), None, i64(0), None, None) == TG_OK
    assert lib.tg_gather_rows(None, i64(0), i64(16), i64(16), None, i64(0), None, None, None) == TG_OK
