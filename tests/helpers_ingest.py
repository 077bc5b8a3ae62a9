"""NumPy restatements of device ingest and the index plumbing around it (include/tchgeo.h: tg_coo_to_csx, tg_ind2ptr,
tg_graph_max_degree, tg_check_range, tg_sanitize_range, tg_compact_rows, tg_gather_rows), written from the header's rules
alone.  Nothing here imports the library under test: tests/test_ingest_cpu.py proves these functions against brute force
and the oracle on the CPU, the GPU tests then hold the kernels to them word for word."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def keys_of(row, col, size0, size1, csc):
    """The reference's sort key (storage.rs:112,119): col*size0+row for a CSC, row*size1+col for a CSR."""
    row, col = _i64(row), _i64(col)
    if row.size:
        major, minor, size_minor = (col, row, size0) if csc else (row, col, size1)
        assert int(major.max()) * int(size_minor) + int(minor.max()) < (1 << 63)   # in Python ints: no silent wrap below
    return col * np.int64(size0) + row if csc else row * np.int64(size1) + col


def to_csx(row, col, size0, size1, csc):
    """(ptrs [m + 1], indices [nnz], perm [nnz]): a stable sort by the key, so parallel edges keep their input order."""
    row, col = _i64(row), _i64(col)
    m, size_minor = (size1, size0) if csc else (size0, size1)
    assert int(m) * int(size_minor) < (1 << 63)
    keys = keys_of(row, col, size0, size1, csc)
    perm = np.argsort(keys, kind="stable").astype(np.int64)
    indices = (row if csc else col)[perm]
    bounds = np.arange(m + 1, dtype=np.int64) * np.int64(size_minor)
    ptrs = np.searchsorted(keys[perm], bounds, "left").astype(np.int64)
    return ptrs, indices, perm


def ind2ptr(ind, m):
    """out[j] = number of entries of the sorted `ind` below j, j = 0..m (entries >= m are counted by no j but m's own
    rule: they are simply not below it)."""
    return np.searchsorted(_i64(ind), np.arange(m + 1, dtype=np.int64), "left").astype(np.int64)


def max_degree(ptrs):
    ptrs = _i64(ptrs)
    return int((ptrs[1:] - ptrs[:-1]).max()) if ptrs.size > 1 else 0


def check_range(v, lo, hi):
    """True when any value lies outside [lo, hi)."""
    v = _i64(v)
    return bool(((v < lo) | (v >= hi)).any())


def sanitize_range(v, lo, hi):
    """(out, flag): out[i] = v[i] inside [lo, hi), else lo; flag = whether any was replaced."""
    v = _i64(v)
    bad = (v < lo) | (v >= hi)
    return np.where(bad, np.int64(lo), v), bool(bad.any())


def compact_rows(slab, lens):
    """slab [n_rows, pitch], lens [n_rows] -> the concatenation of slab[r, :lens[r]]."""
    slab, lens = _i64(slab), _i64(lens)
    parts = [slab[r, :int(lens[r])] for r in range(slab.shape[0])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def gather_rows(src_bytes, n_src_rows, row_bytes, stride_bytes, index):
    """(dst_bytes, status) on flat uint8 arrays: dst row i = the row_bytes bytes at src_bytes[index[i] * stride_bytes],
    all zero for an index outside [0, n_src_rows), which also sets status to 1."""
    src_bytes, index = np.asarray(src_bytes, dtype=np.uint8), _i64(index)
    ok = (index >= 0) & (index < n_src_rows)
    dst = np.zeros((index.size, row_bytes), dtype=np.uint8)
    if ok.any():
        at = index[ok][:, None] * np.int64(stride_bytes) + np.arange(row_bytes, dtype=np.int64)[None, :]
        dst[ok] = src_bytes[at]
    return dst.reshape(-1), int(not ok.all())
