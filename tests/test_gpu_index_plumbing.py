"""The index plumbing around the samplers at the C ABI, word for word against tests/helpers_ingest.py (proven on the CPU in
tests/test_ingest_cpu.py): tg_graph_max_degree, tg_ind2ptr, tg_check_range, tg_sanitize_range, tg_compact_rows,
tg_gather_rows and the empty-batch edge of tg_ns_homo_compact.  The range checks are the only thing between a bad node id
and a kernel that indexes `ptrs` with it; the others size or fill what a loader hands out.  Every output sits between
guard words (bytes for the gather) that must survive the call, starts as a value the call cannot produce, and is compared
for exact equality.  Each case names, in its comment, the defect it would catch."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_ingest as hi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16
SENTINEL = -0x5A5A5A5A5A5A5A5B
SENTINEL32 = -0x5A5A5A5B
GRID_THREADS = 8192 * 256                 # the grid cap of the element-wise kernels: past it the grid-stride loop runs


@pytest.fixture(scope="module")
def cabi():
    from tch_geometric import _cabi
    return _cabi


def i64(v):
    return C.c_int64(int(v))


def dev_of(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sync():
    torch.cuda.current_stream(torch.device(DEV)).synchronize()


class Guarded:
    """n elements between GUARD sentinel elements on either side; the payload starts as `payload` (default: sentinels)."""

    def __init__(self, n, dtype=torch.int64, payload=None):
        self.n, self.fill = n, SENTINEL if dtype == torch.int64 else SENTINEL32
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]
        if payload is not None:
            self.view.copy_(payload if torch.is_tensor(payload) else torch.full((n,), payload, dtype=dtype))

    def ptr(self):   # by arithmetic: an empty view's data_ptr() is null
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def assert_guards(self):
        assert bool((self.buf[:GUARD] == self.fill).all()), "elements in front of the output were written"
        assert bool((self.buf[GUARD + self.n:] == self.fill).all()), "elements behind the output were written"

    def numpy(self):
        return self.view.cpu().numpy()


# ------------------------------------------------------------------ tg_graph_max_degree
def _degree_case(n_major, longest_at):
    rng = np.random.default_rng([21, n_major])
    deg = rng.integers(0, 5, n_major)
    if longest_at == "empty":
        deg[:] = 0
    elif longest_at is not None:
        deg[longest_at] = 1000
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


MAX_DEGREE_CASES = [(0, None), (1, 0), (1, "empty"), (2, 0), (2, 1),
                    (255, 0), (255, 254),                                     # one ragged workgroup
                    (256, 0), (256, 255),                                     # a full workgroup: lane 255 is the last wavefront's
                    (257, 0), (257, 255), (257, 256),                         # the first column of a second workgroup
                    (100000, 0), (100000, 255), (100000, 256), (100000, 257), (100000, 99999), (100000, "empty"),
                    (GRID_THREADS + 1, GRID_THREADS)]                         # the longest column is the grid-stride tail's only one


@pytest.mark.parametrize("view", ["ptrs", "ptrs32"])
@pytest.mark.parametrize("n_major,longest_at", MAX_DEGREE_CASES)
def test_graph_max_degree(cabi, n_major, longest_at, view):
    """a reduction that drops a lane, a wavefront (part[] read before it is written) or the last column; j + 1 read as j;
    the u32 view read with 64-bit strides"""
    ptrs = _degree_case(n_major, longest_at)
    want = hi.max_degree(ptrs)
    assert want == (1000 if isinstance(longest_at, int) else 0)
    g = cabi.TgGraph()
    keep = dev_of(ptrs) if view == "ptrs" else dev_of(ptrs.astype(np.uint32).view(np.int32))
    g.ptrs, g.ptrs32 = (keep.data_ptr(), None) if view == "ptrs" else (None, keep.data_ptr())
    g.n_major = n_major
    out = Guarded(1, payload=1 << 50)            # larger than any degree: the word is overwritten, not max-ed with
    cabi.check(cabi.lib.tg_graph_max_degree(C.byref(g), out.ptr(), cabi.stream_ptr(torch.device(DEV))))
    sync()
    assert int(out.numpy()[0]) == want
    out.assert_guards()                          # the word behind the result (and the one in front) is intact


# ------------------------------------------------------------------ tg_ind2ptr
def _ind2ptr(cabi, ind, m):
    out = Guarded(m + 1)
    d = dev_of(ind) if ind.size else None
    cabi.check(cabi.lib.tg_ind2ptr(cabi.ptr(d), i64(ind.size), i64(m), out.ptr(), cabi.stream_ptr(torch.device(DEV))))
    sync()
    out.assert_guards()
    return out.numpy()


@pytest.mark.parametrize("numel", [0, 1, 1000000])
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257,                # out has m + 1 words: the last one dropped (j < m for j <= m)
                               GRID_THREADS + 1])                   # more outputs than threads: the grid-stride tail
def test_ind2ptr(cabi, m, numel):
    rng = np.random.default_rng([22, m, numel])
    lo, hi_ = (m // 4, max(m - m // 4, m // 4 + 1)) if m > 8 else (0, max(m, 1))   # empty ends where m leaves room
    ind = np.sort(rng.integers(lo, hi_, numel)).astype(np.int64)    # drawn with replacement: values repeat (m = 0: all >= m)
    got = _ind2ptr(cabi, ind, m)
    assert np.array_equal(got, hi.ind2ptr(ind, m))
    if m > 8 and numel:
        assert got[lo] == 0 and got[hi_] == numel == got[-1]        # the empty ends are there


@pytest.mark.parametrize("m", [1, 256, 5000])
def test_ind2ptr_entries_past_m(cabi, m):
    """entries >= m (the reference writes out of bounds on them): out[j] still counts the entries below j, so out[m] is
    short of numel; a kernel that scatters instead of searching would write past out[m] -- the guards stand there"""
    rng = np.random.default_rng([23, m])
    ind = np.sort(rng.integers(0, m + 50, 20000)).astype(np.int64)
    assert int(ind.max()) >= m
    got = _ind2ptr(cabi, ind, m)
    assert np.array_equal(got, hi.ind2ptr(ind, m)) and got[-1] == int((ind < m).sum()) < ind.size


# ------------------------------------------------------------------ tg_check_range / tg_sanitize_range
RANGE_N = [1, 63, 64, 65, 256, 257, GRID_THREADS + 5]


def _check_range(cabi, values_dev, n, lo, hi_, flag0=0, null_values=False):
    flag = Guarded(1, dtype=torch.int32, payload=flag0)
    rc = cabi.lib.tg_check_range(None if null_values else cabi.ptr(values_dev), i64(n), i64(lo), i64(hi_), flag.ptr(),
                                 cabi.stream_ptr(torch.device(DEV)))
    cabi.check(rc)
    sync()
    flag.assert_guards()                         # the int32 after the flag is intact: the OR is 4 bytes wide
    return int(flag.numpy()[0])


def _sanitize_range(cabi, values, lo, hi_, flag0=0, in_place=False):
    """values: NumPy.  -> (out, flag word); the input is checked to be unchanged unless in place"""
    n = values.size
    if in_place:
        out = Guarded(n, payload=dev_of(values))
        src_ptr = out.ptr()
    else:
        out, src = Guarded(n), Guarded(n, payload=dev_of(values))
        src_ptr = src.ptr()
    flag = Guarded(1, payload=flag0)
    cabi.check(cabi.lib.tg_sanitize_range(src_ptr, i64(n), i64(lo), i64(hi_), out.ptr(), flag.ptr(),
                                          cabi.stream_ptr(torch.device(DEV))))
    sync()
    for g in (out, flag) + (() if in_place else (src,)):
        g.assert_guards()
    if not in_place:
        assert np.array_equal(src.numpy(), values)
    return out.numpy(), int(flag.numpy()[0])      # the whole 8-byte word: a 4-byte OR into a poisoned word would show


def _bad_positions(n):
    at = {0, min(63, n - 1), n - 1}
    if n > GRID_THREADS:
        at |= {GRID_THREADS, GRID_THREADS + 3}    # elements only the second round of the grid-stride loop reads
    return sorted(at)


@pytest.mark.parametrize("n", RANGE_N)
def test_check_range_positions(cabi, n):
    """one bad value at index 0, 63, n - 1 and in the grid-stride tail: a loop bound off by one, a wavefront whose ballot is
    lost because lane 0 is past n, a tail never read"""
    lo, hi_ = 0, 10
    values = np.random.default_rng([24, n]).integers(lo, hi_, n)
    d = dev_of(values)
    assert not hi.check_range(values, lo, hi_)
    assert _check_range(cabi, d, n, lo, hi_) == 0                       # a clean input leaves a zero flag at 0
    assert _check_range(cabi, d, n, lo, hi_, flag0=1) == 1              # the flag is OR-ed, not stored
    for at in _bad_positions(n):
        for bad in (hi_, lo - 1):
            old = int(values[at])
            values[at] = bad
            d[at] = bad
            assert hi.check_range(values, lo, hi_)
            assert _check_range(cabi, d, n, lo, hi_) == 1, (at, bad)
            assert _check_range(cabi, d, n, lo, hi_, flag0=2) == 3, (at, bad)   # other bits survive
            values[at] = old
            d[at] = old
    assert _check_range(cabi, d, n, lo, hi_) == 0


@pytest.mark.parametrize("n", RANGE_N)
def test_sanitize_range_positions(cabi, n):
    """the same positions; the bad entry becomes lo (5, not 0), every other word is copied, the flag word is exactly 1"""
    lo, hi_ = 5, 9
    values = np.random.default_rng([25, n]).integers(lo, hi_, n)
    out, flag = _sanitize_range(cabi, values, lo, hi_)
    assert np.array_equal(out, values) and flag == 0
    assert _sanitize_range(cabi, values, lo, hi_, flag0=1)[1] == 1
    for at in _bad_positions(n):
        v = values.copy()
        v[at] = hi_ if at % 2 else lo - 1
        want, wflag = hi.sanitize_range(v, lo, hi_)
        assert wflag and want[at] == lo
        for in_place in (False, True):                                  # out == values is how a host reuses its buffer
            out, flag = _sanitize_range(cabi, v, lo, hi_, in_place=in_place)
            assert np.array_equal(out, want) and flag == 1, (at, in_place)
        assert _sanitize_range(cabi, v, lo, hi_, flag0=2)[1] == 3


@pytest.mark.parametrize("lo,hi_", [(0, 10), (5, 6), (-3, 3)])
def test_range_boundaries(cabi, lo, hi_):
    """lo - 1 bad, lo good, hi - 1 good, hi bad, the int64 extremes bad: `>` for `>=`, `<=` for `<`, an unsigned compare
    (which accepts nothing below a negative lo), hi - lo computed in 32 bits"""
    base = np.full(65, lo, dtype=np.int64)
    for value, bad in ((lo - 1, True), (lo, False), (hi_ - 1, False), (hi_, True), (hi.I64_MIN, True), (hi.I64_MAX, True)):
        for at in (0, 64):
            v = base.copy()
            v[at] = value
            assert hi.check_range(v, lo, hi_) == bad
            assert _check_range(cabi, dev_of(v), v.size, lo, hi_) == int(bad), (value, at)
            want, wflag = hi.sanitize_range(v, lo, hi_)
            out, flag = _sanitize_range(cabi, v, lo, hi_)
            assert np.array_equal(out, want) and flag == int(wflag) == int(bad), (value, at)
            assert out[at] == (lo if bad else value)


def test_check_range_empty_range_flags_every_value(cabi):
    """lo >= hi: no value is inside (a type with no nodes); tg_sanitize_range refuses such a range instead"""
    for lo, hi_ in ((3, 3), (4, 3), (0, 0), (0, -1)):
        for v in ([3], [0], [-1], [2, 3, 4]):
            assert hi.check_range(v, lo, hi_)
            assert _check_range(cabi, dev_of(np.array(v, dtype=np.int64)), len(v), lo, hi_) == 1


def test_range_checks_with_no_values(cabi):
    """n = 0 returns TG_OK without a launch: null value pointers are fine and the flag keeps its word"""
    assert _check_range(cabi, None, 0, 0, 10, flag0=0, null_values=True) == 0
    assert _check_range(cabi, None, 0, 0, 10, flag0=2, null_values=True) == 2
    flag = Guarded(1, payload=2)
    cabi.check(cabi.lib.tg_sanitize_range(None, i64(0), i64(0), i64(10), None, flag.ptr(), cabi.stream_ptr(torch.device(DEV))))
    sync()
    assert int(flag.numpy()[0]) == 2
    flag.assert_guards()


# ------------------------------------------------------------------ tg_compact_rows
def _compact_rows(cabi, lens, pitch, lens_stride):
    """slab[r, i] = r * 2^32 + i, so a word read past lens[r], from the wrong row or with the wrong pitch names itself"""
    lens = np.asarray(lens, dtype=np.int64)
    n_rows, dev = lens.size, torch.device(DEV)
    slab = (torch.arange(n_rows, device=dev).view(-1, 1) << 32) + torch.arange(pitch, device=dev).view(1, -1)
    slab = slab.contiguous()
    assert slab.shape == (n_rows, pitch) and slab.dtype == torch.int64
    counts = torch.full((max(n_rows, 1), lens_stride), 1 << 40, dtype=torch.int64, device=dev)   # the other column: poison
    if n_rows:
        counts[:, 0] = dev_of(lens)
    col = counts[:n_rows, 0]                       # what a loader passes: a column of its [n_rows, 2] counts tensor
    assert n_rows == 0 or (col.stride(0) == lens_stride and col.data_ptr() == counts.data_ptr())
    off = dev_of(np.cumsum(lens) - lens)
    dst = Guarded(int(lens.sum()))
    null = n_rows == 0
    cabi.check(cabi.lib.tg_compact_rows(None if null else cabi.ptr(slab), i64(pitch), None if null else cabi.ptr(counts),
                                        i64(lens_stride), None if null else cabi.ptr(off), i64(n_rows),
                                        None if null else dst.ptr(), cabi.stream_ptr(dev)))
    sync()
    dst.assert_guards()
    want = hi.compact_rows(slab.cpu().numpy().reshape(n_rows, pitch), lens)
    got = dst.numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("lens_stride", [1, 2])                     # 2: lens read as consecutive words picks up the other column
@pytest.mark.parametrize("pitch", [10000, 10007])                    # the longest row exactly, and larger: pitch taken for a length
def test_compact_rows_lengths(cabi, pitch, lens_stride):
    """row lengths around the workgroup (256) and around one round of a row's 8 x 256 threads (2 048), past which a thread
    takes a second element; zero-length rows between them write nothing"""
    _compact_rows(cabi, [0, 1, 255, 256, 257, 0, 2047, 2048, 2049, 10000, 0, 3], pitch, lens_stride)


@pytest.mark.parametrize("lens_stride", [1, 2])
@pytest.mark.parametrize("n_rows", [0, 1, 3, 40000])                  # 0: no launch, null pointers; 40 000: one grid row each
def test_compact_rows_row_counts(cabi, n_rows, lens_stride):
    rng = np.random.default_rng([26, n_rows])
    lens = rng.integers(0, 25, n_rows)
    lens[rng.integers(0, max(n_rows, 1), n_rows // 4)] = 0
    longest = int(lens.max()) if n_rows else 1
    for pitch in (max(longest, 1), longest + 3):
        _compact_rows(cabi, lens, pitch, lens_stride)


def test_compact_rows_all_rows_empty(cabi):
    """nothing to write: the guards are the whole check"""
    _compact_rows(cabi, [0, 0, 0], 8, 1)


# ------------------------------------------------------------------ tg_gather_rows on flat bytes
BYTE_GUARD = 64


def _gather(cabi, src_host, n_src_rows, row_bytes, stride, index, src_off=0, dst_off=0, status0=0, null_src=False):
    """src_host: NumPy uint8, the bytes from the source pointer on.  The device source starts src_off bytes past a 256-byte
    boundary, the destination dst_off bytes past one.  status0 None: a null status pointer.  -> status word or None"""
    dev = torch.device(DEV)
    index = np.asarray(index, dtype=np.int64)
    n = index.size
    sbuf = torch.zeros(src_off + src_host.size + 16, dtype=torch.uint8, device=dev)
    sbuf[src_off:src_off + src_host.size] = dev_of(src_host)
    front = 256 + dst_off
    dbuf = torch.full((front + n * row_bytes + BYTE_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert sbuf.data_ptr() % 256 == 0 and dbuf.data_ptr() % 256 == 0
    status = Guarded(1, dtype=torch.int32, payload=0 if status0 is None else status0)
    rc = cabi.lib.tg_gather_rows(None if null_src else C.c_void_p(sbuf.data_ptr() + src_off), i64(n_src_rows), i64(row_bytes),
                                 i64(stride), cabi.ptr(dev_of(index)), i64(n), C.c_void_p(dbuf.data_ptr() + front),
                                 None if status0 is None else status.ptr(), cabi.stream_ptr(dev))
    cabi.check(rc)
    sync()
    want, wstatus = hi.gather_rows(src_host, n_src_rows, row_bytes, stride, index)
    got = dbuf.cpu().numpy()
    assert np.all(got[:front] == 0xA5), "bytes in front of the destination were written"
    assert np.all(got[front + n * row_bytes:] == 0xA5), "bytes behind the destination were written"
    assert np.array_equal(got[front:front + n * row_bytes], want)
    status.assert_guards()
    if status0 is None:
        return None
    assert int(status.numpy()[0]) == (status0 | wstatus)
    return int(status.numpy()[0])


def _source(key, n_rows, stride, row_bytes):
    """random bytes 1..255 (a zero row is then a row the kernel zeroed); rows `stride` apart, the last one `row_bytes` long"""
    return np.random.default_rng([27] + list(key)).integers(1, 256, (n_rows - 1) * stride + row_bytes).astype(np.uint8)


@pytest.mark.parametrize("row_bytes", list(range(1, 131)) + [255, 256, 257, 1023, 1024, 1025, 1040, 4096])
def test_gather_row_widths(cabi, row_bytes):
    """every vector width (16 / 8 / 4 / 1 bytes by the row length), every lanes_log2 and, from 1 040 bytes on, the second
    pass of the column loop: a row's tail vector dropped, lanes past the row writing, vpr rounded the wrong way"""
    index = np.random.default_rng([28, row_bytes]).integers(0, 300, 1000)
    assert _gather(cabi, _source((row_bytes,), 300, row_bytes, row_bytes), 300, row_bytes, row_bytes, index) == 0


@pytest.mark.parametrize("stride", [64, 72, 68, 65])
def test_gather_alignment_dispatch(cabi, stride):
    """64-byte rows with the destination, the source and the stride each at 16 / 8 / 4 / 1-byte alignment: the dispatcher
    must fall to a width every one of them allows (an alignment left out of the OR is a misaligned vector access, whose
    result would differ).  The width it picks is not asserted, only the bytes."""
    index = np.random.default_rng([29, stride]).integers(0, 300, 1000)
    src = _source((64, stride), 300, stride, 64)
    for dst_off in (0, 4, 8, 1):
        for src_off in (0, 4, 8, 1):
            assert _gather(cabi, src, 300, 64, stride, index, src_off=src_off, dst_off=dst_off) == 0


@pytest.mark.parametrize("row_bytes,tile", [(16, 1024),      # one lane per row: 256 rows a pass, 4 passes unrolled
                                            (1024, 16)])     # a wavefront per row: 4 rows a pass
@pytest.mark.parametrize("tiles,extra", [(1, -1), (1, 0), (1, 1), (4, 3)])
def test_gather_n_around_the_tile(cabi, row_bytes, tile, tiles, extra):
    """n one short of, at and one past a workgroup's tile: the unrolled slots past n must neither load nor store"""
    n = tiles * tile + extra
    index = np.random.default_rng([30, row_bytes, n]).integers(0, 50, n)
    assert _gather(cabi, _source((row_bytes, 1), 50, row_bytes, row_bytes), 50, row_bytes, row_bytes, index) == 0


def test_gather_past_the_grid_cap(cabi):
    """33-byte rows take the byte path with 64 lanes a row and 16 rows a tile; 16 384 x 16 + 17 rows are one more than the
    grid cap of 16 384 workgroups covers in a round, so the grid-stride loop runs a second, ragged one (9 MB written)"""
    n = 16384 * 16 + 17
    index = np.random.default_rng([31]).integers(0, 1000, n)
    assert _gather(cabi, _source((33,), 1000, 33, 33), 1000, 33, 33, index) == 0


@pytest.mark.parametrize("row_bytes,rows_per_pass", [(16, 256), (1024, 4)])
def test_gather_bad_indices(cabi, row_bytes, rows_per_pass):
    """-1, n_src_rows and INT64_MIN in the first, second and last unrolled slot of a tile, valid neighbours in the same tile:
    the bad rows are zero, the valid rows right, the status bit set without touching the others"""
    tile, n_src = 4 * rows_per_pass, 40
    n = 4 * tile + 3
    rng = np.random.default_rng([32, row_bytes])
    src = _source((row_bytes, 2), n_src, row_bytes, row_bytes)
    good = rng.integers(0, n_src, n)
    assert _gather(cabi, src, n_src, row_bytes, row_bytes, good) == 0                 # all valid: status stays 0
    for t0 in (0, 2 * tile):                                                          # the first tile and a later one
        index = good.copy()
        for slot, bad in ((0, -1), (1, n_src), (3, hi.I64_MIN)):
            index[t0 + slot * rows_per_pass + 1] = bad
        assert _gather(cabi, src, n_src, row_bytes, row_bytes, index) == 1
        assert _gather(cabi, src, n_src, row_bytes, row_bytes, index, status0=2) == 3
        assert _gather(cabi, src, n_src, row_bytes, row_bytes, index, status0=None) is None   # a null status is accepted
    index = good.copy()
    index[-1] = hi.I64_MAX                                                            # the ragged tile's last row
    assert _gather(cabi, src, n_src, row_bytes, row_bytes, index) == 1


@pytest.mark.parametrize("row_bytes", [16, 24, 33])
def test_gather_from_an_empty_source(cabi, row_bytes):
    """n_src_rows = 0 with a null source: every index is bad, five zero rows, status 1, the source never read"""
    empty = np.zeros(0, dtype=np.uint8)
    assert _gather(cabi, empty, 0, row_bytes, row_bytes, [0, 1, -1, 5, 0], null_src=True) == 1


def test_gather_source_past_4_gib(cabi):
    """rows 0-7 and the last 8 of a 2^20 + 8 row x 4 096 byte source: a row offset computed in 32 bits wraps to the front"""
    n_rows, row_bytes, dev = (1 << 20) + 8, 4096, torch.device(DEV)
    if torch.cuda.mem_get_info()[0] < (16 << 30):
        pytest.skip("needs 16 GiB of free device memory")
    patterns = np.random.default_rng([33]).integers(1, 256, (16, row_bytes)).astype(np.uint8)
    src = torch.empty(n_rows * row_bytes, dtype=torch.uint8, device=dev)
    assert src.numel() > (1 << 32) and src.data_ptr() % 16 == 0
    rows = list(range(8)) + list(range(n_rows - 8, n_rows))
    for k, r in enumerate(rows):
        src[r * row_bytes:(r + 1) * row_bytes] = dev_of(patterns[k])
    order = np.random.default_rng([34]).permutation(16)
    index = np.array(rows, dtype=np.int64)[order]
    dst = torch.full((256 + 16 * row_bytes + BYTE_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    status = Guarded(1, dtype=torch.int32, payload=0)
    cabi.check(cabi.lib.tg_gather_rows(cabi.ptr(src), i64(n_rows), i64(row_bytes), i64(row_bytes), cabi.ptr(dev_of(index)),
                                       i64(16), C.c_void_p(dst.data_ptr() + 256), status.ptr(), cabi.stream_ptr(dev)))
    sync()
    # the restatement on the 16 pattern rows packed together, indexed by their rank in `rows`
    want, wstatus = hi.gather_rows(patterns.reshape(-1), 16, row_bytes, row_bytes, order)
    got = dst.cpu().numpy()
    assert np.array_equal(got[256:256 + 16 * row_bytes], want) and wstatus == 0 and int(status.numpy()[0]) == 0
    assert np.all(got[:256] == 0xA5) and np.all(got[256 + 16 * row_bytes:] == 0xA5)
    status.assert_guards()


# ------------------------------------------------------------------ tg_ns_homo_compact: an empty batch between two others
def test_ns_homo_compact_empty_batch_in_the_middle(cabi):
    """a batch with zero nodes and zero edges between two non-empty ones: its offsets equal its successor's, and a loop
    that runs at least once would overwrite the successor's first word (the other edges: test_gpu_slab_alignment.py)"""
    dev = torch.device(DEV)
    nb, cap_nodes, cap_edges = 3, 50, 40
    counts = np.array([[7, 5], [0, 0], [9, 11]], dtype=np.int64)
    rng = np.random.default_rng([35])
    slabs = [rng.integers(0, 1 << 40, (nb, cap)) for cap in (cap_nodes, cap_edges, cap_edges, cap_edges)]
    keep = [dev_of(s) for s in slabs] + [dev_of(counts)]
    o = cabi.TgNsOut()
    o.samples, o.rows, o.cols, o.edge_index = (t.data_ptr() for t in keep[:4])
    o.counts, o.cap_nodes, o.cap_edges = keep[4].data_ptr(), cap_nodes, cap_edges
    off = [dev_of(np.concatenate([[0], np.cumsum(counts[:, k])]).astype(np.int64)) for k in (0, 1)]
    flat = [Guarded(int(counts[:, 0].sum()))] + [Guarded(int(counts[:, 1].sum())) for _ in range(3)]
    cabi.check(cabi.lib.tg_ns_homo_compact(C.byref(o), i64(nb), cabi.ptr(off[0]), cabi.ptr(off[1]), flat[0].ptr(),
                                           flat[1].ptr(), flat[2].ptr(), flat[3].ptr(), cabi.stream_ptr(dev)))
    sync()
    for k, (g, slab) in enumerate(zip(flat, slabs)):
        g.assert_guards()
        assert np.array_equal(g.numpy(), hi.compact_rows(slab, counts[:, 0 if k == 0 else 1]))
