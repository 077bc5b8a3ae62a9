"""Single-call negative sampling and the walks' host side, without a GPU.

check_semantics (tests/helpers_negative.py) is the oracle-free validator the GPU tests run on every result: here it must
accept what the CPU oracle returns on 50 small random problems and reject four corruptions by the name of the broken rule.
Then every refusal of tg_neg_sample that precedes its first device call, the laws of tg_neg_workspace_bytes and
tg_edge_set_bytes, and tg_tempo_random_walk's refusal of a row that does not fit the LDS walk buffer -- all with fake
pointers, so nothing can have been launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers_negative as hn
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_INVALID, TG_ERR_UNSUPPORTED = 1, 3
FAKE = 0x1000                                            # a non-null pointer nobody may follow


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


# ------------------------------------------------------------------------------------------------ the validator
def _random_csr(rng, n_rows, n_cols, deg):
    row = np.repeat(np.arange(n_rows, dtype=np.int64), deg)
    col = rng.integers(0, n_cols, row.size)
    ptrs, idx, _ = orc.to_csr(np.stack([row, col]), (n_rows, n_cols))
    return ptrs, idx


def small_spec(k):
    """Problem k of 50: even k homogeneous, odd k three types and five relations (two of them between the same types);
    few distinct inputs, so slots repeat, and a node range a few times the inputs, so both kinds of col occur."""
    rng = np.random.default_rng([0x4E65, k])
    if k % 2 == 0:
        n = int(rng.integers(20, 80))
        ptrs, idx = _random_csr(rng, n, n, int(rng.integers(1, 6)))
        inputs = rng.integers(0, max(n // 3, 2), int(rng.integers(5, 40)))
        return hn.NegSpec(1, [(0, 0, ptrs, idx, n)], [inputs], int(rng.integers(1, 6)), int(rng.integers(1, 5)),
                          homogeneous=True)
    sizes = [int(x) for x in rng.integers(30, 60, 3)]
    sizes[0] = max(sizes)                                # type 0 is the largest: inbound stays inside every CSR
    pattern = [(0, 0), (0, 1), (0, 1), (1, 2), (2, 2)]
    inbound = k % 4 == 3 and sizes[2] <= sizes[1]
    rels = [(s, d) + _random_csr(rng, sizes[s], sizes[d], 3) + (sizes[d],) for s, d in pattern]
    inputs = [rng.integers(0, 10, int(rng.integers(5, 30))), rng.integers(0, 10, int(rng.integers(1, 30))),
              None if k % 3 == 0 else rng.integers(0, 10, int(rng.integers(0, 10)))]
    return hn.NegSpec(3, rels, inputs, int(rng.integers(1, 5)), int(rng.integers(1, 5)), inbound=inbound)


@pytest.mark.parametrize("k", range(50))
def test_validator_accepts_the_oracle(k):
    spec = small_spec(k)
    hn.check_semantics(spec, hn.oracle(spec, 77, k))


def _copy(out):
    return dict(samples=[a.copy() for a in out["samples"]], rows=[a.copy() for a in out["rows"]],
                cols=[a.copy() for a in out["cols"]], panic=out["panic"])


def _rejected(spec, out, rule):
    with pytest.raises(hn.SemanticsError) as e:
        hn.check_semantics(spec, out)
    assert rule in e.value.rules, e.value.rules


def _homo_case():
    """A homogeneous problem on which every corruption below finds its place (asserted where it is applied)."""
    rng = np.random.default_rng(0xC0FFEE)
    n = 60
    ptrs, idx = _random_csr(rng, n, n, 6)
    spec = hn.NegSpec(1, [(0, 0, ptrs, idx, n)], [rng.integers(0, 15, 40)], 4, 6, homogeneous=True)
    out = hn.oracle(spec, 5, 0)
    hn.check_semantics(spec, out)
    return spec, out


def test_validator_rejects_a_col_moved_to_the_first_slot_of_a_duplicate_input():
    """atomicMin for atomicMax in neg_insert_inputs_kernel."""
    spec, out = _homo_case()
    inputs, bad = spec.inputs[0], _copy(out)
    moved = 0
    for e, c in enumerate(out["cols"][0]):
        if c < inputs.size and int(np.flatnonzero(inputs == inputs[c])[0]) != c:
            bad["cols"][0][e] = np.flatnonzero(inputs == inputs[c])[0]
            moved += 1
    assert moved > 0
    _rejected(spec, bad, "last-slot")


def test_validator_rejects_two_new_samples_swapped():
    """The same pairs under another numbering of the new samples: ranks taken in another order than the items'."""
    spec, out = _homo_case()
    n_in, bad = spec.inputs[0].size, _copy(out)
    a, b = n_in, out["samples"][0].size - 1
    assert b > a
    bad["samples"][0][[a, b]] = out["samples"][0][[b, a]]
    bad["cols"][0][out["cols"][0] == a] = b
    bad["cols"][0][out["cols"][0] == b] = a
    _rejected(spec, bad, "first-naming")


def test_validator_rejects_a_pair_that_is_an_edge():
    """A candidate accepted although has_edge said yes."""
    spec, out = _homo_case()
    _, _, ptrs, idx, _ = spec.rels[0]
    S, bad, done = out["samples"][0], _copy(out), False
    for e, i in enumerate(out["rows"][0]):
        v = spec.inputs[0][i]
        for w in idx[ptrs[v]:ptrs[v + 1]]:
            at = np.flatnonzero(S == w)
            if w != v and at.size:
                bad["cols"][0][e] = at[-1]           # the neighbour's slot as the rules number it: the last one
                done = True
                break
        if done:
            break
    assert done
    _rejected(spec, bad, "not-an-edge")


def test_validator_rejects_a_row_with_more_than_num_neg_pairs():
    """An edge rank that counts an item twice."""
    spec, out = _homo_case()
    rows, cols = out["rows"][0], out["cols"][0]
    full = np.flatnonzero(np.bincount(rows, minlength=spec.inputs[0].size) == spec.num_neg)
    assert full.size
    e = int(np.flatnonzero(rows == full[0])[-1])
    bad = _copy(out)
    bad["rows"][0], bad["cols"][0] = np.insert(rows, e, rows[e]), np.insert(cols, e, cols[e])
    _rejected(spec, bad, "row-count")


def test_validator_rejects_on_a_heterogeneous_result_too():
    """The last-slot and the ordering rule across two source types and two relations between one pair of types."""
    spec = small_spec(1)
    out = hn.oracle(spec, 77, 1)
    bad, moved = _copy(out), 0
    for r, (s, d, _, _, _) in enumerate(spec.rels):
        ins = spec.inputs[d]
        for e, c in enumerate(out["cols"][r]):
            if ins is not None and c < ins.size and int(np.flatnonzero(ins == ins[c])[0]) != c:
                bad["cols"][r][e] = np.flatnonzero(ins == ins[c])[0]
                moved += 1
    assert moved > 0
    _rejected(spec, bad, "last-slot")
    bad = _copy(out)
    n_in = spec.n_in(1)
    a, b = n_in, out["samples"][1].size - 1              # type 1: named from rows of type 0 through relations 1 and 2
    first_row = {}
    for r in (1, 2):
        for i, c in zip(out["rows"][r], out["cols"][r]):
            first_row[int(c)] = min(first_row.get(int(c), 1 << 60), int(i))
    assert first_row[a] < first_row[b]                   # named first in different rows: the order is decided
    bad["samples"][1][[a, b]] = out["samples"][1][[b, a]]
    for r in (1, 2):
        bad["cols"][r][out["cols"][r] == a] = b
        bad["cols"][r][out["cols"][r] == b] = a
    _rejected(spec, bad, "first-naming")


# ------------------------------------------------------------------------------------------------ refusals, sizes
def _fake_out(T, R):
    keep = [(C.c_void_p * T)(*[FAKE] * T), (C.c_void_p * R)(*[FAKE] * R), (C.c_void_p * R)(*[FAKE] * R)]
    out = hn.TgNegOut(keep[0], keep[1], keep[2], FAKE, FAKE, FAKE)
    out._keep = keep
    return out


def _spec(n_rels=1, n_in=8, num_neg=2, tries=2, node_count=100):
    z = np.zeros(2, dtype=np.int64)
    if n_rels == 1:
        return hn.NegSpec(1, [(0, 0, z, z, node_count)], [np.zeros(n_in, dtype=np.int64)], num_neg, tries, homogeneous=True)
    return hn.NegSpec(2, [(0, 1, z, z, node_count)] * n_rels, [np.zeros(n_in, dtype=np.int64), None], num_neg, tries)


def _sample_refused(cabi, p, word, null=None):
    out, rng = _fake_out(max(p.n_types, 1), max(p.n_rels, 1)), cabi.TgRng(1, 0)
    args = dict(pb=C.byref(p), rng=C.byref(rng), out=C.byref(out), ws=C.c_void_p(FAKE))
    if null:
        args[null] = None
    rc = cabi.lib.tg_neg_sample(args["pb"], args["rng"], args["out"], args["ws"], None)
    msg = cabi.lib.tg_last_error().decode()
    assert rc == TG_ERR_INVALID and "tg_neg_sample" in msg and word in msg, (rc, msg)


def test_neg_sample_refusals_before_the_first_device_call(cabi):
    """Each of these is checked before anything touches a device; every pointer handed over is fake, so a check that came
    too late would not return at all."""
    good = hn.problem(cabi, _spec(), None, None)
    for null in ("pb", "rng", "out", "ws"):
        _sample_refused(cabi, good, "null", null=null)
    p = hn.problem(cabi, _spec(), None, None)
    p.n_rels = 0
    _sample_refused(cabi, p, "relations")
    _sample_refused(cabi, hn.problem(cabi, _spec(n_rels=33), None, None), "33 relations")
    _sample_refused(cabi, hn.problem(cabi, _spec(num_neg=-1), None, None), "negative counts")
    _sample_refused(cabi, hn.problem(cabi, _spec(tries=-1), None, None), "negative counts")
    p = hn.problem(cabi, _spec(n_rels=3), None, None)
    p.graphs[2].ptrs = None
    _sample_refused(cabi, p, "relation 2 has no CSR")
    _sample_refused(cabi, hn.problem(cabi, _spec(node_count=0), None, None), "empty node range")
    p = hn.problem(cabi, _spec(n_rels=3), None, None)
    p.node_count[1] = 0
    _sample_refused(cabi, p, "relation 1 has an empty node range")


def test_neg_workspace_bytes(cabi):
    """The laws of hn.check_workspace_law.  The query asks the scan library for its temporary storage, which needs a device:
    where there is none it must say so (it guesses no size) and tests/test_gpu_negative_cabi.py runs the same laws."""
    nbytes = C.c_int64(-1)
    assert cabi.lib.tg_neg_workspace_bytes(None, C.byref(nbytes)) == TG_ERR_INVALID
    assert cabi.lib.tg_neg_workspace_bytes(C.byref(hn.problem(cabi, _spec(), None, None)), None) == TG_ERR_INVALID
    rc = cabi.lib.tg_neg_workspace_bytes(C.byref(hn.problem(cabi, _spec(), None, None)), C.byref(nbytes))
    if rc == 0:
        hn.check_workspace_law(cabi)
    else:
        assert b"device" in cabi.lib.tg_last_error()


def test_workspace_words_named_is_the_layout_comment():
    """The test's own count for 100 inputs x 3 (m = 300): 5 arrays of m int64, maps of 2 x (256 + 1 024) int64, two rank
    slack words, m int32 and the int32 panic flag."""
    z = np.zeros(2, dtype=np.int64)
    sp = hn.NegSpec(1, [(0, 0, z, z, 9)], [np.zeros(100, dtype=np.int64)], 3, 1, homogeneous=True)
    assert hn.workspace_words_named(sp) == 8 * (1500 + 2 * 256 + 2 * 1024 + 2) + 1200 + 4


@pytest.mark.parametrize("n_edges,slots", [(0, 64), (1, 64), (32, 64), (33, 128), (2048, 4096), (2049, 8192)])
def test_edge_set_bytes(cabi, n_edges, slots):
    """8 bytes a slot, max(64, smallest power of two >= 2 * n_edges) slots: a load factor of at most one half."""
    want = 64
    while want < 2 * n_edges:
        want *= 2
    assert want == slots
    nbytes = C.c_int64(-1)
    cabi.check(cabi.lib.tg_edge_set_bytes(C.byref(cabi.graph_sizing(10, n_edges)), C.byref(nbytes)))
    assert nbytes.value == 8 * slots


def test_edge_set_refuses_ids_that_do_not_fit_half_a_key(cabi):
    nbytes = C.c_int64(-1)
    assert cabi.lib.tg_edge_set_bytes(C.byref(cabi.graph_sizing((1 << 32) - 1, 10)), C.byref(nbytes)) == TG_ERR_INVALID
    assert "32-bit halves" in cabi.lib.tg_last_error().decode() and nbytes.value == -1
    cabi.check(cabi.lib.tg_edge_set_bytes(C.byref(cabi.graph_sizing((1 << 32) - 2, 10)), C.byref(nbytes)))
    assert nbytes.value == 8 * 64
    g = cabi.graph_sizing((1 << 32) - 1, 10)
    g.ptrs = g.indices = FAKE
    assert cabi.lib.tg_edge_set_build(C.byref(g), C.c_void_p(FAKE), C.c_int64(8 * 64), None) == TG_ERR_INVALID


def test_tempo_walk_refuses_a_row_longer_than_the_lds_buffer(cabi):
    """4 097 columns of (node, time) are 65 552 bytes for one wavefront: TG_ERR_UNSUPPORTED before any launch."""
    g = cabi.graph_sizing(10, 10)
    g.ptrs = g.indices = FAKE
    f = C.c_void_p(FAKE)
    rng = cabi.TgRng(1, 0)
    rc = cabi.lib.tg_tempo_random_walk(C.byref(g), f, f, f, f, C.c_int64(1), C.c_int64(4097), C.c_int64(0), C.c_int64(2),
                                       C.byref(rng), f, f, None)
    assert rc == TG_ERR_UNSUPPORTED and "walk_length 4097" in cabi.lib.tg_last_error().decode()
