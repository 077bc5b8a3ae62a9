"""Single-call negative sampling (tg_neg_sample, csrc/negative.hip) at the C ABI, on buffers the test owns, and a validator
of one call's outputs that does not use the oracle.

NegSpec describes one call in NumPy.  oracle(spec, seed, call_id) runs the CPU oracle on it; run_neg(cabi, spec, ...) runs
the library through ctypes: every output buffer has exactly the capacity include/tchgeo.h promises (max(n_inputs[t], 0) +
total items for a type, n_inputs[src] * num_neg for a relation) and sits between GUARD sentinel words, the workspace is
exactly the queried bytes between 32 guard words, and every word the call had no business writing must still hold the
sentinel afterwards.  check_semantics restates the rules of negative_sampling.rs on the outputs alone."""
import ctypes as C

import numpy as np

GUARD = 16
WS_GUARD = 32
SENTINEL = -0x5A5A5A5A5A5A5A5B          # negative: no node id, slot or count
SENTINEL32 = -0x5A5A5A5B


class TgNegOut(C.Structure):            # include/tchgeo.h tg_neg_out
    _fields_ = [("samples", C.POINTER(C.c_void_p)), ("rows", C.POINTER(C.c_void_p)), ("cols", C.POINTER(C.c_void_p)),
                ("n_samples", C.c_void_p), ("n_edges", C.c_void_p), ("panic", C.c_void_p)]


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


class NegSpec:
    """One negative-sampling call.  rels: (src type index, dst type index, CSR ptrs, CSR indices, node_count) in
    edge_types order; inputs: per type a NumPy array, or None for a type without an entry in `inputs` (n_inputs = -1)."""

    def __init__(self, n_types, rels, inputs, num_neg, try_count, inbound=False, homogeneous=False):
        self.n_types = n_types
        self.rels = [(int(s), int(d), _i64(p), _i64(i), int(nc)) for s, d, p, i, nc in rels]
        self.inputs = [None if x is None else _i64(x) for x in inputs]
        self.num_neg, self.try_count = int(num_neg), int(try_count)
        self.inbound, self.homogeneous = bool(inbound), bool(homogeneous)
        assert len(self.inputs) == n_types and (not homogeneous or (n_types == 1 and len(rels) == 1))
        self._dev = None

    @property
    def n_inputs(self):
        return [-1 if x is None else int(x.size) for x in self.inputs]

    def n_in(self, t):
        return 0 if self.inputs[t] is None else int(self.inputs[t].size)

    @property
    def items(self):
        return sum(self.n_in(t) for t in range(self.n_types)) * self.num_neg

    def item_range(self, t):
        b = sum(self.n_in(u) for u in range(t)) * self.num_neg
        return b, b + self.n_in(t) * self.num_neg

    def cap_nodes(self, t):
        return self.n_in(t) + self.items

    def cap_edges(self, r):
        return self.n_in(self.rels[r][0]) * self.num_neg

    def replace(self, **kw):
        args = dict(n_types=self.n_types, rels=self.rels, inputs=self.inputs, num_neg=self.num_neg,
                    try_count=self.try_count, inbound=self.inbound, homogeneous=self.homogeneous)
        args.update(kw)
        new = NegSpec(**args)
        if "rels" not in kw:
            new._dev = self._dev            # the graphs are the same tensors: upload them once
        return new

    def device_rels(self, torch, dev):
        if self._dev is None:
            up = {}

            def put(a):                     # relations that share one array share one upload
                if id(a) not in up:
                    up[id(a)] = torch.from_numpy(a).to(dev)
                return up[id(a)]
            self._dev = [(s, d, put(p), put(i), nc) for s, d, p, i, nc in self.rels]
        return self._dev


def oracle(spec, seed, call_id):
    """orc.neg_homo / orc.neg_hetero under orc.rng_philox(seed, call_id) -> the dict run_neg returns (panic 0); raises
    RuntimeError where the reference would panic."""
    import orc
    rng = orc.rng_philox(seed, call_id)
    if spec.homogeneous:
        _, _, p, i, nc = spec.rels[0]
        s, r, c, _ = orc.neg_homo(p, i, (p.size - 1, nc), spec.inputs[0], spec.num_neg, spec.try_count, rng)
        return dict(samples=[s], rows=[r], cols=[c], panic=0)
    names = ["t%d" % t for t in range(spec.n_types)]
    ets = [(names[s], "r%d" % k, names[d]) for k, (s, d, _, _, _) in enumerate(spec.rels)]
    keys = ["%s__%s__%s" % et for et in ets]
    P = {k: rel[2] for k, rel in zip(keys, spec.rels)}
    I = {k: rel[3] for k, rel in zip(keys, spec.rels)}
    S = {k: (rel[2].size - 1, rel[4]) for k, rel in zip(keys, spec.rels)}
    ins = {names[t]: x for t, x in enumerate(spec.inputs) if x is not None}
    s, r, c, _ = orc.neg_hetero(names, ets, P, I, S, ins, spec.num_neg, spec.try_count, spec.inbound, rng)
    return dict(samples=[_i64(s[n]) for n in names], rows=[_i64(r[k]) for k in keys], cols=[_i64(c[k]) for k in keys], panic=0)


def assert_equal(got, want):
    """Exact equality of two result dicts, buffer by buffer."""
    assert got["panic"] == want["panic"]
    for name in ("samples", "rows", "cols"):
        assert len(got[name]) == len(want[name])
        for k, (g, w) in enumerate(zip(got[name], want[name])):
            assert g.shape == w.shape, "%s[%d]: %d words, the oracle has %d" % (name, k, g.size, w.size)
            assert np.array_equal(g, w), "%s[%d] differs from the oracle first at word %d" % (
                name, k, int(np.flatnonzero(g != w)[0]))


# ------------------------------------------------------------------------------------------------ the C call
class Guarded:
    """n words between GUARD sentinel words on either side, all pre-filled with the sentinel."""

    def __init__(self, torch, dev, n, dtype=None, fill=SENTINEL):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype or torch.int64, device=dev)

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def numpy(self):
        return self.buf.cpu().numpy()

    def split(self, what):
        """-> the payload as NumPy, after asserting both guards."""
        a = self.numpy()
        assert (a[:GUARD] == self.fill).all(), "words in front of %s were written" % what
        assert (a[GUARD + self.n:] == self.fill).all(), "words behind %s (capacity %d) were written" % (what, self.n)
        return a[GUARD:GUARD + self.n]


def workspace_bytes(cabi, spec):
    nbytes = C.c_int64(-1)
    cabi.check(cabi.lib.tg_neg_workspace_bytes(C.byref(problem(cabi, spec, None, None)), C.byref(nbytes)))
    return nbytes.value


def problem(cabi, spec, torch, dev):
    """The tg_neg_problem of a spec; torch None: host-only, for the size query and the refusals that precede any launch
    (the graph pointers name a small host tensor that nothing may read, the input pointers are null)."""
    if torch is None:
        import torch as T
        z = T.zeros(2, dtype=T.int64)
        rels = [(s, d, z, z, nc) for s, d, _, _, nc in spec.rels]
        return cabi.neg_problem(spec.n_types, rels, spec.n_inputs, spec.num_neg, spec.try_count, None, spec.inbound,
                                spec.homogeneous)
    rels = spec.device_rels(torch, dev)
    ins = [None if x is None else torch.from_numpy(x).to(dev) for x in spec.inputs]
    return cabi.neg_problem(spec.n_types, rels, spec.n_inputs, spec.num_neg, spec.try_count, ins, spec.inbound,
                            spec.homogeneous)


def run_neg(cabi, problem_spec, seed, call_id, ws_shift=0, expect_rc=0):
    """tg_neg_workspace_bytes + tg_neg_sample on exact, guarded, sentinel-filled buffers -> dict(samples [T], rows [R],
    cols [R], panic), trimmed to n_samples / n_edges, as NumPy.  ws_shift: the workspace starts that many bytes past a
    256-byte boundary.  expect_rc != 0: the call must be refused with that code and must leave every word alone; -> the
    error text."""
    import torch
    spec, dev = problem_spec, torch.device("cuda:0")
    T, R = spec.n_types, len(spec.rels)
    pb = problem(cabi, spec, torch, dev)
    samples = [Guarded(torch, dev, spec.cap_nodes(t)) for t in range(T)]
    rows = [Guarded(torch, dev, spec.cap_edges(r)) for r in range(R)]
    cols = [Guarded(torch, dev, spec.cap_edges(r)) for r in range(R)]
    n_samples, n_edges = Guarded(torch, dev, T), Guarded(torch, dev, R)
    panic = Guarded(torch, dev, 1, torch.int32, SENTINEL32)
    keep = [(C.c_void_p * T)(*[g.ptr() for g in samples]), (C.c_void_p * R)(*[g.ptr() for g in rows]),
            (C.c_void_p * R)(*[g.ptr() for g in cols])]
    out = TgNegOut(keep[0], keep[1], keep[2], n_samples.ptr(), n_edges.ptr(), panic.ptr())
    nbytes = C.c_int64(-1)
    rc = cabi.lib.tg_neg_workspace_bytes(C.byref(pb), C.byref(nbytes))
    if rc != 0 and expect_rc:
        nbytes.value = 1 << 16              # a problem the size query refuses as well: any workspace will do
    else:
        cabi.check(rc)
    assert nbytes.value > 0 and ws_shift % 8 == 0 and 0 <= ws_shift < 256
    W = (nbytes.value + 7) // 8
    ws = torch.full((W + 2 * WS_GUARD + 64,), SENTINEL, dtype=torch.int64, device=dev)
    skip = (-(ws.data_ptr() + 8 * WS_GUARD)) % 256 + ws_shift        # bytes from the end of the front guard to the base
    first = WS_GUARD + skip // 8
    base = ws.data_ptr() + 8 * first
    assert base % 256 == ws_shift and first + W + WS_GUARD <= ws.numel()
    rc = cabi.lib.tg_neg_sample(C.byref(pb), C.byref(cabi.TgRng(seed, call_id)), C.byref(out), C.c_void_p(base),
                                cabi.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    w = ws.cpu().numpy()
    assert (w[:first] == SENTINEL).all(), "words in front of the workspace were written"
    assert (w[first + W:] == SENTINEL).all(), "words behind the workspace (%d bytes) were written" % nbytes.value
    if expect_rc:
        msg = cabi.lib.tg_last_error().decode()
        assert rc == expect_rc, (rc, msg)
        for what, g in [("an output", x) for x in samples + rows + cols + [n_samples, n_edges, panic]]:
            assert (g.numpy() == g.fill).all(), "a refused call wrote %s" % what
        return msg
    cabi.check(rc)
    ns, ne = n_samples.split("n_samples"), n_edges.split("n_edges")
    res = dict(samples=[], rows=[], cols=[], panic=int(panic.split("panic")[0]))
    assert res["panic"] in (0, 1)
    for t in range(T):
        a = samples[t].split("samples[%d]" % t)
        assert 0 <= ns[t] <= a.size, "n_samples[%d] = %d, capacity %d" % (t, ns[t], a.size)
        assert (a[ns[t]:] == SENTINEL).all(), "samples[%d] was written past n_samples = %d" % (t, ns[t])
        res["samples"].append(a[:ns[t]].copy())
    for r in range(R):
        for name, bufs in (("rows", rows), ("cols", cols)):
            a = bufs[r].split("%s[%d]" % (name, r))
            assert 0 <= ne[r] <= a.size, "n_edges[%d] = %d, capacity %d" % (r, ne[r], a.size)
            assert (a[ne[r]:] == SENTINEL).all(), "%s[%d] was written past n_edges = %d" % (name, r, ne[r])
            res[name].append(a[:ne[r]].copy())
    return res


def workspace_words_named(spec):
    """The words the layout comment in tg_neg_workspace_bytes names, from the problem alone: cand, ids, rank, erank and flag
    (m int64 each), rel_of (m int32), two hash maps of keys and values (power-of-two capacities above twice the largest
    input list and twice the items), the totals and the panic flag.  The scan library's own storage comes on top."""
    m = spec.items
    max_in = max([spec.n_in(t) for t in range(spec.n_types)] + [0])

    def pow2(n):
        c = 64
        while c < n:
            c <<= 1
        return c
    return 8 * (5 * m + 2 * pow2(2 * max_in + 2) + 2 * pow2(2 * m + 2) + 2) + 4 * m + 4


def check_workspace_law(cabi):
    """tg_neg_workspace_bytes is non-decreasing in every n_inputs[t] and in num_neg, covers the named words, and counts a
    type with n_inputs < 0 as one with none.  The query asks the scan library for its storage and so needs a device."""
    z = np.zeros(2, dtype=np.int64)
    rels = [(0, 0, z, z, 1000), (0, 1, z, z, 1000), (1, 2, z, z, 1000), (2, 0, z, z, 1000)]

    def spec_of(n_in, num_neg):
        return NegSpec(3, rels, [None if n < 0 else np.zeros(n, dtype=np.int64) for n in n_in], num_neg, 3)
    sizes = [0, 1, 31, 32, 33, 1000, 5461, 5462, 16384, 16385, 40000]      # 5 461 x 3 = 16 383: the one-workgroup limit
    for t in range(3):
        last = 0
        for n in sizes:
            n_in = [100, 200, 300]
            n_in[t] = n
            sp = spec_of(n_in, 3)
            got = workspace_bytes(cabi, sp)
            assert got >= last, "workspace shrinks as n_inputs[%d] grows to %d" % (t, n)
            assert got >= workspace_words_named(sp)
            last = got
    last = 0
    for num_neg in (0, 1, 2, 3, 7, 16, 55, 56, 100):                        # 300 x 55 = 16 500 crosses the limit
        sp = spec_of([100, 100, 100], num_neg)
        got = workspace_bytes(cabi, sp)
        assert got >= last and got >= workspace_words_named(sp), num_neg
        last = got
    for n_in in ([100, -1, 300], [-1, -5, 7], [-1, -1, -1]):
        zero = [max(n, 0) for n in n_in]
        assert workspace_bytes(cabi, spec_of(n_in, 3)) == workspace_bytes(cabi, spec_of(zero, 3))


# ------------------------------------------------------------------------------------------------ the validator
class SemanticsError(AssertionError):
    """.rules: the names of the broken rules."""

    def __init__(self, found):
        self.rules = [r for r, _ in found]
        AssertionError.__init__(self, "; ".join("%s: %s" % f for f in found))


def _edge_keys(ptrs, indices):
    rows = np.repeat(np.arange(ptrs.size - 1, dtype=np.int64), np.diff(ptrs))
    return np.unique(rows * np.int64(1 << 32) + indices)


def check_semantics(spec, out):
    """The rules of negative_sampling.rs on one call's outputs, without the oracle (ids below 2^31).  Raises
    SemanticsError naming every broken rule:
      inputs-first      samples[t][:n_in] == inputs[t]
      new-samples       the rest of samples[t] is distinct, in [0, node_count) and disjoint from the inputs of t
      cols-range        cols lie below n_samples[dst]
      rows              rows are non-decreasing and below n_inputs[src]
      row-count         at most num_neg pairs per row over the relations of one source type taken together
      last-slot         a col that names an input value names its LAST slot (HashMap::extend overwrites, :26 / :89)
      first-naming      every non-input sample is named by a col, and samples holds them in the order in which items, taken
                        type-major and then by row, first name them (:36-39 / :118-121)
      not-an-edge       no pair is an edge (has_edge(v, w), has_edge(w, v) when inbound) or has v == w (:35 / :117)"""
    T, R = spec.n_types, len(spec.rels)
    S, rows, cols = out["samples"], out["rows"], out["cols"]
    bad = []

    def rule(name, ok, text=""):
        if not ok:
            bad.append((name, text))
    assert len(S) == T and len(rows) == R and len(cols) == R
    n_in = [spec.n_in(t) for t in range(T)]
    for t in range(T):
        rule("inputs-first", S[t].size >= n_in[t] and (n_in[t] == 0 or np.array_equal(S[t][:n_in[t]], spec.inputs[t])),
             "type %d" % t)
        new = S[t][n_in[t]:]
        bound = max([nc for _, d, _, _, nc in spec.rels if d == t] + [0])
        rule("new-samples", np.unique(new).size == new.size, "type %d repeats a sample" % t)
        rule("new-samples", new.size == 0 or (new.min() >= 0 and new.max() < bound), "type %d: id outside [0, %d)" % (t, bound))
        rule("new-samples", n_in[t] == 0 or not np.isin(new, spec.inputs[t]).any(), "type %d: an input appears again" % t)
    per_row = [np.zeros(n_in[t], dtype=np.int64) for t in range(T)]
    ok_rel = []                                             # relations whose rows and cols can be used as indices below
    for r, (s, d, ptrs, idx, nc) in enumerate(spec.rels):
        rule("rows", rows[r].size == cols[r].size, "relation %d: rows and cols differ in length" % r)
        in_range = rows[r].size == 0 or (rows[r].min() >= 0 and rows[r].max() < n_in[s])
        rule("rows", in_range, "relation %d: a row outside [0, %d)" % (r, n_in[s]))
        rule("rows", bool((np.diff(rows[r]) >= 0).all()), "relation %d: rows decrease" % r)
        c_ok = cols[r].size == 0 or (cols[r].min() >= 0 and cols[r].max() < S[d].size)
        rule("cols-range", c_ok, "relation %d: a col outside [0, %d)" % (r, S[d].size))
        ok_rel.append(in_range and c_ok and rows[r].size == cols[r].size)
        if in_range:
            np.add.at(per_row[s], rows[r], 1)
    for t in range(T):
        rule("row-count", n_in[t] == 0 or per_row[t].max() <= spec.num_neg, "type %d: a row has %d pairs" % (
            t, per_row[t].max() if n_in[t] else 0))
    if not all(ok_rel):
        raise SemanticsError(bad)
    for r, (s, d, ptrs, idx, nc) in enumerate(spec.rels):
        if rows[r].size == 0:
            continue
        v, w = spec.inputs[s][rows[r]], S[d][cols[r]]
        rule("new-samples", w.max() < nc and w.min() >= 0, "relation %d pairs an id outside its node_count %d" % (r, nc))
        named_input = cols[r] < n_in[d]
        if named_input.any():
            last = {}
            for k, x in enumerate(spec.inputs[d].tolist()):
                last[x] = k
            want = np.array([last[x] for x in w[named_input].tolist()], dtype=np.int64)
            rule("last-slot", np.array_equal(cols[r][named_input], want), "relation %d" % r)
        a, b = (w, v) if spec.inbound else (v, w)
        in_rows = a < ptrs.size - 1                         # an inbound row past the CSR is the reference's panic, not an edge
        rule("not-an-edge", bool(in_rows.all()), "relation %d indexes a row past the CSR" % r)
        hit = np.isin(a * np.int64(1 << 32) + b, _edge_keys(ptrs, idx))
        rule("not-an-edge", not hit.any(), "relation %d returns an edge" % r)
        rule("not-an-edge", not (v == w).any(), "relation %d returns v == w" % r)
    for d in range(T):
        # items that name a non-input sample of d, in item order as far as the outputs tell it: (source type, row), then
        # the relation's own order; ties between relations inside one row are left open
        ent = [(np.full(cols[r].size, s, dtype=np.int64), rows[r], np.full(cols[r].size, r, dtype=np.int64),
                np.arange(cols[r].size, dtype=np.int64), cols[r])
               for r, (s, dd, _, _, _) in enumerate(spec.rels) if dd == d]
        n_new = S[d].size - n_in[d]
        if not ent:
            rule("first-naming", n_new == 0, "type %d has samples nobody names" % d)
            continue
        st, rw, rl, ps, cl = [np.concatenate(x) for x in zip(*ent)]
        keep = cl >= n_in[d]
        st, rw, rl, ps, cl = st[keep], rw[keep], rl[keep], ps[keep], cl[keep] - n_in[d]
        group = st * np.int64(1 << 32) + rw
        first = np.full(n_new, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(first, cl, group)
        rule("first-naming", bool((first < np.iinfo(np.int64).max).all()), "type %d: a sample no col names" % d)
        rule("first-naming", bool((np.diff(first) >= 0).all()), "type %d: samples are not in the order of first naming" % d)
        # inside one (row, relation) the relation's list is in item order: the samples it names first there ascend --
        # where no second relation joins the same two types, whose items could have named one of them in between
        pairs = [(s, dd) for s, dd, _, _, _ in spec.rels]
        alone = np.array([pairs.count(p) == 1 for p in pairs], dtype=bool)
        mine = (first[cl] == group) & alone[rl]
        order = np.lexsort((ps[mine], rl[mine], group[mine]))
        g, rr, cc = group[mine][order], rl[mine][order], cl[mine][order]
        seen_before = np.zeros(cc.size, dtype=bool)
        _, first_pos = np.unique(cc + rr * np.int64(1 << 40), return_index=True)     # first time relation rr names cc
        seen_before[:] = True
        seen_before[first_pos] = False
        g, rr, cc = g[~seen_before], rr[~seen_before], cc[~seen_before]
        same = (g[1:] == g[:-1]) & (rr[1:] == rr[:-1])
        rule("first-naming", bool((cc[1:][same] > cc[:-1][same]).all()),
             "type %d: inside one row a relation names new samples out of order" % d)
    if bad:
        raise SemanticsError(bad)
