"""The streaming last-k neighbour state (include/tchgeo_lastn.h, _cabi_lastn.LastN, LastNeighborLoader, TemporalEventLoader),
host-only parts: the NumPy restatement against a brute-force version that keeps every node's full history in a Python list,
and against helpers_recent.recent_ns_homo on the CSC of the same entries (timestamps = e_id); the state and workspace
formulas; every refusal that comes before a launch; the Python-side ValueErrors; the header under C99; the exports.  No GPU:
every device pointer handed over is null or an address that is never read."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_lastn as hl
import helpers_recent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_lastn.h")
NAMES = ["tg_lastn_state_bytes", "tg_lastn_reset", "tg_lastn_insert_workspace_bytes", "tg_lastn_insert", "tg_lastn_sample",
         "tg_lastn_replay_workspace_bytes", "tg_lastn_replay"]


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi_lastn
    return _cabi_lastn


# ---- the restatement against brute force ---------------------------------------------------------------------------------------
class BruteForce:
    """every node's full history in a list; nothing is ever overwritten"""

    def __init__(self, n_nodes, k):
        self.n_nodes, self.k, self.hist = n_nodes, k, [[] for _ in range(n_nodes)]

    def insert(self, src, dst, e_id=None, e_base=0, symmetric=True):
        status = 0
        for j, (s, d) in enumerate(zip(src, dst)):
            e = e_base + j if e_id is None else int(e_id[j])
            for node, nbr in ((d, s), (s, d))[:2 if symmetric else 1]:
                if 0 <= node < self.n_nodes:
                    self.hist[node].append((int(nbr), e))
                else:
                    status |= 2
        return status

    def state_words(self):
        st = hl.State(self.n_nodes, self.k)
        for v, h in enumerate(self.hist):
            st.count[v] = len(h)
            for c in range(max(0, len(h) - self.k), len(h)):
                st.slot[v, c % self.k] = h[c]
        return st.words

    def sample(self, seeds, fanout):
        samples, rows, cols, eidx, lo = [int(s) for s in seeds], [], [], [], []
        frontier = list(range(len(seeds)))
        for f in fanout:
            lo.append((len(samples), len(eidx), len(samples)))
            nxt = []
            for i in frontier:
                v = samples[i]
                if not 0 <= v < self.n_nodes:
                    continue
                for nbr, e in self.hist[v][::-1][:min(f, self.k)]:
                    rows.append(len(samples))
                    cols.append(i)
                    eidx.append(e)
                    nxt.append(len(samples))
                    samples.append(nbr)
            frontier = nxt
        return samples, rows, cols, eidx, lo, (len(samples), len(eidx))


def stream(seed, n, k):
    """insert calls of a random stream: directed and symmetric, self loops, repeated events, bursts on one node, ids out of
    range, explicit non-monotone e_id"""
    rs = np.random.default_rng(seed)
    calls, base = [], 0
    for c in range(8):
        m = int(rs.integers(0, 3 * k + 4))
        src, dst = rs.integers(0, n, m), rs.integers(0, n, m)
        if c % 3 == 1 and m:
            dst[:] = dst[0]                                          # a burst: more than k entries of one node in one call
        if c % 4 == 2 and m:
            src[0], dst[-1] = -1, n                                  # out of range at the first and last entry
        if m > 2:
            src[1] = dst[1]                                          # a self loop
            src[2], dst[2] = src[1], dst[1]                          # a repeated event
        e_id = rs.integers(-50, 50, m) if c % 5 == 3 else None
        calls.append(dict(src=src, dst=dst, e_id=e_id, e_base=base, symmetric=bool(c % 2 == 0)))
        base += m
    return rs, calls


@pytest.mark.parametrize("seed", range(10))
@pytest.mark.parametrize("k", [1, 2, 3, 10])
def test_rule_equals_brute_force(seed, k):
    n = 7 + seed
    rs, calls = stream(seed, n, k)
    st, bf = hl.State(n, k), BruteForce(n, k)
    assert st.words.size * 8 == hl.state_bytes(n, k)
    for call in calls:
        assert st.insert(**call) == bf.insert(**call)
        assert np.array_equal(st.words, bf.state_words())
        for fanout in ([k], [1], [min(3, k), min(2, k)], [min(2, k)] * 3):
            seeds = np.concatenate([rs.integers(0, n, 5), [-1, n, 0, 0]])
            got, want = st.sample(seeds, fanout), bf.sample(seeds, fanout)
            for g, w in zip(got[:4], want[:4]):
                assert np.array_equal(g, np.asarray(w, dtype=np.int64).reshape(-1))
            assert got[4] == want[4] and got[5] == want[5] and got[6] == 2
            assert got[5][0] <= hl.capacity(len(seeds), fanout)[0]
    st.reset()
    assert np.array_equal(st.words, hl.State(n, k).words)


@pytest.mark.parametrize("seed", range(6))
def test_rule_equals_the_recent_sampler_on_the_csc_of_the_entries(seed):
    """strictly increasing e_id: the ring's newest-first rule is TG_SAMPLER_RECENT's rank (larger timestamp first) on the CSC
    whose column v holds node v's entries (a fan-out is at most k, so the ring still holds every entry that rank selects;
    the two entries of a symmetric self loop tie, and carry the same words)"""
    rs = np.random.default_rng(100 + seed)
    n, k = 12, 4
    st, entries, base = hl.State(n, k), [], 0
    for c in range(6):
        m = int(rs.integers(1, 20))
        src, dst = rs.integers(0, n, m), rs.integers(0, n, m)
        st.insert(src, dst, e_base=base, symmetric=bool(c % 2))
        entries += hl.entries_of(src, dst, e_base=base, symmetric=bool(c % 2))
        base += m
        ptrs, idx, ts = hl.entries_csc(entries, n)
        for fanout in ([4], [1], [3, 2], [2, 2, 2]):
            seeds = rs.integers(0, n, 6)
            s, r, cc, e, lo, cnt, _ = st.sample(seeds, fanout)
            ws, wr, wc, we, wlo, wcnt, _ = helpers_recent.recent_ns_homo(ptrs, idx, ts, seeds, fanout)
            assert np.array_equal(s, ws) and np.array_equal(r, wr) and np.array_equal(cc, wc)
            assert np.array_equal(e, ts[we]) and lo == wlo and cnt == wcnt


def test_loader_view_numbers_the_inputs_first():
    st = hl.State(6, 3)
    st.insert([1, 2, 1, 5], [0, 0, 3, 0])
    s, r, c, e, _, _, _ = st.sample([0, 3], [3])
    n_id, ei, e_id = hl.loader_view(s, r, c, e)
    assert list(n_id) == [0, 3, 5, 2, 1] and list(e_id) == [3, 1, 0, 2]
    assert ei.tolist() == [[2, 3, 4, 4], [0, 0, 0, 1]]
    assert np.array_equal(n_id[ei[0]], s[r]) and np.array_equal(n_id[ei[1]], s[c])


# ---- formulas, header, exports -------------------------------------------------------------------------------------------------
def test_state_and_workspace_formulas(ops):
    for n, k in ((1, 1), (31, 64), (32, 10), (33, 3), (1 << 23, 33), (1 << 31, 64)):
        assert ops.lastn_state_bytes(n, k) == hl.state_bytes(n, k)
    assert hl.state_bytes(1, 1) == 256 + 16 and hl.state_bytes(1 << 23, 33) > 1 << 32
    for n_events in (0, 1, 31, 32, 33, 2047, 2048, 2049, 4096, 4097, 1 << 22):
        for symmetric in (False, True):
            for form in (0, 1, 2):
                if form == 1 and n_events * (1 + symmetric) > hl.LDS_ENTRIES:
                    with pytest.raises(RuntimeError, match="LDS form"):
                        ops.lastn_insert_workspace_bytes(n_events, symmetric, form)
                    continue
                assert ops.lastn_insert_workspace_bytes(n_events, symmetric, form) == hl.insert_workspace_bytes(
                    n_events, symmetric, form), (n_events, symmetric, form)
    assert ops.lastn_insert_workspace_bytes(2048, True)[1] == 1 and ops.lastn_insert_workspace_bytes(2049, True)[1] == 2
    assert ops.lastn_insert_workspace_bytes(4096, False) == (0, 1)
    for step in (1, 200, 2048, 2049, 1 << 22):
        assert ops.lastn_replay_workspace_bytes(step) == hl.insert_workspace_bytes(step, True)[0]
    assert ops.LASTN_LDS_ENTRIES == hl.LDS_ENTRIES and ops.LASTN_MAX_K == hl.MAX_K and ops.LASTN_MAX_EVENTS == hl.MAX_EVENTS


def test_header_is_c99():
    src = '#include "tchgeo_lastn.h"\nint main(void) { tg_lastn s; s.k = TG_LASTN_MAX_K; return s.k == 64 ? 0 : 1; }\n'
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)


def test_exports_equal_the_header(ops):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    assert [f for f, _ in ops.TgLastN._fields_] == ["state", "state_bytes", "n_nodes", "k"]
    assert "#define TG_LASTN_LDS_ENTRIES 4096" in text and "#define TG_LASTN_MAX_K 64" in text


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a non-null address that is never read: every call below is refused before anything is launched
BIG = 1 << 50


def state(ops, state=FAKE, n=100, k=10, state_bytes=None):
    return ops.TgLastN(state, hl.state_bytes(max(n, 1), min(max(k, 1), 64)) if state_bytes is None else state_bytes, n, k)


def out_struct(n_seeds, fanout, **kw):
    from tch_geometric import _cabi
    o = _cabi.TgNsOut()
    for f in ("samples", "rows", "cols", "edge_index", "layer_offsets", "counts"):
        setattr(o, f, kw.pop(f, FAKE))
    o.cap_nodes, o.cap_edges = hl.capacity(n_seeds, [min(max(f, 1), 64) for f in fanout])
    o.cap_nodes += kw.pop("d_nodes", 0)
    assert not kw
    return o


def call(ops, which, st="default", **kw):
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    st = state(ops, **{k: kw.pop(k) for k in ("state", "n", "k", "state_bytes") if k in kw}) if st == "default" else st
    sp = C.byref(st) if st is not None else None
    fanout = kw.pop("fanout", [3, 2])
    fan = (C.c_int64 * 8)(*fanout) if fanout is not None else None
    n_hops = kw.pop("n_hops", len(fanout) if fanout is not None else 2)
    if which == "reset":
        assert not kw
        return ops.lib.tg_lastn_reset(sp, None)
    if which == "insert":
        a = [p(kw.pop("src", FAKE)), p(kw.pop("dst", FAKE)), p(kw.pop("e_id", None)), i64(0), i64(kw.pop("n_events", 5000)),
             i32(kw.pop("symmetric", 1)), p(kw.pop("status", FAKE)), p(kw.pop("ws", FAKE)), i64(kw.pop("ws_bytes", BIG)),
             i32(kw.pop("form", 0))]
        assert not kw, kw
        return ops.lib.tg_lastn_insert(sp, *a, None)
    n_seeds = kw.pop("n_seeds", 4)
    o = kw.pop("out", "default")
    o = out_struct(n_seeds, fanout or [1], **{k: kw.pop(k) for k in ("samples", "rows", "cols", "edge_index", "layer_offsets",
                                                                      "counts", "d_nodes") if k in kw}) if o == "default" else o
    op = C.byref(o) if o is not None else None
    if which == "sample":
        a = [p(kw.pop("seeds", FAKE)), i64(kw.pop("n_batches", 2)), i64(n_seeds), fan, i32(n_hops), op, p(kw.pop("status", FAKE))]
        assert not kw, kw
        return ops.lib.tg_lastn_sample(sp, *a, None)
    a = [p(kw.pop("src", FAKE)), p(kw.pop("dst", FAKE)), i64(0), i64(kw.pop("n_events", 9000)), i64(kw.pop("step_events", 3000)),
         p(kw.pop("seeds", FAKE)), i64(n_seeds), fan, i32(n_hops), op, p(kw.pop("status", FAKE)), p(kw.pop("ws", FAKE)),
         i64(kw.pop("ws_bytes", BIG))]
    assert not kw, kw
    return ops.lib.tg_lastn_replay(sp, *a, None)


STATE = [
    (dict(st=None), "null state"),
    (dict(state=None), "null state"),
    (dict(k=0), "k = 0"),
    (dict(k=65), "k = 65"),
    (dict(n=0), "n_nodes = 0"),
    (dict(n=(1 << 31) + 1), "n_nodes"),
    (dict(state_bytes=hl.state_bytes(100, 10) - 1), "state_bytes"),
    (dict(state=FAKE + 8), "16-byte aligned"),
]
GRID_BYTES = hl.insert_workspace_bytes(5000, True)[0]
INSERT = STATE + [
    (dict(src=None), "null src"),
    (dict(dst=None), "null src"),
    (dict(status=None), "null status"),
    (dict(n_events=-1), "n_events"),
    (dict(n_events=(1 << 22) + 1), "n_events"),
    (dict(form=3), "unknown form"),
    (dict(form=-1), "unknown form"),
    (dict(form=1, n_events=2049), "LDS form"),
    (dict(form=1, n_events=4097, symmetric=0), "LDS form"),
    (dict(ws=None), "workspace"),
    (dict(ws_bytes=GRID_BYTES - 1), "workspace"),
    (dict(ws=FAKE + 4), "8-byte aligned"),
    (dict(form=2, n_events=1, ws_bytes=hl.insert_workspace_bytes(1, True, 2)[0] - 1), "workspace"),
]
SAMPLE = STATE + [
    (dict(seeds=None), "null seeds"),
    (dict(out=None), "null out"),
    (dict(status=None), "null out"),
    (dict(fanout=None), "null fanout"),
    (dict(fanout=[0]), "fanout\\[0\\] = 0"),
    (dict(fanout=[3, 11]), "fanout\\[1\\] = 11"),
    (dict(fanout=[1] * 8, n_hops=9), "n_hops"),
    (dict(n_hops=-1), "n_hops"),
    (dict(samples=None), "null output"),
    (dict(counts=None), "null output"),
    (dict(layer_offsets=None), "null output"),
    (dict(cols=None), "null edge output"),
    (dict(d_nodes=-1), "too small"),
    (dict(n_seeds=-1), "bad sizes"),
]
REPLAY = SAMPLE + [
    (dict(src=None), "null src"),
    (dict(dst=None), "null src"),
    (dict(n_events=-1), "n_events"),
    (dict(n_events=(1 << 22) + 1), "n_events"),
    (dict(step_events=0), "step_events"),
    (dict(ws=None), "workspace"),
    (dict(ws_bytes=hl.insert_workspace_bytes(3000, True)[0] - 1), "workspace"),
    (dict(ws=FAKE + 4), "8-byte aligned"),
]


@pytest.mark.parametrize("which, kw, word", [("reset", kw, w) for kw, w in STATE] + [("insert", kw, w) for kw, w in INSERT] +
                         [("sample", kw, w) for kw, w in SAMPLE + [(dict(n_batches=-1), "bad sizes"), (dict(n_batches=1 << 31), "bad sizes")]] +
                         [("replay", kw, w) for kw, w in REPLAY])
def test_refusals(ops, which, kw, word):
    assert call(ops, which, **kw) == 1                               # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_the_short_workspaces_above_are_one_byte_short_and_empty_calls_launch_nothing(ops):
    assert ops.lastn_insert_workspace_bytes(5000, True) == (GRID_BYTES, 2) and GRID_BYTES > 0
    assert ops.lastn_replay_workspace_bytes(3000) == hl.insert_workspace_bytes(3000, True)[0] > 0
    assert call(ops, "insert", n_events=0, ws=None, ws_bytes=0) == 0
    assert call(ops, "insert", n_events=0, src=None, dst=None, form=1, ws=None, ws_bytes=0) == 0
    assert call(ops, "sample", n_batches=0) == 0
    assert call(ops, "sample", n_batches=0, k=64, fanout=[64], n=1 << 31, state_bytes=hl.state_bytes(1 << 31, 64)) == 0
    assert call(ops, "replay", n_events=0, ws=None, ws_bytes=0) == 0
    b = C.c_int64(0)
    assert ops.lib.tg_lastn_state_bytes(0, 1, C.byref(b)) == 1 and ops.lib.tg_lastn_state_bytes(1, 65, C.byref(b)) == 1
    assert ops.lib.tg_lastn_state_bytes(1, 1, None) == 1 and ops.lib.tg_lastn_replay_workspace_bytes(0, C.byref(b)) == 1


# ---- the Python-side refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [(dict(size=0), "size"), (dict(size=65), "size"), (dict(num_nodes=0), "num_nodes"),
                                      (dict(num_nodes=(1 << 31) + 1), "num_nodes")])
def test_last_neighbor_loader_refusals_need_no_device(ops, kw, word):
    import tch_geometric
    assert tch_geometric.LastNeighborLoader is tch_geometric.last_neighbor.LastNeighborLoader
    args = dict(num_nodes=10, size=4)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        tch_geometric.LastNeighborLoader(device="cuda:0", **args)
    with pytest.raises(ValueError, match=word):
        ops.LastN(args["num_nodes"], args["size"], "cuda:0")


@pytest.mark.parametrize("kw, word", [
    (dict(size=0), "size"),
    (dict(size=65), "size"),
    (dict(num_neighbors=[5]), "fan-out"),
    (dict(num_neighbors=[2, 0]), "fan-out"),
    (dict(t=torch.tensor([0, 2, 1, 3])), "ascending"),
    (dict(t=torch.tensor([0, 1, 2])), "length"),
    (dict(batch_size=0), "batch_size"),
    (dict(prefetch=0), "prefetch"),
    (dict(neg_sampling_ratio=-1), "neg_sampling_ratio"),
    (dict(neg_range=(3, 3)), "neg_range"),
    (dict(num_nodes=0), "num_nodes"),
])
def test_temporal_event_loader_refusals_need_no_device(ops, kw, word):
    import tch_geometric
    assert tch_geometric.TemporalEventLoader is tch_geometric.last_neighbor.TemporalEventLoader
    args = dict(src=torch.tensor([0, 1, 2, 3]), dst=torch.tensor([1, 2, 3, 0]), t=torch.tensor([0, 1, 1, 5]), num_nodes=4,
                size=4, batch_size=2)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        tch_geometric.TemporalEventLoader(device="cuda:0", **args)
