"""tg_lastn_reset / _insert / _sample / _replay at the C ABI, on buffers the test owns: guard words before and after the
state, every output slab and the workspace (which has exactly the queried bytes), sentinels past every count.  The state is
compared byte for byte and every slab word for word with the NumPy restatement (helpers_lastn); both insert forms are forced
and must leave equal bytes; the samples must also equal tg_ns_homo_batched_ws with TG_SAMPLER_RECENT on the CSC of the
entries so far (timestamps = e_id)."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_lastn as hl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7
GUARD = 32           # guard words (256 bytes: the buffer behind them keeps its alignment)
LDS = hl.LDS_ENTRIES


def guarded(words, fill=SENT, dtype=torch.int64):
    """-> (whole buffer, the `words` words between two guards)"""
    buf = torch.full((GUARD + max(words, 1) + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + max(words, 1)]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).to(DEV)


class Ring:
    """a device state between guards and its restatement, driven together"""

    def __init__(self, n, k):
        from tch_geometric import _cabi, _cabi_lastn
        self.cabi, self.ops, self.n, self.k = _cabi, _cabi_lastn, n, k
        self.ref = hl.State(n, k)
        self.buf, self.state = guarded(hl.state_bytes(n, k) // 8)
        self.sbuf, self.status = guarded(1, dtype=torch.int32)
        self.status.zero_()
        self.entries = []
        self.st = self.ops.TgLastN(self.state.data_ptr(), self.state.numel() * 8, n, k)
        self.stream = self.cabi.stream_ptr(torch.device(DEV))
        self.cabi.check(self.ops.lib.tg_lastn_reset(C.byref(self.st), self.stream))
        self.check_state(0)

    def check_state(self, status):
        assert np.array_equal(self.state.cpu().numpy(), self.ref.words)
        assert guards_intact(self.buf) and guards_intact(self.sbuf)
        assert int(self.status.cpu()[0]) == status
        self.status.zero_()

    def reset(self):
        self.cabi.check(self.ops.lib.tg_lastn_reset(C.byref(self.st), self.stream))
        self.ref.reset()
        self.entries = []
        self.check_state(0)

    def device_insert(self, src, dst, e_id, e_base, symmetric, form):
        need, taken = self.ops.lastn_insert_workspace_bytes(len(src), symmetric, form)
        assert (need, taken) == hl.insert_workspace_bytes(len(src), symmetric, form) and (form == 0 or taken == form)
        wbuf, ws = guarded(need // 8)
        d_src, d_dst, d_e = dev(src), dev(dst), dev(e_id) if e_id is not None else None      # alive across the call
        self.cabi.check(self.ops.lib.tg_lastn_insert(
            C.byref(self.st), self.cabi.ptr(d_src), self.cabi.ptr(d_dst), self.cabi.ptr(d_e),
            e_base, len(src), int(symmetric), self.cabi.ptr(self.status), self.cabi.ptr(ws) if need else None, need, form, self.stream))
        torch.cuda.synchronize()
        assert guards_intact(wbuf)

    def insert(self, src, dst, e_id=None, e_base=0, symmetric=True, forms=(1, 2)):
        """the insert under every form of `forms` from the same state: equal bytes, equal to the restatement"""
        src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
        before = self.state.clone()
        status = self.ref.insert(src, dst, e_id, e_base, symmetric)
        self.entries += hl.entries_of(src, dst, e_id, e_base, symmetric)
        for i, form in enumerate(forms):
            if i:
                self.state.copy_(before)
            self.device_insert(src, dst, e_id, e_base, symmetric, form)
            self.check_state(status)

    def out(self, G, n_seeds, fanout, pad=0):
        cap_nodes, cap_edges = hl.capacity(n_seeds, fanout)
        cap_nodes, cap_edges = cap_nodes + pad, cap_edges + pad
        o = self.cabi.TgNsOut()
        bufs = {}
        for name, words in (("samples", G * cap_nodes), ("rows", G * cap_edges), ("cols", G * cap_edges),
                            ("edge_index", G * cap_edges), ("layer_offsets", G * len(fanout) * 3), ("counts", G * 2)):
            bufs[name] = guarded(words)
            setattr(o, name, bufs[name][1].data_ptr())
        o.cap_nodes, o.cap_edges = cap_nodes, cap_edges
        return o, bufs

    def expected(self, seeds, fanout, pad=0):
        """the slabs as the restatement leaves them from all-sentinel buffers -> (dict of arrays, status)"""
        G, n_seeds = seeds.shape
        cap_nodes, cap_edges = hl.capacity(n_seeds, fanout)
        cap_nodes, cap_edges = cap_nodes + pad, cap_edges + pad
        e = dict(samples=np.full((G, cap_nodes), SENT), rows=np.full((G, cap_edges), SENT), cols=np.full((G, cap_edges), SENT),
                 edge_index=np.full((G, cap_edges), SENT), layer_offsets=np.full((G, len(fanout), 3), SENT),
                 counts=np.full((G, 2), SENT))
        status = 0
        for b in range(G):
            s, r, c, ei, lo, cnt, st = self.ref.sample(seeds[b], fanout)
            e["samples"][b, :s.size], e["rows"][b, :r.size], e["cols"][b, :c.size], e["edge_index"][b, :ei.size] = s, r, c, ei
            e["layer_offsets"][b] = np.asarray(lo, dtype=np.int64).reshape(len(fanout), 3)
            e["counts"][b] = cnt
            status |= st
        return e, status

    def compare(self, bufs, want):
        for name, (buf, body) in bufs.items():
            w = want[name].reshape(-1)
            assert np.array_equal(body.cpu().numpy()[:w.size], w), name
            assert guards_intact(buf), name

    def sample(self, seeds, fanout, pad=0):
        seeds = np.asarray(seeds, dtype=np.int64)
        G, n_seeds = seeds.shape
        o, bufs = self.out(G, n_seeds, fanout, pad)
        fan = (C.c_int64 * max(len(fanout), 1))(*fanout)
        sd = dev(seeds) if seeds.size else torch.empty(1, dtype=torch.int64, device=DEV)
        self.cabi.check(self.ops.lib.tg_lastn_sample(C.byref(self.st), self.cabi.ptr(sd), G, n_seeds, fan, len(fanout), C.byref(o),
                                                     self.cabi.ptr(self.status), self.stream))
        want, status = self.expected(seeds, fanout, pad)
        self.compare(bufs, want)
        self.check_state(status)                                     # a lookup leaves the state as it is
        return want

    def recent(self, seeds, fanout):
        """the same lookup by TG_SAMPLER_RECENT on the CSC of the entries so far -> the slabs, e_id through the timestamps"""
        cabi = self.cabi
        ptrs, idx, ts = (dev(a) for a in hl.entries_csc(self.entries, self.n))
        g = cabi.graph_view(ptrs, idx, timestamps=ts)
        G, n_seeds = seeds.shape
        out = cabi.NsBatchedOut(G, n_seeds, fanout, DEV)
        ws = cabi.ns_homo_batched_workspace(g, G, n_seeds, fanout, DEV, sampler=cabi.SAMPLER_RECENT)
        cabi.ns_homo_batched(g, dev(seeds), fanout, 1, 2, out, sampler=cabi.SAMPLER_RECENT, ws=ws)
        torch.cuda.synchronize()
        return out, ts


def events(rs, n, m):
    return rs.integers(0, n, m), rs.integers(0, n, m)


# ---- insert --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 10, 63, 64])
def test_entries_per_node_and_ring_position(k):
    """0, 1, k-1, k, k+1 and 2k+1 entries of a node in one insert, over successive inserts whose counts land on, one below and
    one above a multiple of k; the ring wraps more than once"""
    per_node = [0, 1, k - 1, k, k + 1, 2 * k + 1]
    n = len(per_node) + 3
    ring = Ring(n, k)
    rs = np.random.default_rng(k)
    base = 0
    for rnd in range(4):
        per = per_node[rnd:] + per_node[:rnd]                        # every node sees every count, from every ring position
        dst = np.repeat(np.arange(len(per)), per)
        rs.shuffle(dst)
        src = rs.integers(0, n, dst.size)
        ring.insert(src, dst, e_base=base, symmetric=False)
        base += dst.size
    assert ring.ref.count.max() > 2 * k
    # land exactly one below, on and one above a multiple of k
    for v, target in ((0, -1), (1, 0), (2, 1)):
        c = int(ring.ref.count[v])
        add = (target - c) % k + k
        ring.insert(np.full(add, n - 1), np.full(add, v), e_base=base, symmetric=False)
        base += add
        assert int(ring.ref.count[v]) % k == target % k
    ring.sample(np.arange(n).reshape(1, -1), [k])
    ring.sample(np.arange(n).reshape(1, -1), [1])
    ring.reset()


@pytest.mark.parametrize("entries", [0, 1, 63, 64, 65, LDS - 1, LDS, LDS + 1])
def test_entry_counts_under_both_forms(entries):
    ring = Ring(500, 10)
    rs = np.random.default_rng(entries)
    ring.insert(*events(rs, 500, 300), symmetric=True)                  # the counts the call reads are not all zero
    src, dst = events(rs, 500, entries)
    ring.insert(src, dst, e_base=300, symmetric=False, forms=(1, 2) if entries <= LDS else (2, 0))
    if entries > LDS:
        with pytest.raises(ring.cabi.TchGeoError, match="LDS form"):
            ring.device_insert(src, dst, None, 0, False, 1)
    if entries % 2 == 0:
        half = entries // 2
        ring.insert(src[:half], dst[:half], e_base=900, symmetric=True, forms=(1, 2, 0))
    ring.sample(rs.integers(0, 500, (3, 65)), [3, 2])


def test_hub_takes_a_full_lds_batch():
    """every entry of a full LDS-form batch on one node; then the same under symmetric self loops"""
    ring = Ring(5, 10)
    ring.insert(np.arange(LDS) % 5, np.full(LDS, 3), symmetric=False)
    assert int(ring.ref.count[3]) == LDS
    ring.insert(np.full(LDS // 2, 2), np.full(LDS // 2, 2), e_base=LDS, symmetric=True)
    assert int(ring.ref.count[2]) == LDS
    ring.sample(np.array([[3, 2, 0]]), [10, 2])


def test_event_kinds_and_bad_ids():
    n, k = 40, 3
    ring = Ring(n, k)
    rs = np.random.default_rng(7)
    src, dst = events(rs, n, 50)
    src[5], dst[5] = 9, 9                                            # a self loop
    src[6:9], dst[6:9] = src[4], dst[4]                              # a repeated event
    ring.insert(src, dst, symmetric=True)
    ring.insert(src, dst, e_id=rs.integers(-100, 100, 50), symmetric=True)        # explicit ids, not monotone
    ring.insert(src, dst, e_id=rs.integers(-100, 100, 50), symmetric=False)
    for bad in (-1, n):                                              # at the first and the last entry, directed and symmetric
        s, d = src.copy(), dst.copy()
        d[0], s[-1] = bad, bad
        ring.insert(s, d, e_base=1000, symmetric=True)
        d[-1] = bad
        ring.insert(s, d, e_base=2000, symmetric=False)
    ring.insert([n, 3], [4, -1], e_base=3000, symmetric=True)       # nodes 4 and 3 now hold the neighbours n and -1
    # stored neighbours outside the range are samples, and empty frontier slots in the next hop; bad seeds raise the bit
    want = ring.sample(np.array([[0, -1, n, 5, 5] + list(range(n))]), [3, 2])
    assert ((want["samples"][0] == -1) | (want["samples"][0] == n)).sum() > 2


def test_large_state_past_4_gib():
    from tch_geometric import _cabi, _cabi_lastn as ops
    n, k = 1 << 23, 33
    words = hl.state_bytes(n, k) // 8
    assert words * 8 > 1 << 32
    buf = torch.empty(GUARD + words + GUARD, dtype=torch.int64, device=DEV)
    buf[:GUARD], buf[-GUARD:] = SENT, SENT
    state = buf[GUARD:GUARD + words]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = ops.TgLastN(state.data_ptr(), words * 8, n, k)
    stream = _cabi.stream_ptr(torch.device(DEV))
    _cabi.check(ops.lib.tg_lastn_reset(C.byref(st), stream))
    pad = hl.r256(8 * n) // 8
    assert not bool(state[:pad].any()) and bool((state[pad:] == -1).all())
    small = hl.State(2, k)                                           # node n - 1 stands at 1
    src = np.arange(100, 100 + 2 * k + 5)
    for form in (1, 2):
        need, _ = ops.lastn_insert_workspace_bytes(src.size, True, form)
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
        dst = np.where(np.arange(src.size) % 2 == 0, 0, n - 1)
        d_src, d_dst = dev(src), dev(dst)
        _cabi.check(ops.lib.tg_lastn_insert(C.byref(st), _cabi.ptr(d_src), _cabi.ptr(d_dst), None, 5, src.size, 0,
                                            _cabi.ptr(status), _cabi.ptr(ws), need, form, stream))
        small.insert(src, dst % (n - 2), e_base=5, symmetric=False)
    slots = state[pad:].view(n, k, 2)
    assert np.array_equal(slots[0].cpu().numpy(), small.slot[0]) and np.array_equal(slots[n - 1].cpu().numpy(), small.slot[1])
    assert state[:n].nonzero().reshape(-1).tolist() == [0, n - 1]
    assert [int(state[0]), int(state[n - 1])] == small.count.tolist() and not bool(state[n:pad].any())
    assert bool((slots[1:n - 1] == -1).all()) and guards_intact(buf) and int(status.item()) == 0
    seeds = dev([[n - 1, 0, 1]])
    out = ops.LastN.__new__(ops.LastN)                               # the wrapper's sample on the test's state
    out.n_nodes, out.k, out.device, out.state, out.state_bytes, out.status = n, k, torch.device(DEV), state, words * 8, status
    got = out.sample(seeds, [k])
    torch.cuda.synchronize()
    want = [n - 1, 0, 1] + [nbr for v in (1, 0) for nbr, _ in small.newest(v, k)]
    assert got.counts.cpu().tolist() == [[len(want), len(want) - 3]] and got.samples[0, :len(want)].cpu().tolist() == want


# ---- sample --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def busy():
    """one state with history: bursts, wrapped rings, empty nodes"""
    n, k = 300, 10
    ring = Ring(n, k)
    rs = np.random.default_rng(11)
    base = 0
    for m in (700, 40, 1500):
        src, dst = events(rs, n - 20, m)                             # the last 20 nodes stay empty
        ring.insert(src, dst, e_base=base, symmetric=True, forms=(0,))
        base += m
    return ring, rs


@pytest.mark.parametrize("n_seeds", [0, 1, 63, 64, 65, 1025])
@pytest.mark.parametrize("n_batches", [1, 3])
def test_sample_sizes(busy, n_seeds, n_batches):
    ring, rs = busy
    ring.sample(rs.integers(0, ring.n, (n_batches, n_seeds)), [3, 2])


@pytest.mark.parametrize("fanout", [[10], [1], [3, 2], [2, 2, 2], []])
def test_fanouts_with_300_batches(busy, fanout):
    ring, rs = busy
    seeds = rs.integers(0, ring.n, (300, 5))
    seeds[:, 1] = seeds[:, 0]                                        # repeated seeds
    seeds[7, 2], seeds[299, 4] = -1, ring.n                          # out of range
    seeds[:, 3] = ring.n - 1 - np.arange(300) % 20                   # nodes without entries
    ring.sample(seeds, fanout)


def test_capacity_is_exact_and_slack_is_left_alone(busy):
    ring, rs = busy
    full = np.flatnonzero(ring.ref.count >= 3)[:64].reshape(1, -1)   # every vertex fills its fan-out: the slabs are full
    want = ring.sample(full, [3])
    assert want["counts"][0].tolist() == list(hl.capacity(full.size, [3]))
    ring.sample(rs.integers(0, ring.n, (3, 64)), [3, 2], pad=5)      # cap_nodes above the capacity: the stride is honoured


def test_equals_the_recent_sampler_at_three_points_of_a_stream():
    n, k = 200, 4
    ring = Ring(n, k)
    rs = np.random.default_rng(23)
    base = 0
    for m in (60, 500, 3000):
        src, dst = events(rs, n, m)
        ring.insert(src, dst, e_base=base, symmetric=True, forms=(0,))
        base += m
        for fanout in ([4], [3, 2]):
            seeds = rs.integers(0, n, (3, 65))
            want = ring.sample(seeds, fanout)
            out, ts = ring.recent(seeds, fanout)
            assert np.array_equal(out.counts.cpu().numpy(), want["counts"])
            assert np.array_equal(out.layer_offsets.cpu().numpy(), want["layer_offsets"])
            for b in range(3):
                ns, ne = want["counts"][b]
                assert np.array_equal(out.samples[b, :ns].cpu().numpy(), want["samples"][b, :ns])
                assert np.array_equal(out.rows[b, :ne].cpu().numpy(), want["rows"][b, :ne])
                assert np.array_equal(out.cols[b, :ne].cpu().numpy(), want["cols"][b, :ne])
                assert np.array_equal(ts[out.edge_index[b, :ne]].cpu().numpy(), want["edge_index"][b, :ne])


# ---- replay --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G, step", [(1, 37), (3, 50), (64, 9), (2, 2100)])
def test_replay_equals_the_pairs_of_calls(G, step):
    """one call against the step-by-step calls and the restatement, with a short last step; (2, 2100) takes the grid insert"""
    n, k, fanout, n_seeds = 150, 5, [3, 2], 12
    n_events = G * step - step // 3
    rs = np.random.default_rng(G)
    src, dst = events(rs, n, n_events)
    seeds = rs.integers(0, n, (G, n_seeds))
    one, two = Ring(n, k), Ring(n, k)
    for r in (one, two):
        r.insert(*events(np.random.default_rng(5), n, 80), e_base=-80, forms=(0,))
    # the pairs of calls (each compared with the restatement)
    slabs = []
    for g in range(G):
        slabs.append(two.sample(seeds[g:g + 1], fanout))
        two.insert(src[g * step:(g + 1) * step], dst[g * step:(g + 1) * step], e_base=1000 + g * step, forms=(0,))
    want = {name: np.concatenate([s[name] for s in slabs]) for name in slabs[0]}
    # one call
    need = one.ops.lastn_replay_workspace_bytes(step)
    assert need == hl.insert_workspace_bytes(step, True)[0] and (need > 0) == (2 * step > LDS)
    wbuf, ws = guarded(need // 8)
    o, bufs = one.out(G, n_seeds, fanout)
    fan = (C.c_int64 * 2)(*fanout)
    d_src, d_dst, d_seeds = dev(src), dev(dst), dev(seeds)
    one.cabi.check(one.ops.lib.tg_lastn_replay(
        C.byref(one.st), one.cabi.ptr(d_src), one.cabi.ptr(d_dst), 1000, n_events, step, one.cabi.ptr(d_seeds), n_seeds, fan, 2,
        C.byref(o), one.cabi.ptr(one.status), one.cabi.ptr(ws) if need else None, need, one.stream))
    one.compare(bufs, want)
    assert guards_intact(wbuf)
    one.ref = two.ref
    one.check_state(0)
    assert torch.equal(one.state, two.state)
