"""tg_pinsage_hop / PinSAGELoader without a device: the restatement's selection against brute force, its termination
uniform against the oracle's Philox, the law the device test relies on by enumeration, a negative control of that test's
statistic, the header as C, every refusal of the C ABI (fake pointers: nothing is launched) and of the loader."""
import ctypes as C
import itertools
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import exact_laws
import orc
from helpers_labor import named_draw
from helpers_pinsage import TAG_PINSAGE, blocks, ends_before, select, select_brute, truncate, uniform01

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo.h")


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("R,T,k,n", [(1, 1, 3, 5), (4, 3, 2, 6), (10, 2, 3, 8), (7, 5, 64, 4), (40, 1, 5, 41), (16, 4, 1, 3)])
def test_select_equals_brute_force(R, T, k, n):
    rs = np.random.default_rng(R * 100 + T)
    m = 23
    walks = rs.integers(0, n, (m * R, T + 1)).astype(np.int64)
    cut = rs.integers(1, T + 2, m * R)                       # -1 padding from a random column on (never column 0)
    walks[np.arange(T + 1)[None, :] >= cut[:, None]] = -1
    walks[:R, 1:] = -1                                       # a slot that visits nothing
    got, want = select(walks, R, k), select_brute(walks, R, k)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert got[0][0] == 0 and got[0].max() <= k and (np.diff(got[2]) >= 0).all()
    skipped = select(walks, R, k, skip=[3])
    assert skipped[0][3] == 0 and 3 not in skipped[2]


def _f32_uniform(word):
    return struct.unpack("<f", struct.pack("<I", 0x3F800000 | (word >> 9)))[0] - 1.0


def test_termination_uniform_equals_the_oracles_philox():
    for seed, call, w, l, alpha in ((0, 0, 0, 1, 0.5), (7, 9, 12345, 2, 0.15), (2 ** 63 + 5, 2 ** 40 + 3, 2 ** 35 + 17, 63, 0.99),
                                    (1, 2, 163839, 1, 0.5), (0xABC, 77, 2 ** 44, 19, 0.01)):
        word = orc.philox_named_draw(seed, call, TAG_PINSAGE, w, l, 0)[0]
        u = _f32_uniform(word)
        assert float(uniform01(np.array([word]))[0]) == u and 0.0 <= u < 1.0
        got = bool(ends_before(np.uint64(seed), np.uint64(call), np.array([w], dtype=np.uint64), l, alpha)[0])
        assert got == (np.float32(u) < np.float32(alpha))
    assert float(uniform01(np.array([0xFFFFFFFF]))[0]) < 1.0 and float(uniform01(np.array([0]))[0]) == 0.0


def test_truncate_cuts_at_the_first_draw_below_alpha_and_never_the_first_step():
    R, T, m = 5, 4, 6
    walks = np.arange(m * R * (T + 1), dtype=np.int64).reshape(m * R, T + 1)
    ids = np.array([3, 0, 5, 1, 4, 2])
    calls = np.array([10, 10, 11, 12, 12, 12], dtype=np.uint64)
    out = truncate(walks, 42, calls, R, 0.5, ids)
    assert np.array_equal(truncate(walks, 42, calls, R, 0.0, ids), walks[(ids[:, None] * R + np.arange(R)).reshape(-1)])
    cuts = 0
    for i in range(m):
        for r in range(R):
            w = int(ids[i]) * R + r
            want, alive = walks[w].copy(), True
            for l in range(1, T):
                word = orc.philox_named_draw(42, int(calls[i]), TAG_PINSAGE, w, l, 0)[0]
                alive = alive and not (np.float32(_f32_uniform(word)) < np.float32(0.5))
                if not alive:
                    want[l + 1] = -1
            cuts += int((want < 0).any())
            assert np.array_equal(out[i * R + r], want) and out[i * R + r, 1] >= 0
    assert 0 < cuts < m * R


def test_blocks_composition():
    table = {0: ([5, 1], [3, 2]), 1: ([0], [4]), 5: ([1, 7], [2, 2]), 7: ([], [])}

    def hop(l, F):
        cnt, nbr, par, vis = [], [], [], []
        for i, v in enumerate(F):
            a, c = table.get(int(v), ([], []))
            cnt.append(len(a))
            nbr += a
            vis += c
            par += [i] * len(a)
        return tuple(np.asarray(x, dtype=np.int64) for x in (cnt, nbr, par, vis))

    bl, F = blocks([0, 1], hop, 2)
    assert F.tolist() == [0, 1, 5, 7] and len(bl) == 2
    inner, outer = bl[1], bl[0]
    assert inner["n_id"].tolist() == [0, 1, 5] and inner["n_dst"] == 2
    assert inner["edge_index"].tolist() == [[2, 1, 0], [0, 0, 1]] and inner["edge_weight"].tolist() == [3, 2, 4]
    assert outer["n_dst"] == 3 and outer["edge_index"].tolist() == [[2, 1, 0, 1, 3], [0, 0, 1, 2, 2]]


# ---------------------------------------------------------------- the law of the device test
def test_count_law_is_binomial_by_enumeration():
    """s -> a, a -> b, b a sink; T = 2: every walk visits a, and b iff it does not end before step 1.  Enumerating the 2^R
    outcomes of the termination draws at R = 4 gives P(count_b = c) = Binomial(R, 1 - alpha)."""
    R, alpha = 4, 0.3
    law = np.zeros(R + 1)
    for ends in itertools.product((False, True), repeat=R):
        walks = np.array([[0, 1, -1 if e else 2] for e in ends], dtype=np.int64)
        cnt, nbr, par, vis = select(walks, R, 2)
        assert nbr[0] == 1 and vis[0] == R
        c = int(vis[1]) if cnt[0] == 2 else 0
        assert c == R - sum(ends)
        law[c] += np.prod([alpha if e else 1 - alpha for e in ends])
    want = [math.comb(R, c) * (1 - alpha) ** c * alpha ** (R - c) for c in range(R + 1)]
    assert np.allclose(law, want, rtol=0, atol=1e-15)


def test_the_law_statistic_accepts_real_draws_and_rejects_six_bit_ones():
    """the device law test's statistic at its sample size (16 384 slots, R = 16, alpha = 0.5) on the restated draws: the
    real uniform passes; one cut to its top 6 bits and compared with <= ends a walk with probability 33 / 64 and must be
    rejected."""
    N, R = 16384, 16
    walker = np.arange(N * R, dtype=np.uint64)
    word = named_draw(np.uint64(5), np.uint64(0), TAG_PINSAGE, walker, 1, 0)[0]
    law = np.array([math.comb(R, c) * 0.5 ** R for c in range(R + 1)])
    real = ~ends_before(np.uint64(5), np.uint64(0), walker, 1, 0.5)
    assert np.array_equal(real, ~(uniform01(word) < np.float32(0.5)))
    exact_laws.chi2_gof(np.bincount(real.reshape(N, R).sum(1), minlength=R + 1), law, "restated counts")
    six = ~(uniform01((word >> np.uint64(26)) << np.uint64(26)) <= np.float32(0.5))
    with pytest.raises(AssertionError):
        exact_laws.chi2_gof(np.bincount(six.reshape(N, R).sum(1), minlength=R + 1), law, "6-bit draws")


# ---------------------------------------------------------------- header and binding
def test_header_compiles_as_c_with_the_new_names(tmp_path):
    src = tmp_path / "pinsage.c"
    src.write_text('#include "tchgeo.h"\n'
                   'typedef char a15[TG_TAG_PINSAGE == 15u ? 1 : -1];\n'
                   'typedef char a16[sizeof(tg_pinsage_config) == 16 ? 1 : -1];\n'
                   'int main(void) { tg_pinsage_config c; c.n_walks = 10; c.walk_length = 2; c.termination = 0.5f;\n'
                   '  c._reserved = 0; return c.n_walks * c.walk_length == 20 ? TG_OK : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])


def test_cabi_mirrors_the_header():
    from tch_geometric import _cabi
    assert _cabi.TAG_PINSAGE == TAG_PINSAGE == 15 and _cabi.PINSAGE_MAX_VISITS == 4096
    assert C.sizeof(_cabi.TgPinsageConfig) == 16
    for name in ("tg_pinsage_hop", "tg_pinsage_hop_workspace_bytes"):
        assert name in _cabi.EXPORTS and hasattr(_cabi.lib, name)
    assert _cabi.pinsage_hop_workspace_bytes(1000, 64) >= 1000 * 64 * 8 and _cabi.pinsage_hop_workspace_bytes(0, 1) == 0
    import tch_geometric
    assert tch_geometric.PinSAGELoader is tch_geometric.loader.PinSAGELoader


# ---------------------------------------------------------------- refusals of the C ABI: fake pointers, nothing is launched
FAKE = 1 << 20


def _args(cabi, m=1, fanout=3, R=10, T=2, alpha=0.5, n_major=8):
    g = cabi.TgGraph()
    g.ptrs = g.indices = FAKE
    g.n_major, g.n_edges = n_major, 100
    hin, hout = cabi.TgHopIn(), cabi.TgHopOut()
    hin.vertices, hin.m, hin.fanout = FAKE, m, fanout
    hout.cnt = hout.offsets = hout.neighbors = hout.parents = FAKE
    return dict(g=g, hin=hin, cfg=cabi.TgPinsageConfig(R, T, alpha, 0), rng=cabi.TgRng(1, 2), hout=hout, visits=FAKE,
                status=FAKE, ws=FAKE << 8, ws_bytes=1 << 30)


def _hop(cabi, a):
    ref = lambda x: C.byref(x) if x is not None else None
    vp = lambda x: C.c_void_p(x) if x else None
    rc = cabi.lib.tg_pinsage_hop(ref(a["g"]), ref(a["hin"]), ref(a["cfg"]), ref(a["rng"]), ref(a["hout"]), vp(a["visits"]),
                                 vp(a["status"]), vp(a["ws"]), C.c_int64(a["ws_bytes"]), None)
    return rc, cabi.lib.tg_last_error().decode()


def test_hop_refusals():
    from tch_geometric import _cabi as cabi
    for name in ("g", "hin", "cfg", "rng", "hout"):           # null structs
        a = _args(cabi)
        a[name] = None
        rc, err = _hop(cabi, a)
        assert rc == 1 and "null" in err, name
    for name in ("visits", "status"):                         # null buffers while m > 0
        a = _args(cabi)
        a[name] = None
        rc, err = _hop(cabi, a)
        assert rc == 1 and "null" in err, name
    for field in ("cnt", "offsets", "neighbors", "parents"):
        a = _args(cabi)
        setattr(a["hout"], field, None)
        rc, err = _hop(cabi, a)
        assert rc == 1 and "null" in err, field
    a = _args(cabi)
    a["hin"].vertices = None
    rc, err = _hop(cabi, a)
    assert rc == 1 and "null" in err
    a = _args(cabi)
    a["g"].ptrs = None
    rc, err = _hop(cabi, a)
    assert rc == 1 and "null graph" in err
    a = _args(cabi)
    a["hout"].edge_ptrs = FAKE
    rc, err = _hop(cabi, a)
    assert rc == 1 and "edge_ptrs" in err
    for R, T, word in ((0, 2, "n_walks"), (-1, 2, "n_walks"), (10, 0, "walk_length"), (10, -3, "walk_length")):
        rc, err = _hop(cabi, _args(cabi, R=R, T=T))
        assert rc == 1 and word in err
    for k in (0, 65, -1):
        rc, err = _hop(cabi, _args(cabi, fanout=k))
        assert rc == 1 and "1..64" in err
    for alpha in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        rc, err = _hop(cabi, _args(cabi, alpha=alpha))
        assert rc == 1 and "termination" in err, alpha
    rc, err = _hop(cabi, _args(cabi, m=-1))
    assert rc == 1 and "negative" in err
    a = _args(cabi)                                           # the workspace: missing, short, misaligned
    a["ws"] = None
    rc, err = _hop(cabi, a)
    assert rc == 1 and "workspace" in err
    a = _args(cabi, m=1000, fanout=3)
    a["ws_bytes"] = 1000 * 3 * 8 - 1
    rc, err = _hop(cabi, a)
    assert rc == 1 and "too small" in err
    a = _args(cabi)
    a["ws"] = (FAKE << 8) + 4
    rc, err = _hop(cabi, a)
    assert rc == 1 and "aligned" in err
    # unsupported: more than 4096 visits per vertex, more than 2^31 vertices
    for R, T in ((4097, 1), (1, 4097), (64, 65), (2 ** 20, 2 ** 20)):
        rc, err = _hop(cabi, _args(cabi, R=R, T=T))
        assert rc == 3 and "4096" in err, (R, T)
    rc, err = _hop(cabi, _args(cabi, n_major=2 ** 31 + 1))
    assert rc == 3 and "32-bit" in err


def test_the_visit_limit_is_4096_and_an_empty_frontier_launches_nothing():
    from tch_geometric import _cabi as cabi
    nbytes = C.c_int64(-1)
    assert cabi.lib.tg_pinsage_hop_workspace_bytes(C.c_int64(5), C.c_int32(64), C.byref(nbytes)) == 0 and nbytes.value == 5 * 64 * 8
    for m, k in ((-1, 3), (5, 0), (5, 65)):
        assert cabi.lib.tg_pinsage_hop_workspace_bytes(C.c_int64(m), C.c_int32(k), C.byref(nbytes)) == 1
    assert cabi.lib.tg_pinsage_hop_workspace_bytes(C.c_int64(5), C.c_int32(3), None) == 1
    for R, T in ((2048, 2), (64, 64), (4096, 1), (1, 4096)):  # V = 4096 is accepted: m = 0 returns TG_OK, no buffer is looked at
        a = _args(cabi, m=0, R=R, T=T, n_major=2 ** 31)
        a["hin"].vertices = None
        a["hout"].cnt = a["hout"].offsets = a["hout"].neighbors = a["hout"].parents = None
        a["visits"] = a["status"] = a["ws"] = None
        a["ws_bytes"] = 0
        rc, err = _hop(cabi, a)
        assert rc == 0, err
    rc, err = _hop(cabi, _args(cabi, m=0, R=4097, T=1))       # the limits hold for an empty frontier too
    assert rc == 3 and "4096" in err


# ---------------------------------------------------------------- the loader's refusals need no device
def _graph(n=6):
    from tch_geometric.transforms import Graph
    ei = torch.tensor([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]])
    return Graph(edge_index=ei, num_nodes=n, x=torch.zeros(n, 2))


@pytest.mark.parametrize("kw,exc,match", [
    (dict(num_neighbors=[]), ValueError, "at least one layer"),
    (dict(num_neighbors=[3, 65]), ValueError, "1..64"),
    (dict(num_neighbors=[0]), ValueError, "1..64"),
    (dict(batch_size=0), ValueError, "batch_size"),
    (dict(n_walks=0), ValueError, "n_walks"),
    (dict(walk_length=0), ValueError, "walk_length"),
    (dict(n_walks=64, walk_length=65), ValueError, "4096"),
    (dict(termination=1.0), ValueError, "termination"),
    (dict(termination=-0.1), ValueError, "termination"),
    (dict(termination=float("nan")), ValueError, "termination"),
    (dict(prefetch=0), ValueError, "prefetch"),
    (dict(call_id0=-1), ValueError, "call_id0"),
    (dict(input_nodes=torch.tensor([0, 6])), IndexError, "outside"),
    (dict(input_nodes=torch.tensor([-1, 2])), IndexError, "outside"),
    (dict(input_nodes=torch.tensor([0, 1, 0, 3]), batch_size=3), ValueError, "twice"),
    (dict(input_nodes=torch.tensor([0, 1, 2, 0]), batch_size=2, shuffle=True), ValueError, "twice"),
])
def test_loader_refusals_need_no_device(kw, exc, match):
    from tch_geometric import PinSAGELoader
    args = dict(num_neighbors=[3, 2], batch_size=2, n_walks=10, walk_length=2, device="cuda:0")
    args.update(kw)
    fan = args.pop("num_neighbors")
    with pytest.raises(exc, match=match):
        PinSAGELoader(_graph(), fan, **args)
