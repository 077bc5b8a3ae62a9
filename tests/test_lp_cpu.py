"""The label-propagation partitioner without a GPU: the restatement (helpers_lp) against a brute-force dict version on three
hand graphs; the planted-partition check; the workspace formula; every refusal happens before a launch; the header is C99; the
exports equal the header; lp_partition's ValueErrors.  test_restatement_against_brute_force and
test_planted_partition_halves_the_cut need nothing but the helper."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_lp as hl
from helpers_labor import named_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_lp.h")
FAKE, BIG = 0x10000, 1 << 50   # a non-null address that is never read: every call below is refused before a launch

sym = lambda pairs: [e for a, b in pairs for e in ((a, b), (b, a))]
HAND = {   # name -> (n, directed entries (x, w): w stands in x's row, labels)
    "two_triangles": (6, sym([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]), [0, 1, 0, 1, 1, 0]),
    "star": (7, sym([(0, i) for i in range(1, 7)]) + [(0, 0), (0, 3), (0, 3)], [0, 1, 1, 2, 2, 2, 0]),  # a self loop, (0, 3) thrice
    "bad_entries": (5, sym([(0, 1), (1, 2), (3, 4)]) + [(2, -1), (2, 5), (4, 4)], [0, 0, 1, 2, 0]),
}


def brute(n, entries, label, P, cap, seed, rnd):
    """one round by dicts and Python ints -> (skey list, cut, label, size, moved)"""
    skey, cut = [], 0
    for v in range(n):
        cnt = {}
        for x, w in entries:
            if x == v and 0 <= w < n and w != v:
                cnt[label[w]] = cnt.get(label[w], 0) + 1
                cut += label[w] != label[v]
        own = cnt.pop(label[v], 0)
        best = min(cnt, key=lambda l: (-cnt[l], l)) if cnt else None
        if best is None or cnt[best] <= own:
            skey.append(2 ** 64 - 1)
        else:
            h = int(named_draw(seed, rnd, hl.TAG_LP, np.array([v]), 0, 0)[0][0])
            skey.append((best << 44) | ((4095 - min(cnt[best] - own, 4095)) << 32) | h)
    size = [label.count(l) for l in range(P)]
    free, label, moved = [max(0, cap - s) for s in size], list(label), 0
    for k, v in sorted((k, v) for v, k in enumerate(skey) if k != 2 ** 64 - 1):
        if free[k >> 44] > 0:
            free[k >> 44] -= 1
            size[label[v]] -= 1
            size[k >> 44] += 1
            label[v] = k >> 44
            moved += 1
    return skey, cut, label, size, moved


@pytest.mark.parametrize("name", list(HAND))
@pytest.mark.parametrize("cap", [1, 3, 9])
def test_restatement_against_brute_force(name, cap):
    n, entries, label = HAND[name]
    ptrs = np.concatenate([[0], np.cumsum(np.bincount([x for x, _ in entries], minlength=n))])
    idx = np.array([w for x, w in sorted(entries, key=lambda e: e[0])])
    for rnd in range(3):
        skey, cut, new_label, size, moved = brute(n, entries, label, 3, cap, 11, rnd)
        got_skey, got_cut = hl.propose(ptrs, idx, label, 3, 11, rnd)
        assert got_skey.tolist() == skey and got_cut == cut
        got = hl.commit(label, np.bincount(label, minlength=3), cap, got_skey, 3)
        assert (got[0].tolist(), got[1].tolist(), got[2], got[3]) == (new_label, size, moved, 0)
        label = new_label


def test_planted_partition_halves_the_cut():
    """4 000 vertices, 16 communities, P = 16, slack 1.1, from range_partition, 40 rounds: the cut share falls below half the
    initial one and no part ever exceeds cap"""
    ptrs, idx = hl.planted()
    n, P, cap = len(ptrs) - 1, 16, hl.cap_of(4000, 16, 1.1)
    label, size = np.arange(n) * P // n, None
    size = np.bincount(label, minlength=P)
    cuts = []
    for r in range(40):
        skey, cut = hl.propose(ptrs, idx, label, P, 0, r)
        label, size, _, _ = hl.commit(label, size, cap, skey, P)
        cuts.append(cut)
        assert size.max() <= cap and size.tolist() == np.bincount(label, minlength=P).tolist()
    final = hl.propose(ptrs, idx, label, P, 0, 40)[1]
    print("cut share %.3f -> %.3f" % (cuts[0] / len(idx), final / len(idx)))
    assert final < cuts[0] / 2


@pytest.fixture(scope="module")
def ops():
    from tch_geometric import _cabi_lp
    _cabi_lp.lib.tg_last_error.restype = C.c_char_p
    return _cabi_lp


r256 = lambda x: (x + 255) // 256 * 256


def test_workspace_formula(ops):
    for n in (0, 1, 1000, 100000):
        for P in (1, 2048, 2049, 1 << 20):
            for form in (0, 1, 2):
                propose = 256 + (r256(4 * n) if form == 0 else 0) + (32 * r256(8 * P) if form != 1 and P > 2048 else 0)
                commit = r256(8 * P) + r256(4 * P) + 2 * r256(4 * n) + r256(8 * n)      # and the sort's temporary storage
                got, taken = ops.lp_workspace_bytes(n, P, form, 64)
                assert taken == form and got % 256 == 0 and got >= max(propose, commit), (n, P, form)
                if propose > commit + (1 << 20) + 16 * n:     # far beyond any temporary storage: propose sets the size
                    assert got == propose, (n, P, form)
    assert ops.lp_workspace_bytes(1000, 1 << 20, 2)[0] == 256 + 32 * 8 * (1 << 20)


def graph(n_major=100, n_edges=500, ptrs=FAKE):
    from tch_geometric import _cabi
    g = _cabi.TgGraph()
    g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, FAKE, n_major, n_edges
    return g


def propose(ops, g="default", label=FAKE, P=4, form=0, wave_max=0, skey=FAKE, cut=FAKE, status=FAKE, ws=FAKE, ws_bytes=BIG, **kw):
    g = graph(**kw) if g == "default" else g
    return ops.lib.tg_lp_propose(C.byref(g) if g is not None else None, label, P, 1, 2, form, wave_max, skey, cut, status, ws,
                                 ws_bytes, None)


def commit(ops, label=FAKE, size=FAKE, n=100, P=4, cap=30, skey=FAKE, moved=FAKE, status=FAKE, ws=FAKE, ws_bytes=BIG):
    return ops.lib.tg_lp_commit(label, size, n, P, cap, skey, moved, status, ws, ws_bytes, None)


def sizes(ops, label=FAKE, n=100, P=4, size=FAKE, status=FAKE):
    return ops.lib.tg_lp_sizes(label, n, P, size, status, None)


REFUSALS = [
    (propose, dict(g=None), "null graph"), (propose, dict(P=0), "n_parts = 0"), (propose, dict(P=(1 << 20) + 1), "n_parts"),
    (propose, dict(form=3), "unknown form"), (propose, dict(form=-1), "unknown form"), (propose, dict(wave_max=-1), "wave_max"),
    (propose, dict(wave_max=513), "wave_max"), (propose, dict(n_major=-1), "negative graph"),
    (propose, dict(ptrs=None), "null graph arrays"), (propose, dict(label=None), "null label"),
    (propose, dict(skey=None), "null label"), (propose, dict(cut=None), "null label"), (propose, dict(status=None), "null label"),
    (propose, dict(ws=None), "workspace"), (propose, dict(ws_bytes=255), "workspace"), (propose, dict(ws_bytes=-1), "workspace_bytes"),
    (propose, dict(ws=FAKE + 8), "16-byte aligned"),
    (commit, dict(n=-1), "n = -1"), (commit, dict(P=0), "n_parts = 0"), (commit, dict(cap=0), "cap = 0"),
    (commit, dict(label=None), "null label"), (commit, dict(size=None), "null label"), (commit, dict(skey=None), "null label"),
    (commit, dict(moved=None), "null label"), (commit, dict(status=None), "null label"), (commit, dict(ws=None), "workspace"),
    (commit, dict(ws_bytes=1024), "workspace"), (commit, dict(ws=FAKE + 4), "16-byte aligned"),
    (sizes, dict(P=0), "n_parts = 0"), (sizes, dict(label=None), "null label"), (sizes, dict(size=None), "null label"),
    (sizes, dict(status=None), "null label"), (sizes, dict(n=-1), "n = -1"),
]


@pytest.mark.parametrize("call, kw, word", REFUSALS, ids=lambda x: x.__name__ if callable(x) else str(x))
def test_refusals_before_any_launch(ops, call, kw, word):
    assert call(ops, **kw) == 1                              # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_unsupported_sizes_and_empty_calls(ops):
    assert propose(ops, n_major=1 << 31) == 3                # TG_ERR_UNSUPPORTED
    assert propose(ops, n_edges=1 << 32) == 3 and commit(ops, n=1 << 31) == 3 and sizes(ops, n=1 << 31) == 3
    assert propose(ops, n_major=0, label=None, skey=None, cut=None, status=None, ws=None, ws_bytes=0) == 0   # launch nothing
    assert commit(ops, n=0, label=None, size=None, skey=None, moved=None, status=None, ws=None, ws_bytes=0) == 0


def test_header_is_c99_and_the_exports_equal_it(ops):
    src = ('#include "tchgeo_lp.h"\nint main(void) { return TG_LP_MAX_PARTS == 1048576 && TG_TAG_LP == 20u && '
           'TG_LP_FORM_GROUP == 2 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) == ["tg_lp_commit", "tg_lp_propose", "tg_lp_sizes", "tg_lp_workspace_bytes"]
    for name in declared:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    defines = dict(re.findall(r"#define TG_LP_(\w+) (\d+)", text))
    for name in ("MAX_PARTS", "WAVE_MAX", "LDS_LABELS", "WAVE_GROUPS", "GROUP_GROUPS", "DENSE_GROUPS"):
        assert int(defines[name]) == getattr(ops, "LP_" + name), name
    assert ops.TAG_LP == hl.TAG_LP == 20 and "#define TG_TAG_LP 20u" in text


def test_lp_partition_refuses_before_any_device_work():
    import tch_geometric
    assert tch_geometric.lp_partition is tch_geometric.loader.lp_partition
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    good = dict(edge_index=ei, num_nodes=3, num_parts=2, device="cuda:0")
    for kw in (dict(edge_index=ei[0]), dict(edge_index=ei.to(torch.int32)), dict(num_nodes=0), dict(num_nodes=1 << 31),
               dict(num_parts=0), dict(num_parts=(1 << 20) + 1), dict(slack=0.9), dict(slack=float("nan")), dict(rounds=-1),
               dict(seed=-1), dict(seed=1 << 64), dict(init=torch.zeros(2, dtype=torch.int64)), dict(init=torch.zeros(3))):
        with pytest.raises(ValueError):
            tch_geometric.lp_partition(**dict(good, **kw))
