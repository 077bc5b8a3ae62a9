"""tg_sketch_* without a GPU: the restatement (helpers_sketch) against exact balls on one hand graph; the byte and workspace
formulas; every refusal happens before a launch; the header is C99; the exports equal the header; the loader's ValueErrors.
Only test_restatement_against_exact_balls needs nothing but the helper and passes without the feature."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_sketch as hk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tchgeo_sketch.h")
FAKE, BIG = 0x10000, 1 << 50   # a non-null aligned address that is never read: every call below is refused before a launch


def test_restatement_against_exact_balls():
    # a path 0-1-2-3, a triangle 4-5-6 with the pendant 7 on 6, the isolated 8; a parallel entry and a self loop
    pairs = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (4, 6), (6, 7)]
    edges = sorted([e for a, b in pairs for e in ((a, b), (b, a))] + [(1, 2), (5, 5)])
    ptrs = np.cumsum([0] + [sum(1 for x, _ in edges if x == r) for r in range(9)])
    indices = np.array([w for _, w in edges])
    hops = [hk.init(9, 64, 8, 7)]
    for _ in range(3):
        hops.append(hk.propagate(ptrs, indices, *hops[-1])[:2])
    balls = hk.balls(ptrs, indices, 3)
    assert balls[2][0] == {0, 1, 2} and balls[3][7] == {4, 5, 6, 7} and balls[3][8] == {8}
    for l in range(4):
        for x in range(9):
            members = sorted(balls[l][x])
            assert np.array_equal(hops[l][0][x], hops[0][0][members].min(0)) and np.array_equal(hops[l][1][x], hops[0][1][members].max(0))
    assert (hops[0][1] != 0).sum(1).tolist() == [1] * 9 and 1 <= hops[0][1].max() <= 33
    out = hk.links(hops, [0, 4, 8, 9], [0, 7, 3, 0])
    assert out["match"][0].diagonal().tolist() == [64] * 3 and out["status"] == 2 and not out["usum"][3].any()
    assert out["nzero"][2, 0].tolist() == [255] * 3 and out["uzero"][2, 0, 0] >= 253   # {8} against N_1(3) = {2, 3}
    assert hk.pack(*hops[0]).shape == (9, 128) and hk.pack(*hops[0])[0, 64:].view(np.uint8).tolist() == hops[0][1][0].tolist()


@pytest.fixture(scope="module")
def ops():
    from tch_geometric import _cabi_sketch
    _cabi_sketch.lib.tg_last_error.restype = C.c_char_p
    return _cabi_sketch


def params(ops, n_perm=128, hll_p=8, hops=2, reserved=0):
    return ops.TgSketchParams(n_perm, hll_p, hops, reserved, 5)


def call(ops, fn, p="default", g="default", n=100, n_edges=500, form=0, tuning=None, status=FAKE, ws=FAKE, ws_bytes=BIG,
         prev=FAKE, nxt=FAKE + (1 << 30), sketch=FAKE, src=FAKE, dst=FAKE, out="default", m=4, ptrs=FAKE, **kw):
    from tch_geometric import _cabi
    p = params(ops, **kw) if p == "default" else p
    ref = lambda s: C.byref(s) if s is not None else None
    if fn == "init":
        return ops.lib.tg_sketch_init(ref(p), n, sketch, None)
    if fn == "propagate":
        if g == "default":
            g = _cabi.TgGraph()
            g.ptrs, g.indices, g.n_major, g.n_edges = ptrs, FAKE, n, n_edges
        return ops.lib.tg_sketch_propagate(ref(g), ref(p), prev, nxt, form, ref(tuning), status, ws, ws_bytes, None)
    if out == "default":
        out = ops.TgSketchLinkOut(*[FAKE] * 5)
    return ops.lib.tg_sketch_links(ref(p), n, sketch, src, dst, ref(out), m, status, None)


BAD_PARAMS = [(dict(n_perm=0), "n_perm"), (dict(n_perm=96), "n_perm"), (dict(n_perm=320), "n_perm"), (dict(hll_p=7), "hll_p"),
              (dict(hll_p=11), "hll_p"), (dict(hops=0), "hops"), (dict(hops=4), "hops"), (dict(reserved=1), "reserved"),
              (dict(n=0), "n = 0"), (dict(n=(1 << 31) + 1), "n = "), (dict(p=None), "null params")]
REFUSALS = [(fn, kw, word) for fn in ("init", "propagate", "links") for kw, word in BAD_PARAMS] + [
    ("init", dict(sketch=None), "null sketch"), ("init", dict(sketch=FAKE + 4), "16-byte aligned"),
    ("propagate", dict(g=None), "null graph"), ("propagate", dict(ptrs=None), "null graph arrays"),
    ("propagate", dict(n_edges=-1), "n_edges"), ("propagate", dict(form=4), "unknown form"), ("propagate", dict(form=-1), "unknown form"),
    ("propagate", dict(prev=None), "null prev"), ("propagate", dict(nxt=None), "null prev"), ("propagate", dict(status=None), "null prev"),
    ("propagate", dict(nxt=FAKE), "overlap"), ("propagate", dict(nxt=FAKE + 256), "overlap"), ("propagate", dict(prev=FAKE + 8), "aligned"),
    ("propagate", dict(ws=None), "workspace"), ("propagate", dict(ws_bytes=255), "workspace"), ("propagate", dict(ws_bytes=-1), "workspace"),
    ("propagate", dict(form=3, ws_bytes=1000), "workspace"), ("propagate", dict(ws=FAKE + 4), "16-byte aligned"),
    ("links", dict(m=-1), "m = -1"), ("links", dict(m=1 << 31), "m = "), ("links", dict(out=None), "null out"),
    ("links", dict(sketch=None), "null sketch"), ("links", dict(src=None), "null sketch"), ("links", dict(dst=None), "null sketch"),
    ("links", dict(status=None), "null sketch"), ("links", dict(sketch=FAKE + 4), "16-byte aligned"),
] + [("propagate", dict(tuning=t), word) for t, word in (((-1, 0, 0), "wave_max"), ((0, -1, 0), "group_max"),
                                                          ((0, 0, 63), "split_seg"), ((0, 0, 2049), "split_seg"))] + \
    [("links", dict(out=tuple(None if k == i else FAKE for k in range(5))), "null match") for i in range(5)]


@pytest.mark.parametrize("fn, kw, word", REFUSALS)
def test_refusals_before_any_launch(ops, fn, kw, word):
    kw = dict(kw)
    if isinstance(kw.get("tuning"), tuple):
        kw["tuning"] = ops.TgSketchTuning(*kw["tuning"])
    if isinstance(kw.get("out"), tuple):
        kw["out"] = ops.TgSketchLinkOut(*kw["out"])
    assert call(ops, fn, **kw) == 1                          # TG_ERR_INVALID
    assert re.search(word, ops.lib.tg_last_error().decode()), ops.lib.tg_last_error()


def test_empty_calls_and_the_binding_s_own_refusals(ops):
    assert call(ops, "links", m=0, sketch=None, src=None, dst=None, status=None) == 0   # launches nothing
    for kw in (dict(n_perm=96), dict(n_perm=320), dict(hll_p=7), dict(hll_p=11), dict(hops=0), dict(hops=4), dict(seed=-1),
               dict(seed=1 << 64), dict(form=4), dict(wave_max=-1), dict(group_max=-1), dict(split_seg=63), dict(split_seg=4096)):
        with pytest.raises(ValueError):
            ops.Sketch(**kw)
    with pytest.raises(RuntimeError, match="an id outside the graph and row pointers"):
        ops.sketch_status_check(6, "here")
    ops.sketch_status_check(0, "here")


def test_byte_and_workspace_formulas(ops):
    r256 = lambda x: (x + 255) // 256 * 256
    for n_perm, hll_p, h in ((64, 8, 1), (128, 8, 2), (192, 9, 3), (256, 10, 3)):
        W = n_perm + (1 << hll_p) // 4
        sizes = ops.Sketch(h, n_perm, hll_p)
        assert sizes.row_words == W
        for n in (1, 700, 1 << 31):
            assert sizes.bytes(n) == ((h + 1) * n * W * 4, W)
        for n, E in ((1, 3), (700, 1050), (700, 0), (1 << 24, 1 << 28)):
            for form, wm, gm, sg in ((0, 0, 0, 0), (0, 64, 256, 64), (0, 512, 100, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 64), (3, 0, 0, 0)):
                got = ops.Sketch(h, n_perm, hll_p, 0, form, wm, gm, sg).workspace_bytes(n, E)
                over = lambda t: min(n, E // (t + 1))
                seg, wave = sg or 2048, wm or 64
                G = over(wave) if form == 0 else 0
                S = over(max(gm or 4096, wave)) if form == 0 else over(0)
                Q = S + E // seg
                want = 0 if form in (1, 2) else 256 + r256(4 * G) + r256(8 * S) + r256(8 * Q) + Q * W * 4
                assert got == (want, form), (n, E, form, wm, gm, sg)


def test_header_is_c99_and_the_exports_equal_it(ops):
    src = ('#include "tchgeo_sketch.h"\nint main(void) { tg_sketch_params p; tg_sketch_tuning t; tg_sketch_link_out o; '
           'p.hops = TG_SKETCH_MAX_HOPS; (void)t; (void)o; return p.hops == 3 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src.encode(), check=True)
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"TG_API\s+[\w\s\*]+?\b(tg_\w+)\s*\(", text)
    assert sorted(declared) == sorted(ops.EXPORTS) and len(declared) == 5
    for name in declared:
        assert hasattr(ops.lib, name) and getattr(ops.lib, name).argtypes
    for struct, name in ((ops.TgSketchLinkOut, "link_out"), (ops.TgSketchParams, "params"), (ops.TgSketchTuning, "tuning")):
        body = re.search(r"typedef struct \{([^}]*)\} tg_sketch_%s;" % name, text).group(1)
        assert [f for f, _ in struct._fields_] == re.findall(r"(\w+);", body), name
    defines = dict(re.findall(r"#define TG_SKETCH_(\w+) (\w+)", text))
    for name in ("MAX_HOPS", "WAVE_MAX", "GROUP_MAX", "SPLIT_SEG", "SPLIT_SEG_MIN", "WAVE_GROUPS", "GROUP_GROUPS"):
        assert int(defines[name]) == getattr(ops, "SKETCH_" + name), name
    assert (int(defines["TAG_MINHASH"], 16), int(defines["TAG_HLL"], 16)) == (hk.TAG_MINHASH, hk.TAG_HLL)


def test_the_loader_refuses_before_any_device_work():
    import tch_geometric
    from tch_geometric.transforms import Graph
    assert tch_geometric.SubgraphSketchLoader is tch_geometric.loader.SubgraphSketchLoader
    data = Graph(edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), num_nodes=3)
    for kw in (dict(hops=0), dict(hops=4), dict(n_perm=100), dict(n_perm=512), dict(hll_p=7), dict(hll_p=11), dict(seed=-1)):
        with pytest.raises(ValueError):
            tch_geometric.SketchData(data, device="cuda:0", **kw)
    sd = object.__new__(tch_geometric.SketchData)            # what a built one holds, without a device
    sd.sizes = tch_geometric._cabi_sketch.Sketch(2, 64, 8, 3)
    sd.hops, sd.n_perm, sd.hll_p, sd.seed, sd.n_nodes, sd.device = 2, 64, 8, 3, 3, torch.device("cuda:0")
    sd.sketch = torch.zeros((3, 3, 128), dtype=torch.int32)
    links = torch.tensor([[0, 1], [1, 2]])
    for kw in (dict(batch_size=0), dict(prefetch=0), dict(sketch_data=data), dict(edge_label_index=links[0]),
               dict(edge_label_index=links.to(torch.int32)), dict(edge_label_index=torch.tensor([[0, 3], [1, 2]])),
               dict(edge_label_index=torch.tensor([[0, -1], [1, 2]])), dict(edge_label=torch.ones(3))):
        with pytest.raises(ValueError):
            tch_geometric.SubgraphSketchLoader(**dict(dict(sketch_data=sd, edge_label_index=links), **kw))
    for name, value in (("n_perm", 128), ("hops", 3), ("seed", 4), ("sketch", torch.zeros((3, 3, 192), dtype=torch.int32))):
        kept = getattr(sd, name)
        setattr(sd, name, value)
        with pytest.raises(ValueError, match="other parameters"):
            tch_geometric.SubgraphSketchLoader(sd, links)
        setattr(sd, name, kept)
