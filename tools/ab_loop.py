"""The A/B of library builds INSIDE one process, on the same buffers (why one process: tools/ab_same_process.py), for a set
of cases: `python tools/ab_<cases>.py parent.so parent.so new.so [--out FILE]` (paths relative to the repo root; "-" = the
default build).  The case sets: tools/ab_dedup.py (the node dedup operators) and tools/ab_chunk_pairs.py (count + emit of the
induced, grouped induced, cluster and full-neighbour pairs).  A case set builds `cases` (name -> a call that launches the
operator once through tch_geometric._cabi) and calls run(cases): three alternating rounds, HIP events, ms per call.  With
the SAME build given first and second, the gap between those two medians is the noise floor of the run; every later
build's median is held against the first build's median + twice that gap."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

from tch_geometric import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cases, warm=3, calls=20):
    args = sys.argv[1:]
    out_path = args.pop(args.index("--out") + 1) if "--out" in args else None
    paths = [a for a in args if a != "--out"]
    default, libs = _cabi.lib, []
    for i, path in enumerate(paths):
        h = default if path == "-" else C.CDLL(os.path.join(ROOT, path))
        h.tg_version.restype = h.tg_last_error.restype = C.c_char_p
        for fn in ("tg_ns_full_workspace_bytes", "tg_ns_full_count", "tg_ns_full_emit"):   # their wrappers pass plain ints
            getattr(h, fn).argtypes, getattr(h, fn).restype = getattr(default, fn).argtypes, getattr(default, fn).restype
        libs.append(("%d:%s" % (i, path), h))
    ms = {c: {name: [] for name, _ in libs} for c in cases}
    for rnd in range(3):
        for name, h in libs:
            _cabi.lib = h
            for c, call in cases.items():
                for _ in range(warm):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                ms[c][name].append(e0.elapsed_time(e1) / calls)
    _cabi.lib = default
    res = {}
    for c in cases:
        med = {name: round(statistics.median(v), 5) for name, v in ms[c].items()}
        entry = {"ms_per_call_median": med, "ms_per_call_rounds": {k: [round(x, 5) for x in v] for k, v in ms[c].items()}}
        if len(libs) >= 3 and paths[0] == paths[1]:
            (a, _), (b, _) = libs[0], libs[1]
            gap = abs(med[a] - med[b])
            entry["noise_floor_ms"] = round(gap, 5)
            entry["verdict"] = {name: "ok" if med[name] <= med[a] + 2 * gap else "slower by %.5f ms" % (med[name] - med[a])
                                for name, _ in libs[2:]}
        res[c] = entry
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")
    return res
