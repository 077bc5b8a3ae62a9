"""A deterministic detector for the first convention of include/tchgeo.h: every entry point is stream-ordered and
never synchronises, allocates or frees.

`run_lagging(case)` runs a case on a non-default stream whose work is held back by a blocker, so that the device runs
BEHIND the host for the whole call.  Ordering then does not depend on who wins a race:

1. reference, default stream: the call with the real inputs -> `want`, with decoy inputs -> `other` (valid, in-range
   inputs of the same shapes: the listed tensors with their elements permuted).  `want != other` and `want` is not all
   zeros, else the case has no power and FAILS.  These runs also load the code objects.
2. every buffer of the measured run -- inputs (holding the decoys), outputs, workspaces, snapshots -- is allocated on
   the default stream, the device is synchronised, nothing is freed before the end.
3. on the side stream `s`: a blocker (`torch.cuda._sleep`) with an event behind it; copies of the real inputs over the
   decoys; a ZERO-fill of every output and workspace buffer (zeros, not poison: a mis-ordered kernel that takes an
   offset or an index from them reads 0, which is in range); the call, or the whole protocol of calls; `returned_early =
   not event.query()`; copies of the outputs into the snapshots.
4. `s.synchronize()`, then snapshots == want, bit for bit.

A first kernel on another stream reads decoys and has its output zeroed; a middle one reads a zeroed workspace; a last
one is overwritten by the zero-fill; a host wait inside a call that promises none makes `returned_early` false.

How a case gets buffers it does not allocate itself: the wrappers of tch_geometric._cabi allocate outputs and workspaces
with torch.empty / zeros / full / *_like.  While a case runs, `Arena` stands in for the name `torch` in that module (and
in the modules a case names): the reference run records every device allocation (and hands out ZEROED memory, so that
words a launch never writes compare equal), the measured run hands out the buffers of step 2 in the same order.  A case
allocates through the same object (`T.empty(...)`).  What torch itself allocates inside an operator (a cumsum, a cat)
comes from the caching allocator on `s`; torch orders those itself.

Classes: ASYNC -- the header or wrapper promises no synchronisation and no read-back: `returned_early` is asserted;
READS_BACK -- wrappers and operator-surface functions that size their results from a read-back: values only.  For the
operator surface (C++, allocates through ATen) nothing can be zero-filled; the case is first run once on `s` with the
decoys so that the blocks the allocator hands out again hold a valid run's in-range words.

Blocker length.  Measured on the MI355X: the host wall time of each case's default-stream call, not waited for.  The
slowest is part[world=3, filtered] (the emulated three-rank tg_part_* protocol under a filter, its per-hop size
read-backs included) with 2.1 to 2.5 ms over four runs, 2.490 ms at most; the slowest ASYNC case is hgt_sample_batched
with 0.352 ms.  LAG_MS = 50 ms is 20 times the largest, rounded up.  `torch.cuda._sleep` counts cycles; cycles per
millisecond are calibrated once per session with two events.  The test module prints the slowest call of its run when it
ends (pytest -s).  One limit: the blocker delays the CALLER's stream, not the library's internal side stream
(csrc/ns_homo_win.hip WinSide), so a fork that does not wait for the caller is caught, a missing final join only if the
snapshots happen to be incomplete.
"""
import contextlib
import importlib
import time

import torch

ASYNC, READS_BACK = "async", "reads back"

HOST_ENQUEUE_MS_MEASURED = 2.490   # part[world=3, filtered], the slowest case of the table on the MI355X
LAG_MS = 50.0                       # 20 x 2.490 ms = 49.8 ms, rounded up

_FACTORIES = ("empty", "zeros", "full", "ones")
_LIKE = ("empty_like", "zeros_like", "full_like", "ones_like")


class StreamOrderError(AssertionError):
    pass


class Arena:
    """Stands in for the module `torch`: device allocations are recorded (mode "record") or served from buffers made
    beforehand (mode "replay"); everything else is torch's."""

    def __init__(self):
        self.mode, self.log, self.bufs, self.next = "record", [], [], 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _serve(self, shape, dtype, device, fill):
        shape = tuple(int(x) for x in shape)
        if self.mode == "record":
            self.log.append((shape, dtype, device))
            t = torch.zeros(shape, dtype=dtype, device=device)
        else:
            if self.next >= len(self.log) or self.log[self.next] != (shape, dtype, device):
                raise StreamOrderError("allocation %d of the measured run is %r, the reference run's was %r -- a size "
                                       "read back from the device differs" % (
                                           self.next, (shape, dtype), self.log[self.next][:2] if self.next < len(self.log) else None))
            t = self.bufs[self.next]
            self.next += 1
        if fill:
            t.fill_(fill)
        return t

    def _factory(self, name, *size, dtype=None, device=None, **kw):
        fill = 0
        if name == "full":
            size, fill = size[:-1], size[-1]
            if "fill_value" in kw:
                fill = kw.pop("fill_value")
        elif name == "ones":
            fill = 1
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dev = torch.device(device) if device is not None else torch.device("cpu")
        if dev.type != "cuda" or kw:
            return getattr(torch, name)(*size, *((fill,) if name == "full" else ()), dtype=dtype, device=device, **kw)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return self._serve(size, dtype or torch.get_default_dtype(), dev, fill)

    def _like(self, name, src, *args, **kw):
        if not src.is_cuda or kw or not src.is_contiguous():
            return getattr(torch, name)(src, *args, **kw)
        fill = args[0] if name == "full_like" else 1 if name == "ones_like" else 0
        return self._serve(src.shape, src.dtype, src.device, fill)

    def prepare_replay(self):
        """Step 2: the buffers of the measured run, on the current (default) stream."""
        self.bufs = [torch.empty(shape, dtype=dtype, device=device) for shape, dtype, device in self.log]
        self.mode, self.next = "replay", 0

    def zero_all(self):
        for b in self.bufs:
            b.zero_()


for _name in _FACTORIES:
    setattr(Arena, _name, (lambda n: lambda self, *a, **k: self._factory(n, *a, **k))(_name))
for _name in _LIKE:
    setattr(Arena, _name, (lambda n: lambda self, *a, **k: self._like(n, *a, **k))(_name))


@contextlib.contextmanager
def _patched(arena, modules):
    saved = [(m, m.torch) for m in modules]
    for m in modules:
        m.torch = arena
    try:
        yield
    finally:
        for m, t in saved:
            m.torch = t


class Case:
    """One launch chain.  names: the C entry points / wrappers the chain reaches (the table of
    test_stream_contract_cpu.py); cls: ASYNC or READS_BACK; make(dev) -> dict of real device input tensors (made on the
    default stream); vary: the keys whose elements are permuted for the decoy run (empty: the call has no device input
    and the zero-fill alone carries the check); call(inp, T) -> sequence of output tensors, every device buffer taken
    from T (or allocated by a patched module); modules: names of further modules whose `torch` the arena replaces; own_buffers:
    False for the operator surface (see the module docstring)."""

    def __init__(self, id, names, cls, make, call, vary=(), modules=(), own_buffers=True):
        self.id, self.names, self.cls, self.make, self.call = id, tuple(names), cls, make, call
        self.vary, self.modules, self.own_buffers = tuple(vary), tuple(modules), own_buffers

    def __repr__(self):
        return self.id


def decoy_of(real, vary, seed=0x0DEC01):
    """The decoy inputs: the tensors named by `vary` with their elements permuted (same shape, same value range, so
    every id stays in range), the others as they are."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    out = {}
    for k, v in real.items():
        if k in vary and v.numel() > 1:
            perm = torch.randperm(v.numel(), generator=g).to(v.device)
            out[k] = v.reshape(-1)[perm].reshape(v.shape).contiguous()
        else:
            out[k] = v.clone()
    return out


_state = {}
enqueue_ms = {}   # case id -> host wall time of the case's default-stream call (not waited for), for LAG_MS


def side_stream():
    """The one extra stream of the process's stream tests."""
    if "s" not in _state:
        _state["s"] = torch.cuda.Stream()
    return _state["s"]


def cycles_per_ms():
    if "cpm" not in _state:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1 << 20)               # warm-up: loads the kernel
        torch.cuda.synchronize()
        probe = 1 << 26
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _state["cpm"] = probe / max(a.elapsed_time(b), 1e-3)
    return _state["cpm"]


def block(stream, ms=None):
    """Enqueues the blocker on `stream` -> the event behind it (unfinished for about `ms`)."""
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles_per_ms() * (LAG_MS if ms is None else ms)))
        ev.record()
    return ev


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype.is_floating_point else a,
                                                                     b.view(torch.uint8) if b.dtype.is_floating_point else b)


def _outputs(x):
    return [t for t in x if t is not None]


def run_lagging(case, dev=None):
    """-> dict(returned_early, mismatches: indices of the outputs that differ from the default-stream run).  Raises
    StreamOrderError when the case has no power."""
    from tch_geometric import _cabi
    dev = dev or torch.device("cuda", torch.cuda.current_device())
    modules = (_cabi,) + tuple(importlib.import_module(m) for m in case.modules)
    s = side_stream()
    real = case.make(dev)
    decoy = decoy_of(real, case.vary)

    # 1. reference runs on the default stream
    ref = Arena()
    with _patched(ref, modules):
        want = [t.clone() for t in _outputs(case.call({k: v.clone() for k, v in real.items()}, ref))]
        log = list(ref.log)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = case.call({k: v.clone() for k, v in decoy.items()}, ref)
        host_ms = (time.perf_counter() - t0) * 1e3
        other = [t.clone() for t in _outputs(got)]
    torch.cuda.synchronize()
    enqueue_ms[case.id] = host_ms
    if not any(bool(w.ne(0).any()) for w in want if w.numel()):
        raise StreamOrderError("%s has no power: the reference outputs are all zeros" % case.id)
    differs = [i for i, w in enumerate(want) if i >= len(other) or not _same(w, other[i])]
    if case.vary and not any(bool(want[i].ne(0).any()) for i in differs):
        raise StreamOrderError("%s has no power: the decoy inputs give the same outputs" % case.id)

    if not case.own_buffers:                     # the operator surface: see the module docstring
        with torch.cuda.stream(s):
            case.call({k: v.clone() for k, v in decoy.items()}, torch)
        s.synchronize()

    # 2. every buffer of the measured run, then a device-wide wait
    arena = Arena()
    arena.log = log
    arena.prepare_replay()
    inp = {k: v.clone() for k, v in decoy.items()}
    snaps = [torch.empty_like(w) for w in want]
    torch.cuda.synchronize()

    # 3. the measured run, behind the blocker
    ev = block(s)
    with torch.cuda.stream(s), _patched(arena, modules):
        for k in inp:
            inp[k].copy_(real[k])
        arena.zero_all()
        outs = _outputs(case.call(inp, arena))
        returned_early = not ev.query()
        mismatches = []
        if len(outs) != len(want):
            mismatches = list(range(max(len(outs), len(want))))
        else:
            for i, (snap, o) in enumerate(zip(snaps, outs)):
                if o.shape != snap.shape or o.dtype != snap.dtype:
                    mismatches.append(i)
                else:
                    snap.copy_(o)

    # 4. compare
    s.synchronize()
    mismatches += [i for i, (snap, w) in enumerate(zip(snaps, want)) if i not in mismatches and not _same(snap, w)]
    torch.cuda.synchronize()
    del outs, inp
    return dict(returned_early=returned_early, mismatches=sorted(mismatches), host_ms=host_ms, n_outputs=len(want))


def check(case, dev=None):
    """run_lagging plus the assertions of the case's class."""
    r = run_lagging(case, dev)
    assert not r["mismatches"], "%s: outputs %s of the run behind the blocker differ from the default-stream run -- a launch, " \
        "memset, copy or scan of this chain is not on the caller's stream" % (case.id, r["mismatches"])
    if case.cls == ASYNC:
        assert r["returned_early"], "%s: the call returned only after the blocker (%.0f ms) had finished -- it waits on the " \
            "host, or the blocker is too short for its enqueue (%.2f ms on the default stream)" % (case.id, LAG_MS, r["host_ms"])
    return r
