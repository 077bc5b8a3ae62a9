"""One round of the label-propagation partitioner (tg_lp_propose, tg_lp_commit) on an RMAT graph (16 edges per node, directed,
its CSC) at Cluster-GCN's part counts, in one process.  Prints one JSON line:
  propose  ms and entries/s of _WAVE and of AUTO under several wave_max, HIP events, ROUNDS interleaved medians and their
           spread; labels are a random partition (the first round's access pattern: no locality in the gathers)
  commit   ms of tg_lp_commit on that propose's skey with cap = ceil(1.1 n / P); label and size are restored un-timed
  torch    the same round as a torch composition on the same device: the (v, label[w]) pairs as one sorted key array,
           unique_consecutive counts, a segmented arg-max by scatter_reduce, then a stable sort of the movers and a rank by
           searchsorted for admission.  Its (target, gain) words and its committed labels are checked against the kernels'
No device setting is touched.  The timing helpers are tools/bench_full_neighbor_loader.py's."""
import json
import os
import sys

import torch

import bench_full_neighbor_loader as bf

SCALE = int(os.environ.get("SCALE", "22"))
PARTS = tuple(int(x) for x in os.environ.get("PARTS", "1500,15000").split(","))
SEED = 0x1B


def torch_propose(ptrs, indices, label, P):
    """-> (best [n] or -1, gain [n]) of every vertex"""
    n = ptrs.numel() - 1
    v = torch.repeat_interleave(torch.arange(n, device=ptrs.device), ptrs[1:] - ptrs[:-1], output_size=indices.numel())
    ok = indices != v
    keys, _ = torch.sort(v[ok] * P + label[indices[ok]])
    pair, cnt = torch.unique_consecutive(keys, return_counts=True)
    pv, pl = pair // P, pair % P
    mine = pl == label[pv]
    own = torch.zeros(n, dtype=torch.int64, device=ptrs.device).index_put_((pv[mine],), cnt[mine])
    score = torch.where(mine, torch.zeros_like(cnt), cnt * P + (P - 1 - pl))        # the larger count, then the smaller label
    top = torch.zeros(n, dtype=torch.int64, device=ptrs.device).scatter_reduce_(0, pv, score, "amax")
    gain = top // P - own
    return torch.where((top > 0) & (gain > 0), P - 1 - top % P, torch.full_like(top, -1)), gain


def torch_commit(label, size, cap, skey_u63, P):
    """skey_u63: the skey words shifted right by one (a non-negative int64 in the same order); -> the new labels"""
    free = (cap - size).clamp(min=0)
    v = torch.nonzero(skey_u63 != (1 << 63) - 1).view(-1)
    k, order = torch.sort(skey_u63[v], stable=True)
    v, target = v[order], k >> 43
    rank = torch.arange(v.numel(), device=v.device) - torch.searchsorted(target, target)
    ok = rank < free[target]
    return label.index_put((v[ok],), target[ok])


def main():
    from tch_geometric import _cabi, _cabi_lp as lp
    dev = torch.device("cuda:0")
    n = 1 << SCALE
    row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
    ptrs, indices, _ = _cabi.coo_to_csx(row, col, n, n, True)
    del row, col
    graph = _cabi.graph_view(ptrs, indices, indices32=indices.to(torch.int32), ptrs32=ptrs.to(torch.int32))
    deg = ptrs[1:] - ptrs[:-1]
    res = {"config": "RMAT-%d CSC, %d entries, longest row %d, %d rows above %d entries; u32 shadows; %d interleaved rounds"
                     % (SCALE, indices.numel(), int(deg.max()), int((deg > lp.LP_WAVE_MAX).sum()), lp.LP_WAVE_MAX, bf.ROUNDS),
           "constants": {"TG_LP_WAVE_MAX": lp.LP_WAVE_MAX, "TG_LP_LDS_LABELS": lp.LP_LDS_LABELS}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    for P in PARTS:
        label0 = torch.randint(0, P, (n,), device=dev, generator=gen, dtype=torch.int32)
        label, label64 = label0.clone(), label0.to(torch.int64)
        size0, size = torch.empty(P, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int64, device=dev)
        state = torch.zeros(3, dtype=torch.int64, device=dev)
        status = state[2:].view(torch.int32)[:1]
        lp.lp_sizes(label0, P, size0, status)
        cap = -(-11 * n // (10 * P))
        forms = [("wave", lp.FORM_WAVE, 0), ("auto", lp.FORM_AUTO, 0)] + [("auto_wave_max_%d" % wm, lp.FORM_AUTO, wm) for wm in (64, 256)]
        runs, skeys = {}, {}
        for key, form, wm in forms:
            ws = lp.lp_workspace(n, P, dev, form, wm)
            skeys[key] = torch.empty(n, dtype=torch.int64, device=dev)
            call = lambda s=skeys[key], ws=ws, form=form, wm=wm: lp.lp_propose(graph, label0, P, SEED, 0, s, state[:1], status, ws, form, wm)
            call()
            runs["propose_" + key] = lambda call=call: bf.timed(call)
        for key, _, _ in forms[1:]:
            assert torch.equal(skeys["wave"], skeys[key]), key
        skey, ws = skeys["auto"], lp.lp_workspace(n, P, dev)

        def restore():
            label.copy_(label0)
            size.copy_(size0)
        runs["commit"] = lambda: bf.timed(lambda: lp.lp_commit(label, size, P, cap, skey, state[1:2], status, ws), before=restore)
        best, gain = torch_propose(ptrs, indices, label64, P)
        mover = skey != -1
        assert torch.equal(best >= 0, mover) and torch.equal(best[mover], (skey[mover] >> 44) & 0xFFFFF)
        assert torch.equal(4095 - gain[mover].clamp(max=4095), (skey[mover] >> 32) & 4095)
        u63 = (skey >> 1) & ((1 << 63) - 1)
        restore()
        lp.lp_commit(label, size, P, cap, skey, state[1:2], status, ws)
        assert torch.equal(torch_commit(label64, size0, cap, u63, P), label.to(torch.int64)) and int(state[2]) == 0
        del best, gain
        runs["torch_propose"] = lambda: bf.timed(lambda: torch_propose(ptrs, indices, label64, P), warm=1, reps=3)
        runs["torch_commit"] = lambda: bf.timed(lambda: torch_commit(label64, size0, cap, u63, P), warm=1, reps=3)
        part = bf.interleaved(runs)
        for key, s in part.items():
            if "propose" in key:
                s["entries_per_s"] = round(indices.numel() / (s["ms_median_of_medians"] * 1e-3), 0)
        part.update({"movers": int(mover.sum()), "cap": cap,
                     "torch_over_auto_propose": round(part["torch_propose"]["ms_median_of_medians"] / part["propose_auto"]["ms_median_of_medians"], 3),
                     "torch_over_commit": round(part["torch_commit"]["ms_median_of_medians"] / part["commit"]["ms_median_of_medians"], 3)})
        res["P_%d" % P] = part
        print(json.dumps({"P_%d" % P: part}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
