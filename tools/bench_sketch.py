"""tg_sketch_propagate and tg_sketch_links on RMAT-24 (16 edges per node, directed, its CSC), n_perm 128, p = 8, h = 2, in one
process.  Prints one JSON line (the kept run: profiles/bench_sketch.json):
  hop      one propagate hop (hop 0 -> hop 1) per form, and AUTO under other thresholds: HIP events, ROUNDS interleaved medians
           and their spread; gathered bytes per second (entries x row bytes, what the fold reads) beside the HBM peak DESIGN.md
           section 5 uses.  Every form's words are compared with the wave form's.
  links    tg_sketch_links over LINKS random links, the same way
  torch    what a user does today, on the same device: the hop as Tensor.scatter_reduce_ with amin on the gathered MinHash rows
           (sign-flipped once outside the timing, so that int32 orders like uint32) and amax on the registers unpacked to a
           uint8 tensor, in chunks of TORCH_ENTRIES entries; the links as gathers and reductions on [L, h, h, W] in chunks of
           TORCH_LINKS links.  Its words are compared with the kernels' too.
No device setting is touched.  The timing helpers are tools/bench_full_neighbor_loader.py's."""
import json
import os
import sys

import torch

import bench_full_neighbor_loader as bf

SCALE = bf.SCALE
LINKS = int(os.environ.get("LINKS", str(1 << 20)))
NP, P, H = 128, 8, 2
TORCH_ENTRIES = 1 << 22
TORCH_LINKS = 1 << 16


def torch_hop(ptrs, indices, cuts, m_prev, r_prev, m_next, r_next):
    """next = prev folded over every row's entries; m_*: int32 [n, n_perm] in signed order, r_*: uint8 [n, m_reg]"""
    m_next.copy_(m_prev)
    r_next.copy_(r_prev)
    n = ptrs.numel() - 1
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        e0, e1 = int(ptrs[r0]), int(ptrs[r1])
        if e1 == e0:
            continue
        row = torch.repeat_interleave(torch.arange(r0, r1, device=ptrs.device), ptrs[r0 + 1:r1 + 1] - ptrs[r0:r1], output_size=e1 - e0)
        src = indices[e0:e1]
        m_next.scatter_reduce_(0, row[:, None].expand(-1, m_prev.shape[1]), m_prev[src], "amin")
        r_next.scatter_reduce_(0, row[:, None].expand(-1, r_prev.shape[1]), r_prev[src], "amax")
    assert n == m_next.shape[0]


def row_cuts(ptrs):
    """cuts of the rows so that a chunk holds at most TORCH_ENTRIES entries (a longer row is a chunk of its own); found once"""
    p = ptrs.cpu()
    cuts = [0]
    while cuts[-1] < p.numel() - 1:
        nxt = int(torch.searchsorted(p, p[cuts[-1]] + TORCH_ENTRIES, right=True)) - 1
        cuts.append(min(max(nxt, cuts[-1] + 1), p.numel() - 1))
    return cuts


def torch_links(sketch, u, v):
    """-> (match, usum, uzero, nsum, nzero) by gathers and reductions on [L, h, h, W]"""
    outs = []
    for a in range(0, u.numel(), TORCH_LINKS):
        ru, rv = sketch[1:, u[a:a + TORCH_LINKS]].transpose(0, 1), sketch[1:, v[a:a + TORCH_LINKS]].transpose(0, 1)   # [L, h, W]
        match = (ru[:, :, None, :NP] == rv[:, None, :, :NP]).sum(-1, dtype=torch.int32)
        bu, bv = ru[:, :, NP:].contiguous().view(torch.uint8), rv[:, :, NP:].contiguous().view(torch.uint8)      # [L, h, m_reg]
        both = torch.maximum(bu[:, :, None], bv[:, None, :])

        def stats(r):
            r = r.to(torch.int64)
            return torch.bitwise_left_shift(torch.ones_like(r), 33 - r).sum(-1), (r == 0).sum(-1, dtype=torch.int32)
        usum, uzero = stats(both)
        nsum, nzero = stats(torch.stack([bu, bv], 1))
        outs.append((match, usum, uzero, nsum, nzero))
    return [torch.cat(parts) for parts in zip(*outs)]


def main():
    from tch_geometric import _cabi, _cabi_sketch as ops
    dev = torch.device("cuda:0")
    n = 1 << SCALE
    row, col = _cabi.rmat_edges(SCALE, n * 16, 0x5EED0000 + SCALE, dev)
    ptrs, indices, _ = _cabi.coo_to_csx(row, col, n, n, True)
    del row, col
    graph = _cabi.graph_view(ptrs, indices, indices32=indices.to(torch.int32), ptrs32=ptrs.to(torch.int32))
    deg = ptrs[1:] - ptrs[:-1]
    E = indices.numel()
    base = ops.Sketch(H, NP, P, 7, ops.FORM_WAVE)
    W = base.row_words
    sketch, status = ops.sketch_build(graph, base)
    assert int(status.item()) == 0
    res = {"config": "RMAT-%d CSC, %d entries, longest row %d, %d rows above %d entries, %d above %d; n_perm %d, p %d, h %d, "
                     "row %d bytes; %d random links; u32 shadows; %d interleaved rounds"
                     % (SCALE, E, int(deg.max()), int((deg > ops.SKETCH_WAVE_MAX).sum()), ops.SKETCH_WAVE_MAX,
                        int((deg > ops.SKETCH_GROUP_MAX).sum()), ops.SKETCH_GROUP_MAX, NP, P, H, W * 4, LINKS, bf.ROUNDS),
           "constants": {"TG_SKETCH_WAVE_MAX": ops.SKETCH_WAVE_MAX, "TG_SKETCH_GROUP_MAX": ops.SKETCH_GROUP_MAX,
                         "TG_SKETCH_SPLIT_SEG": ops.SKETCH_SPLIT_SEG}, "hbm_peak_bytes_per_s": bf.ROOF}

    # ---- a hop ------------------------------------------------------------------------------------------------------------
    forms = [("wave", dict(form=ops.FORM_WAVE)), ("group", dict(form=ops.FORM_GROUP)), ("split", dict(form=ops.FORM_SPLIT)),
             ("auto", dict(form=ops.FORM_AUTO))]
    forms += [("auto_wave_max_%d" % t, dict(form=ops.FORM_AUTO, wave_max=t)) for t in (64, 1024)]
    forms += [("auto_group_max_%d" % t, dict(form=ops.FORM_AUTO, group_max=t)) for t in (1024, 16384)]
    forms += [("auto_split_seg_512", dict(form=ops.FORM_AUTO, split_seg=512))]
    prev, want, scratch = sketch[0], sketch[1], torch.empty_like(sketch[1])
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    runs = {}
    for key, kw in forms:
        sizes = ops.Sketch(H, NP, P, 7, **kw)
        ws = ops.sketch_propagate(graph, sizes, prev, scratch, st, None)
        assert torch.equal(scratch, want) and int(st.item()) == 0, key                 # equal words in every form
        scratch.zero_()
        runs[key] = lambda sizes=sizes, ws=ws: bf.timed(lambda: ops.sketch_propagate(graph, sizes, prev, scratch, st, ws))
    flip = torch.tensor(-2 ** 31, dtype=torch.int32, device=dev)
    m_prev, r_prev = prev[:, :NP] ^ flip, prev[:, NP:].contiguous().view(torch.uint8)
    m_next, r_next = torch.empty_like(m_prev), torch.empty_like(r_prev)
    cuts = row_cuts(ptrs)
    torch_hop(ptrs, indices, cuts, m_prev, r_prev, m_next, r_next)
    assert torch.equal(m_next ^ flip, want[:, :NP]) and torch.equal(r_next.view(torch.int32), want[:, NP:])

    def composition():
        ms = bf.timed(lambda: torch_hop(ptrs, indices, cuts, m_prev, r_prev, m_next, r_next), warm=0, reps=1)
        print("torch hop: %.1f ms" % ms, file=sys.stderr, flush=True)
        return ms
    runs["torch_scatter_reduce"] = composition
    part = bf.interleaved(runs)
    for s in part.values():
        sec = s["ms_median_of_medians"] * 1e-3
        s["entries_per_s"], s["gathered_bytes_per_s"] = round(E / sec, 0), round(E * W * 4 / sec, 0)
        s["of_hbm_peak"] = round(s["gathered_bytes_per_s"] / bf.ROOF, 4)
    part.update({"entries": E, "gathered_bytes": E * W * 4, "torch_chunks": len(cuts) - 1,
                 "torch_over_auto": round(part["torch_scatter_reduce"]["ms_median_of_medians"] / part["auto"]["ms_median_of_medians"], 3)})
    res["hop"] = part
    print(json.dumps({"hop": part}), file=sys.stderr, flush=True)
    del m_prev, r_prev, m_next, r_next, scratch

    # ---- links ------------------------------------------------------------------------------------------------------------
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    u, v = torch.randint(0, n, (2, LINKS), device=dev, generator=gen)
    u, v = u.contiguous(), v.contiguous()
    out = ops.sketch_links(base, sketch, u, v)
    for name, t in zip(ops.LINK_OUTPUTS, torch_links(sketch, u, v)):
        assert torch.equal(out[name], t), name
    runs = {"kernel": lambda: bf.timed(lambda: ops.sketch_links(base, sketch, u, v, out=out, status=out["status"])),
            "torch_gathers": lambda: bf.timed(lambda: torch_links(sketch, u, v), warm=1, reps=3)}
    part = bf.interleaved(runs)
    for s in part.values():
        sec = s["ms_median_of_medians"] * 1e-3
        s["links_per_s"], s["row_bytes_per_s"] = round(LINKS / sec, 0), round(LINKS * 2 * H * W * 4 / sec, 0)
    part.update({"links": LINKS, "row_bytes": LINKS * 2 * H * W * 4,
                 "torch_over_kernel": round(part["torch_gathers"]["ms_median_of_medians"] / part["kernel"]["ms_median_of_medians"], 3)})
    res["links"] = part
    print(json.dumps(res))


if __name__ == "__main__":
    main()
