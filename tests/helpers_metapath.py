"""The metapath skip-gram rule of tg_mp_skipgram (include/tchgeo.h) restated in NumPy and Python integers."""
import numpy as np

import orc
from helpers_skipgram import TAG_RW_NEG, windows  # noqa: F401  (windows: the window rule is tg_rw_skipgram's)


def _low64(seed, call_id, tag, id_, d0):
    w = orc.philox_named_draw(seed, call_id, tag, id_, d0, 0)
    return int(w[0]) | (int(w[1]) << 32)


def column_types(step_src, step_dst, L):
    """type index of every column: column 0 has step_src[0], column l + 1 has step_dst[l mod M]"""
    M = len(step_src)
    return [step_src[0]] + [step_dst[l % M] for l in range(L - 1)]


def walks(seed, call_id, csrs, step_src, step_dst, seeds, R, T):
    """Local-id walks [R * B, T + 1] of one mini-batch, -1 behind an ended walk.  csrs[m] = (ptrs, indices) of metapath[m];
    walker w = r * B + i starts at seeds[i]; step l reads row cur of csrs[l mod M] and draws (TAG_RW, id = w, d0 = l, d1 = 0):
    next = indices[b + floor(a * (e - b) / 2^64)]."""
    seeds = np.asarray(seeds, dtype=np.int64)
    M, W = len(csrs), R * seeds.size
    assert len(step_src) == len(step_dst) == M
    out = np.full((W, T + 1), -1, dtype=np.int64)
    for w in range(W):
        cur = int(seeds[w % seeds.size])
        out[w, 0] = cur
        for l in range(T):
            ptrs, idx = csrs[l % M]
            b, e = int(ptrs[cur]), int(ptrs[cur + 1])
            if e <= b:
                break
            cur = int(idx[b + ((_low64(seed, call_id, orc.TAG_RW, w, l) * (e - b)) >> 64)])
            out[w, l + 1] = cur
    return out


def negatives(seed, call_id, step_src, step_dst, seeds, R, K, L, type_count):
    """Local-id negative rows x [U, L], U = R * K * B: x[u][0] = seeds[u mod B]; x[u][m] = floor(a * type_count[type of
    column m] / 2^64), a = the low 64 bits of the draw (TAG_RW_NEG, id = u, d0 = m, d1 = 0)."""
    seeds = np.asarray(seeds, dtype=np.int64)
    U = R * K * seeds.size
    types = column_types(step_src, step_dst, L)
    x = np.empty((U, L), dtype=np.int64)
    for u in range(U):
        x[u, 0] = seeds[u % seeds.size]
        for m in range(1, L):
            x[u, m] = (_low64(seed, call_id, TAG_RW_NEG, u, m) * int(type_count[types[m]])) >> 64
    return x


def finish(rows, col_types, type_start, pad):
    """The output words of local-id rows [n, L]: id + type_start[type of its column], `pad` where the walk had ended."""
    rows = np.asarray(rows, dtype=np.int64)
    start = np.zeros(len(col_types), dtype=np.int64) if type_start is None else \
        np.asarray([type_start[t] for t in col_types], dtype=np.int64)
    return np.where(rows >= 0, rows + start[None, :], np.int64(pad))
