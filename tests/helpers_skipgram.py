"""The skip-gram batch rule of tg_rw_skipgram (include/tchgeo.h) restated in NumPy and Python integers."""
import numpy as np

import orc

TAG_RW_NEG = 12


def windows(rows, C):
    """PyG's cat([rw[:, j:j + C] for j in range(nw)], 0) for rows [n, L]: [nw * n, C], nw = L - C + 1."""
    rows = np.asarray(rows)
    L = rows.shape[1]
    return np.concatenate([rows[:, j:j + C] for j in range(L - C + 1)], axis=0)


def negatives(seed, call_id, seeds, R, K, L, n_nodes):
    """The negative rows x [U, L] of one mini-batch, U = R * K * B: x[u][0] = seeds[u mod B]; x[u][m] = floor(a * n_nodes /
    2^64), a = the low 64 bits of the draw (seed, call_id, TAG_RW_NEG, id = u, d0 = m, d1 = 0)."""
    seeds = np.asarray(seeds, dtype=np.int64)
    B = seeds.size
    U = R * K * B
    x = np.empty((U, L), dtype=np.int64)
    for u in range(U):
        x[u, 0] = seeds[u % B]
        for m in range(1, L):
            w = orc.philox_named_draw(seed, call_id, TAG_RW_NEG, u, m, 0)
            a = int(w[0]) | (int(w[1]) << 32)
            x[u, m] = (a * int(n_nodes)) >> 64
    return x
