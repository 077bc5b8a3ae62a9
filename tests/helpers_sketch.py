"""The rule of include/tchgeo_sketch.h restated in NumPy uint32 / uint64 over Python loops, and the exact balls as Python
sets; imports nothing of the library."""
import numpy as np

from helpers_labor import philox4x32_10

TAG_MINHASH, TAG_HLL = 0x736B6D68, 0x736B686C


def init(n, n_perm, hll_p, seed):
    """hop 0 -> (M uint32 [n, n_perm], R uint8 [n, m_reg])"""
    x = np.arange(n, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    M = np.zeros((n, n_perm), dtype=np.uint32)
    for j in range(n_perm // 4):
        for i, w in enumerate(philox4x32_10(x, x >> np.uint64(32), j, TAG_MINHASH, k0, k1)):
            M[:, 4 * j + i] = w
    w0, w1, _, _ = philox4x32_10(x, x >> np.uint64(32), 0, TAG_HLL, k0, k1)
    R = np.zeros((n, 1 << hll_p), dtype=np.uint8)
    for v in range(n):
        R[v, int(w0[v]) & ((1 << hll_p) - 1)] = 1 + (32 - int(w1[v]).bit_length())     # clz32(0) = 32
    return M, R


def propagate(ptrs, indices, M, R):
    """a hop over the rows of (ptrs, indices) -> (M', R', status)"""
    n, status = M.shape[0], 0
    M2, R2 = M.copy(), R.copy()
    for x in range(n):
        for y in indices[int(ptrs[x]):int(ptrs[x + 1])]:
            if 0 <= y < n:
                M2[x], R2[x] = np.minimum(M2[x], M[y]), np.maximum(R2[x], R[y])
            else:
                status |= 2
    return M2, R2, status


def pack(M, R):
    """the row layout: the MinHash words, then the registers one byte each, little end first -> uint32 [n, W]"""
    return np.concatenate([M, np.ascontiguousarray(R).view("<u4")], axis=1)


def registers(r):
    """-> (sum of 2^(33 - r[j]), the number of zero registers) as Python ints"""
    return sum(1 << (33 - int(b)) for b in r), int((r == 0).sum())


def links(hops, src, dst):
    """hops = [(M_l, R_l) for l in 0..h] -> dict(match, usum, uzero, nsum, nzero, status) over the slots"""
    h, n, m = len(hops) - 1, hops[0][0].shape[0], len(src)
    out = dict(match=np.zeros((m, h, h), np.int32), usum=np.zeros((m, h, h), np.uint64), uzero=np.zeros((m, h, h), np.int32),
               nsum=np.zeros((m, 2, h), np.uint64), nzero=np.zeros((m, 2, h), np.int32), status=0)
    for i, (u, v) in enumerate(zip(src, dst)):
        if not (0 <= u < n and 0 <= v < n):
            out["status"] |= 2
            continue
        for a in range(1, h + 1):
            for s, x in enumerate((u, v)):
                out["nsum"][i, s, a - 1], out["nzero"][i, s, a - 1] = registers(hops[a][1][x])
            for b in range(1, h + 1):
                out["match"][i, a - 1, b - 1] = int((hops[a][0][u] == hops[b][0][v]).sum())
                out["usum"][i, a - 1, b - 1], out["uzero"][i, a - 1, b - 1] = registers(np.maximum(hops[a][1][u], hops[b][1][v]))
    return out


def balls(ptrs, indices, h):
    """-> [N_0, .., N_h], N_l[x] the set of vertices within l hops of x along the rows"""
    n = len(ptrs) - 1
    out = [[{x} for x in range(n)]]
    for _ in range(h):
        prev = out[-1]
        out.append([set(prev[x]).union(*(prev[y] for y in indices[int(ptrs[x]):int(ptrs[x + 1])] if 0 <= y < n))
                    for x in range(n)])
    return out


def card(S, Z, m_reg):
    """the HyperLogLog estimate in float64"""
    S, Z = np.asarray(S, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    E = 0.7213 / (1 + 1.079 / m_reg) * m_reg * m_reg / (S / 2.0 ** 33)
    return np.where((E <= 2.5 * m_reg) & (Z > 0), m_reg * np.log(m_reg / np.maximum(Z, 1.0)), E)
