"""The rule of include/tchgeo_ppr.h (tg_ppr_topk: forward push in units of 2^-31, synchronous rounds, top-k) restated as a
dict loop over rounds in Python ints; the reference of tests/test_ppr_cpu.py, test_gpu_ppr.py and test_gpu_ppr_loader.py.
Imports nothing."""

U = 1 << 31
W = 1 << 32


def push(ptrs, indices, seed, alpha_q, eps_q, max_rounds, node_cap):
    """-> dict(p, r, touched, rounds, activations, residual, mass) of one slot; dict(refused=1) when a round leaves more
    than node_cap touched vertices, dict(refused=2) for a seed outside [0, len(ptrs) - 1)"""
    if not 0 <= seed < len(ptrs) - 1:
        return dict(refused=2)
    p, r = {seed: 0}, {seed: U}
    keep = W - alpha_q
    rounds = activations = 0
    for _ in range(max_rounds):
        incoming, active = {}, 0
        for v, rv in list(r.items()):                       # the residuals as they stood when the round began
            b, e = int(ptrs[v]), int(ptrs[v + 1])
            d = e - b
            if d == 0:
                if rv >= 1:
                    p[v] += rv
                    r[v] = 0
                    active += 1
                continue
            q = (rv * keep // W) // d
            if rv >= eps_q * d and q >= 1:
                a = alpha_q * q * d // keep
                p[v] += a
                r[v] = rv - a - q * d
                active += 1
                for t in indices[b:e]:
                    incoming[int(t)] = incoming.get(int(t), 0) + q
        for t, x in incoming.items():
            p.setdefault(t, 0)
            r[t] = r.get(t, 0) + x
        if len(p) > node_cap:
            return dict(refused=1)
        if not active:
            break
        rounds += 1
        activations += active
    return dict(p=p, r=r, touched=len(p), rounds=rounds, activations=activations, residual=sum(r.values()),
                mass=sum(p.values()))


def top(state, seed, k):
    """-> (nodes, score) of a slot's output row: the seed, then the other vertices with p > 0 by p descending, id ascending"""
    rest = sorted((-pv, v) for v, pv in state["p"].items() if v != seed and pv > 0)[:k - 1]
    return [seed] + [v for _, v in rest], [state["p"][seed]] + [-pv for pv, _ in rest]
