"""NumPy restatement of GreedyESP's history recurrence for chain-fixed graphs, written from the formulas (for the tests; not a
port of any implementation).

Fixed edges: the chain (i, i+1), parallel links summed.  With Rp[a] the resistance from node 0 to node a along the chain (Rp[0] = 0),
Sigma0_ab = Rp[min(a, b)] in node indexing, so no matrix is kept: candidate e = (u, v, w) starts at
s_e = w (Rp[u] + Rp[v] - 2 Rp[min(u, v)]), and pick k (argmax over the unselected, ties: lowest index) gives, from the history of
the earlier picks' z's and c's,
    alpha_b = c_b (z_b[u] - z_b[v]),   z = Rp[min(u, .)] - Rp[min(v, .)] - sum_{b < k} alpha_b z_b,   c = w / (1 + s*),
    s_e <- s_e - w_e c (z[u_e] - z[v_e])^2.
"""
import numpy as np


def chain_resistances(n, fi, fj, fw, dtype=np.float64):
    lo, hi = np.minimum(fi, fj), np.maximum(fi, fj)
    assert np.all(hi == lo + 1), "the fixed edges must be the chain (i, i+1)"
    link = np.zeros(n - 1, dtype=dtype)
    np.add.at(link, lo, np.asarray(fw, dtype=dtype))
    assert np.all(link > 0), "a link of the chain is missing"
    return np.concatenate([np.zeros(1, dtype=dtype), np.cumsum(dtype(1) / link, dtype=dtype)])


def greedy(n, fi, fj, fw, ci, cj, cw, K, dtype=np.float64):
    """(order, gains, margins) as esp_restatement.greedy, every quantity carried in `dtype`; gains are returned as float64."""
    Rp = chain_resistances(n, np.asarray(fi), np.asarray(fj), fw, dtype)
    u, v = np.asarray(ci), np.asarray(cj)
    cw = np.asarray(cw, dtype=dtype)
    m = len(cw)
    s = cw * (Rp[u] + Rp[v] - dtype(2) * Rp[np.minimum(u, v)])
    sel = np.zeros(m, dtype=bool)
    Z = np.zeros((K, n), dtype=dtype)         # the history, node indexing (column 0 stays 0: node 0)
    cb = np.zeros(K, dtype=dtype)
    nodes = np.arange(n)
    order, gains, margins = [], [], []
    for k in range(K):
        masked = np.where(sel, -np.inf, s)
        e = int(np.argmax(masked))
        best = masked[e]
        masked[e] = -np.inf
        second = masked.max() if m - k > 1 else -np.inf
        margins.append(float((best - second) / abs(best)) if np.isfinite(second) and best != 0 else np.inf)
        alpha = cb[:k] * (Z[:k, u[e]] - Z[:k, v[e]])
        z = Rp[np.minimum(u[e], nodes)] - Rp[np.minimum(v[e], nodes)] - alpha @ Z[:k]
        Z[k] = z
        cb[k] = cw[e] / (dtype(1) + best)
        s = s - cw * cb[k] * (z[u] - z[v]) ** 2
        sel[e] = True
        order.append(e)
        gains.append(float(best))
    return np.array(order), np.array(gains), np.array(margins)


def large_case(seed, n=40000, m=20000):
    """The case beyond the dense limit: chain weights, two draws of endpoints and candidate weights, in that order."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1)
    fw = rng.uniform(0.5, 2.0, n - 1)
    ci = rng.integers(0, n, m)
    cj = rng.integers(0, n, m)
    return n, fi, fi + 1, fw, ci, cj, rng.uniform(0.5, 2.0, m)
