"""NumPy restatement of the relaxation of GreedyESP's problem in edge space (mac_amd/csrc/esp_relax_edge.h), written from the
maths, for chain-fixed graphs.  Graphs are the tuples (n, fi, fj, fw, ci, cj, cw) of tests/esp_relax_restatement.py.

The fixed edges are the chain (t, t+1) with summed parallel weights c_t; R[v] = sum_{t < v} 1 / c_t.  Candidate e has the ends
lo_e <= hi_e and the weight w_e.  G_ef = max(0, R[min(hi_e, hi_f)] - R[max(lo_e, lo_f)]);  D = diag(w_e x_e);  N(x) = I + G D;
F(x) = logdet N(x);  grad_e = w_e [N(x)^-1 G]_ee.
"""
import numpy as np


def chain_resistances(g):
    """R[v], v = 0..n-1: the resistance from node 0 along the chain.  Asserts the fixed edges are exactly the connected chain."""
    n, fi, fj, fw = g[0], np.asarray(g[1]), np.asarray(g[2]), np.asarray(g[3], dtype=np.float64)
    a, b = np.minimum(fi, fj), np.maximum(fi, fj)
    assert np.all(b == a + 1), "the fixed edges are not chain links (t, t+1)"
    c = np.zeros(n - 1)
    np.add.at(c, a, fw)
    assert np.all(c > 0.0), "a hop of the chain has no link (or no positive weight)"
    return np.concatenate([[0.0], np.cumsum(1.0 / c)])


def G_of(g):
    R = chain_resistances(g)
    ci, cj = np.asarray(g[4]), np.asarray(g[5])
    lo, hi = np.minimum(ci, cj), np.maximum(ci, cj)
    return np.maximum(0.0, R[np.minimum.outer(hi, hi)] - R[np.maximum.outer(lo, lo)])


def N_of(g, x):
    d = np.asarray(g[6], dtype=np.float64) * np.asarray(x, dtype=np.float64)
    return np.eye(len(d)) + G_of(g) * d[None, :]


def objective(g, x):
    if len(g[6]) == 0:
        return 0.0
    sign, val = np.linalg.slogdet(N_of(g, x))
    assert sign > 0
    return float(val)


def gradient(g, x):
    """w_e [N^-1 G]_ee by LAPACK: one solve with G as the right-hand sides."""
    return np.asarray(g[6], dtype=np.float64) * np.diag(np.linalg.solve(N_of(g, x), G_of(g)))


# ---- inputs shared by the host and the device tests ----
def awkward12():
    """A 12-node chain with two parallel fixed links on one hop and one reversed fixed edge; candidates (5, 2) and (2, 5) twice
    each, one candidate touching node 0, one self-loop, and a few ordinary ones."""
    rng = np.random.default_rng(12)
    fi = np.concatenate([np.arange(11), [4]]); fj = np.concatenate([np.arange(1, 12), [5]])
    fi[7], fj[7] = fj[7], fi[7]                                    # the link 7-8 given as (8, 7)
    fw = rng.uniform(0.5, 2.0, 12)
    ci = np.array([5, 2, 5, 2, 0, 6, 1, 3, 8, 0])
    cj = np.array([2, 5, 2, 5, 7, 6, 11, 9, 10, 11])
    return 12, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, len(ci))


def wild_x(m, seed=29):
    """30 % exact zeros, the rest 10^U(-14, 0)."""
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(-14.0, 0.0, m)
    x[rng.random(m) < 0.3] = 0.0
    return x


def vertex_x(m, seed=31):
    """A 0/1 vertex: a third of the entries, chosen at random, are 1."""
    x = np.zeros(m)
    x[np.random.default_rng(seed).choice(m, max(1, m // 3), replace=False)] = 1.0
    return x
