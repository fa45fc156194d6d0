"""NumPy restatement of the relaxation of GreedyESP's problem, written from the maths (for the tests; there is no such solver
anywhere else to port).  Built on the helpers of tests/esp_restatement.py.

Node 0 pinned.  M(x) = L_red(fixed) + beta I + sum_e x_e w_e a_e a_e^T;  F(x) = logdet M(x) - logdet M(0);
grad_e = w_e a_e^T M(x)^-1 a_e.  LP vertex over {0 <= s <= 1, sum s <= k} of a non-negative gradient: ones on the k largest
entries, ties at the k-th value to the lowest indices.  Frank-Wolfe: step 2 / (2 + t), dual value F + g.(s - x), running
minimum; stop when |g|_2 < grad_tol or (upper - F) < gap_tol |F| (the iterate is then not moved), or after max_iters.
"""
import networkx as nx
import numpy as np

import esp_restatement as R


# ---- the test graphs (n, fi, fj, fw, ci, cj, cw) ----
def chain_er(n, p, seed):
    """Chain-fixed random graph: links (i, i+1) and ER candidates off the chain, weights uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < p
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def petersen():
    G = nx.petersen_graph()
    T = nx.minimum_spanning_tree(G)
    rng = np.random.default_rng(2)
    f = [(a, b, float(rng.uniform(0.5, 2.0))) for a, b in T.edges]
    c = [(a, b, float(rng.uniform(0.5, 2.0))) for a, b in nx.difference(G, T).edges]
    return (10, np.array([e[0] for e in f]), np.array([e[1] for e in f]), np.array([e[2] for e in f]),
            np.array([e[0] for e in c]), np.array([e[1] for e in c]), np.array([e[2] for e in c]))


def random_general(n=500, seed=4):
    """Connected, not a chain: a random spanning tree plus extra fixed edges (self-loops and parallel edges among them);
    random candidates, some touching node 0."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, 800), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, 820)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, 820)


def disconnected():
    """Two chains 0..199 and 200..399: no node without a fixed edge -> beta = 1e-4."""
    n, fi, fj, fw, ci, cj, cw = chain_er(400, 0.01, 6)
    keep = fi != 199
    return n, fi[keep], fj[keep], fw[keep], ci, cj, cw


# ---- M, F, grad ----
def M_of(g, x, sparse=False):
    n, fi, fj, fw, ci, cj, cw = g
    beta = R.beta_of(n, fi, fj, fw)
    xw = np.asarray(cw, dtype=np.float64) * np.asarray(x, dtype=np.float64)
    M = R.reduced_laplacian(n, fi, fj, fw, sparse=sparse) + R.reduced_laplacian(n, ci, cj, xw, sparse=sparse)
    if sparse:
        import scipy.sparse as sp
        return (M + beta * sp.identity(n - 1, format="csc")).tocsc()
    return M + beta * np.eye(n - 1)


def logdet_dense(M):
    sign, val = np.linalg.slogdet(M)
    assert sign > 0
    return float(val)


def logdets(g, x):
    """log det M(x) by two independent routes: (dense LAPACK LU, sparse SuperLU)."""
    return logdet_dense(M_of(g, x)), R.logdet_sparse(M_of(g, x, sparse=True))


def F_tolerance(g, x):
    """What fp64 allows for log det M(x), measured: d = the disagreement of the two CPU routes; a blocked elimination without
    pivoting sums in a third order, so it gets 10 max(d, 1e-13 |logdet M(x)|).  Returns (tolerance, d, logdet)."""
    a, b = logdets(g, x)
    d = abs(a - b)
    return 10.0 * max(d, 1e-13 * abs(a)), d, a


def objective(g, x, logdet0=None):
    if logdet0 is None:
        logdet0 = logdet_dense(M_of(g, np.zeros(len(g[6]))))
    return logdet_dense(M_of(g, x)) - logdet0


def gradient(g, x):
    """w_e a_e^T M(x)^-1 a_e through solves with the incidence columns (not through the inverse's entries)."""
    n, _, _, _, ci, cj, cw = g
    m = len(cw)
    A = np.zeros((n, m))
    ar = np.arange(m)
    np.add.at(A, (np.asarray(ci), ar), 1.0)
    np.add.at(A, (np.asarray(cj), ar), -1.0)
    A = A[1:]
    Z = np.linalg.solve(M_of(g, x), A)
    return np.asarray(cw) * np.einsum("ij,ij->j", A, Z)


def problem(g, logdet0=None):
    if logdet0 is None:
        logdet0 = logdet_dense(M_of(g, np.zeros(len(g[6]))))
    return lambda x: (objective(g, x, logdet0), gradient(g, x))


# ---- LP vertex ----
def lp_vertex(grad, k):
    grad = np.asarray(grad)
    order = np.lexsort((np.arange(len(grad)), -grad))       # value descending, then index ascending
    s = np.zeros(len(grad))
    s[order[:k]] = 1.0
    return s


def lp_margin(grad, k):
    """(g_(k) - g_(k+1)) / max g: how far the k-th and the (k+1)-th largest entries are apart."""
    s = np.sort(np.asarray(grad))[::-1]
    return np.inf if k >= len(s) else (s[k - 1] - s[k]) / s[0]


# ---- the loop ----
def frank_wolfe(g, k, x0, max_iters=20, gap_tol=1e-4, grad_tol=1e-8):
    """dict: iterates (the x every evaluation was made at), F, grad, vertex, dual per iteration; x (the final iterate), upper."""
    prob = problem(g)
    x = np.array(x0, dtype=np.float64)
    out = dict(iterates=[], F=[], grad=[], vertex=[], dual=[], gnorm=[], margin=[])
    upper = np.inf
    for t in range(max_iters):
        F, gr = prob(x)
        s = lp_vertex(gr, k)
        dual = F + gr @ (s - x)
        upper = min(upper, dual)
        out["iterates"].append(x.copy()); out["F"].append(F); out["grad"].append(gr); out["vertex"].append(s)
        out["dual"].append(dual); out["gnorm"].append(float(np.linalg.norm(gr))); out["margin"].append(lp_margin(gr, k))
        if np.linalg.norm(gr) < grad_tol:
            break
        if (upper - F) < gap_tol * abs(F):
            break
        x = x + (2.0 / (t + 2.0)) * (s - x)
    out["x"] = x
    out["upper"] = upper
    return out
