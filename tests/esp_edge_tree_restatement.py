"""NumPy restatement of the relaxation of GreedyESP's problem in edge space over a spanning tree
(mac_amd/csrc/esp_relax_edge_tree.h), written from the maths, for any connected fixed graph.  Graphs are the tuples
(n, fi, fj, fw, ci, cj, cw) of tests/esp_relax_restatement.py.

T, its root resistances R (by node) and the seeds (u_s, v_s, w_s) -- the fixed links outside T -- are the plan's
(_lib.host_esp_tree, host only).  M = m + r columns: the candidates, then the seeds.  For columns e, f
    G_ef = (R[lca(u_e, u_f)] + R[lca(v_e, v_f)]) - (R[lca(u_e, v_f)] + R[lca(v_e, u_f)])          (this association)
d = (w x, w_seed);  N(x) = I + G diag(d);  F(x) = logdet N(x) - logdet N(0);  grad_e = w_e [N(x)^-1 G]_ee for e < m.

There is no lifting table here.  Lowest common ancestors come from parent walks: every endpoint's path to the root is written out
by following `parent`, and two nodes' lowest common ancestor is the last entry their root-first paths share (the paths of a tree
agree on a prefix, so where they stop agreeing is found by bisection on the explicit paths).  N, F and the gradient: dense LAPACK.
"""
import functools

import numpy as np

import esp_relax_restatement as X
from mac_amd import _lib


def plan_of(g):
    return _lib.host_esp_tree(g[0], g[1], g[2], g[3])


def lca_walk(parent, a, b):
    """lca(a, b) the plain way: a's ancestors into a set, b walks up until it meets one.  (The small graphs check `lca_pairs` with it.)"""
    seen = set()
    while a >= 0:
        seen.add(int(a)); a = parent[a]
    while int(b) not in seen:
        b = parent[b]
    return int(b)


def root_paths(parent, nodes):
    """(anc, cnt): anc[i, d] = the ancestor of nodes[i] at depth d, root first (-1 beyond cnt[i] = depth of nodes[i] + 1)."""
    parent = np.asarray(parent, dtype=np.int64)
    cur = np.asarray(nodes, dtype=np.int64).copy()
    cols = []
    while np.any(cur >= 0):                                   # all walks side by side, one step of `parent` per round
        cols.append(cur)
        cur = np.where(cur >= 0, parent[np.maximum(cur, 0)], -1)
    up = np.stack(cols, axis=1)                               # leaf first
    cnt = (up >= 0).sum(axis=1)
    idx = cnt[:, None] - 1 - np.arange(up.shape[1])[None, :]
    return np.where(idx >= 0, np.take_along_axis(up, np.maximum(idx, 0), axis=1), -1), cnt


def lca_pairs(parent, nodes):
    """L[i, j] = lca(nodes[i], nodes[j]) as a node id."""
    anc, cnt = root_paths(parent, nodes)
    P = len(nodes)
    A, B = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    lo = np.ones((P, P), dtype=np.int64)                      # the root is shared: at least one common entry
    hi = np.minimum(cnt[A], cnt[B])
    while np.any(lo < hi):
        mid = (lo + hi + 1) // 2
        ok = anc[A, mid - 1] == anc[B, mid - 1]
        lo = np.where(ok, mid, lo)
        hi = np.where(ok, hi, mid - 1)
    return anc[A, lo - 1]


def columns(g, plan=None):
    """(u, v, w_seed): the endpoints of the M = m + r columns (candidates, then seeds in the plan's order) and the seeds' weights."""
    plan = plan or plan_of(g)
    su, sv, sw = plan["seeds"]
    return (np.concatenate([np.asarray(g[4], dtype=np.int64), su.astype(np.int64)]),
            np.concatenate([np.asarray(g[5], dtype=np.int64), sv.astype(np.int64)]), sw)


def G_of(g, plan=None):
    plan = plan or plan_of(g)
    u, v, _ = columns(g, plan)
    nodes = np.unique(np.concatenate([u, v]))
    R = plan["R"][lca_pairs(plan["parent"], nodes)]           # R[lca] for every pair of endpoints
    iu, iv = np.searchsorted(nodes, u), np.searchsorted(nodes, v)
    return (R[np.ix_(iu, iu)] + R[np.ix_(iv, iv)]) - (R[np.ix_(iu, iv)] + R[np.ix_(iv, iu)])


def N_of(g, x, G=None, plan=None):
    plan = plan or plan_of(g)
    G = G_of(g, plan) if G is None else G
    d = np.concatenate([np.asarray(g[6], dtype=np.float64) * np.asarray(x, dtype=np.float64), plan["seeds"][2]])
    return np.eye(len(d)) + G * d[None, :]


def _logdet(N):
    if N.shape[0] == 0:
        return 0.0
    sign, val = np.linalg.slogdet(N)
    assert sign > 0
    return float(val)


def objective(g, x, G=None, plan=None):
    plan = plan or plan_of(g)
    G = G_of(g, plan) if G is None else G
    return _logdet(N_of(g, x, G, plan)) - _logdet(N_of(g, np.zeros(len(g[6])), G, plan))


def gradient(g, x, G=None, plan=None):
    """w_e [N^-1 G]_ee, e < m, by LAPACK: one solve with G as the right-hand sides."""
    plan = plan or plan_of(g)
    G = G_of(g, plan) if G is None else G
    m = len(g[6])
    return np.asarray(g[6], dtype=np.float64) * np.diag(np.linalg.solve(N_of(g, x, G, plan), G))[:m]


def frank_wolfe(g, k, x0, max_iters=20):
    """The loop of esp_relax_restatement.frank_wolfe on this form's F and gradient, stop tests off: dict of the iterates, F, grad,
    vertex, dual and margin per iteration."""
    plan = plan_of(g)
    G = G_of(g, plan)
    x = np.array(x0, dtype=np.float64)
    out = dict(iterates=[], F=[], grad=[], vertex=[], dual=[], margin=[])
    for t in range(max_iters):
        F, gr = objective(g, x, G, plan), gradient(g, x, G, plan)
        s = X.lp_vertex(gr, k)
        out["iterates"].append(x.copy()); out["F"].append(F); out["grad"].append(gr); out["vertex"].append(s)
        out["dual"].append(F + gr @ (s - x)); out["margin"].append(X.lp_margin(gr, k))
        x = x + (2.0 / (t + 2.0)) * (s - x)
    return out


# ---- inputs shared by the host and the device tests ----
def move_closures(g, c):
    """g with its first c candidates moved to the end of the fixed list."""
    n, fi, fj, fw, ci, cj, cw = g
    return (n, np.concatenate([fi, ci[:c]]), np.concatenate([fj, cj[:c]]), np.concatenate([fw, cw[:c]]).astype(np.float64),
            ci[c:], cj[c:], np.asarray(cw[c:], dtype=np.float64))


def random_tree(n, r, m, seed, deep=0):
    """A tree on n shuffled node ids (node 0 stays the root's id) plus r extra fixed links and m random candidates, weights
    U(0.5, 2).  deep = 0: a random recursive tree (shallow).  deep = s: a spine of s nodes with the other n - s nodes hanging off it
    in branches of up to 3 nodes; its extra links join spine nodes 2 or 3 apart, so each shortens the BFS tree by at most 2 levels.
    Candidate 0 touches node 0; the extra links are distinct from the tree's and from each other."""
    rng = np.random.default_rng(seed)
    label = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    par = np.zeros(n, dtype=np.int64)
    for v in range(1, n):
        if deep and v < deep:
            par[v] = v - 1
        elif deep:
            par[v] = v - 1 if (v - deep) % 3 and v - 1 >= deep else rng.integers(0, deep)
        else:
            par[v] = rng.integers(0, v)
    have = {(min(a, b), max(a, b)) for a, b in zip(range(1, n), par[1:].tolist())}
    ea, eb = [], []
    while len(ea) < r:
        a, b = (int(t) for t in rng.integers(0, n, 2))
        if deep:
            a = int(rng.integers(0, deep - 3)); b = a + 2 + int(rng.integers(0, 2))
        if a != b and (min(a, b), max(a, b)) not in have:
            have.add((min(a, b), max(a, b))); ea.append(a); eb.append(b)
    fi = label[np.concatenate([np.arange(1, n), np.array(ea, dtype=np.int64)])]
    fj = label[np.concatenate([par[1:], np.array(eb, dtype=np.int64)])]
    ci, cj = rng.integers(0, n, m), rng.integers(0, n, m)
    if m:
        ci[0] = 0
    return n, fi, fj, rng.uniform(0.5, 2.0, len(fi)), ci, cj, rng.uniform(0.5, 2.0, m)


def tree40():
    """A 40-node random tree plus 6 extra fixed links; ER candidates (p = 0.1) over all pairs."""
    n, fi, fj, fw, _, _, _ = random_tree(40, 6, 0, 40)
    rng = np.random.default_rng(41)
    iu, ju = np.triu_indices(n, 1)
    pick = rng.random(len(iu)) < 0.1
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def star(n=30, hub=3, m=45, seed=3):
    """Every node hangs off `hub` (node 0 is a leaf: the tree rooted at 0 has depth 2); no seeds."""
    rng = np.random.default_rng(seed)
    leaves = np.array([v for v in range(n) if v != hub])
    return n, leaves, np.full(n - 1, hub), rng.uniform(0.5, 2.0, n - 1), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m)


def awkward12():
    """12 nodes.  Fixed: a tree given partly reversed, the link 4-5 twice (once as (5, 4)), and four links more than a tree has, one of
    them twice.  Candidates: (5, 2) and (2, 5) twice each, one at node 0, a self-loop, one equal to a tree link, one equal to a
    seed, and a few ordinary ones."""
    rng = np.random.default_rng(12)
    fi = np.array([0, 1, 2, 2, 4, 5, 6, 4, 8, 9, 9, 5, 3, 11, 7, 10, 11])
    fj = np.array([1, 2, 3, 4, 5, 4, 5, 7, 4, 8, 10, 11, 6, 1, 0, 3, 1])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.array([5, 2, 5, 2, 0, 6, 1, 3, 8, 0, 2, 3])
    cj = np.array([2, 5, 2, 5, 7, 6, 11, 9, 10, 11, 4, 6])
    return 12, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, len(ci))


@functools.lru_cache(maxsize=None)
def intel_fixed50():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2o_intel.npz"))
    return move_closures((int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
                          np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64)), 50)


TEACHER_K_PCT = 0.5


@functools.lru_cache(maxsize=None)
def teacher_run():
    """The 20 restated Frank-Wolfe iterates of intel with 50 closures fixed at K = 50 %, from the k heaviest candidates: the teacher-forcing
    input of the device test (tests/test_esp_edge_tree_gpu.py) and of the host test that checks its margins."""
    g = intel_fixed50()
    m = len(g[6])
    k = int(TEACHER_K_PCT * m)
    x0 = np.zeros(m)
    x0[np.argsort(-g[6], kind="stable")[:k]] = 1.0         
    return k, frank_wolfe(g, k, x0, max_iters=20)
