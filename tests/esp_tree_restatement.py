"""NumPy restatement of GreedyESP's matrix-free route for any connected fixed graph, written from the formulas (for the tests; not a
port of any implementation, and free of lowest-common-ancestor logic).

Fixed edges: parallel edges summed in list order ((a, b) and (b, a) are one link), self-loops dropped.  T = the BFS tree from node
0, neighbours in order of first appearance; the links outside T, in order of first appearance, are the seeds.  With M_T the reduced
Laplacian of T (node 0 pinned), Sigma0 = M_T^-1 and the Sigma0 row difference of an edge e = (u, v) is the solution of
M_T x = a_e:
  * float64: a sparse solve (SuperLU) against M_T;
  * np.longdouble (SuperLU has no extended precision): the same solve by elimination on the tree.  The current through the link
    above node a is f_a = [u in subtree(a)] - [v in subtree(a)], and x_i is the sum of f_a / w_a over the ancestors a of i (i
    included): with preorder intervals, f is two interval tests and x is a running sum of +f_a / w_a at pre[a], -f_a / w_a behind end[a].
Initial scores: w_e times the resistance of the tree path between u and v = the sum of 1 / w_a over the nodes a that have exactly
one of u, v in their subtree.  Then the seeds (forced, c = w / (1 + w (z_u - z_v)), no entry in order / gains) and the picks follow
the history recurrence of tests/esp_free_restatement.py:
    alpha_b = c_b (z_b[u] - z_b[v]),   z = x - sum_b alpha_b z_b,   s_e <- s_e - w_e c (z[u_e] - z[v_e])^2.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu


def plan(n, fi, fj, fw):
    """dict(parent, w (of the link above each node), R, pre, end, order (BFS), seeds = (u, v, w)) by the stated rule."""
    links, at = [], {}
    for a, b, w in zip(np.asarray(fi).tolist(), np.asarray(fj).tolist(), np.asarray(fw, dtype=np.float64).tolist()):
        if a == b:
            continue
        key = (min(a, b), max(a, b))
        if key in at:
            links[at[key]][2] += w
        else:
            at[key] = len(links)
            links.append([a, b, w])
    adj = [[] for _ in range(n)]
    for l, (a, b, _) in enumerate(links):
        adj[a].append(l)
        adj[b].append(l)
    parent = np.full(n, -1, dtype=np.int64)
    wup = np.zeros(n)
    R = np.zeros(n)
    seen = np.zeros(n, dtype=bool)
    intree = np.zeros(len(links), dtype=bool)
    children = [[] for _ in range(n)]
    order, seen[0] = [0], True
    for x in order:                                   # (grows while it is walked: the BFS queue)
        for l in adj[x]:
            a, b, w = links[l]
            y = b if a == x else a
            if seen[y]:
                continue
            seen[y], intree[l], parent[y], wup[y] = True, True, x, w
            R[y] = R[x] + 1.0 / w
            children[x].append(y)
            order.append(y)
    assert len(order) == n, "the fixed graph is not connected"
    pre = np.zeros(n, dtype=np.int64)
    size = np.ones(n, dtype=np.int64)
    for y in reversed(order[1:]):
        size[parent[y]] += size[y]
    stack, cnt = [0], 0
    while stack:
        x = stack.pop()
        pre[x] = cnt
        cnt += 1
        stack.extend(reversed(children[x]))
    seeds = [links[l] for l in range(len(links)) if not intree[l]]
    return dict(parent=parent, w=wup, R=R, pre=pre, end=pre + size - 1, order=np.array(order),
                seeds=(np.array([s[0] for s in seeds], dtype=np.int64), np.array([s[1] for s in seeds], dtype=np.int64),
                       np.array([s[2] for s in seeds], dtype=np.float64)))


def tree_laplacian(n, P):
    """The reduced Laplacian of the spanning tree (sparse, node 0 pinned)."""
    v = np.arange(1, n)
    p, w = P["parent"][1:], P["w"][1:]
    rows = np.concatenate([v, p, v, p])
    cols = np.concatenate([v, p, p, v])
    data = np.concatenate([w, w, -w, -w])
    return sp.coo_matrix((data, (rows, cols)), shape=(n, n)).tocsc()[1:, 1:].tocsc()


class Sigma0:
    """Rows differences and path resistances of Sigma0 = M_T^-1 in `dtype`."""

    def __init__(self, n, P, dtype):
        self.n, self.P, self.dtype = n, P, dtype
        self.pre, self.end = P["pre"], P["end"]
        self.rinv = np.zeros(n, dtype=dtype)
        self.rinv[1:] = dtype(1) / P["w"][1:].astype(dtype)
        self.lu = splu(tree_laplacian(n, P)) if dtype is np.float64 else None

    def row(self, u, v):
        """x with M_T x = a_(u, v), node indexing (x[0] = 0)."""
        n = self.n
        if self.lu is not None:
            a = np.zeros(n)
            a[u] += 1.0
            a[v] -= 1.0
            return np.concatenate([[0.0], self.lu.solve(a[1:])])
        pre, end = self.pre, self.end
        f = ((pre <= pre[u]) & (pre[u] <= end)).astype(self.dtype) - ((pre <= pre[v]) & (pre[v] <= end)).astype(self.dtype)
        g = f * self.rinv                                         # (rinv[0] = 0: no link above the root)
        D = np.zeros(n + 1, dtype=self.dtype)
        np.add.at(D, pre, g)
        np.add.at(D, end + 1, -g)
        return np.cumsum(D[:n], dtype=self.dtype)[pre]

    def path_resistance(self, u, v, chunk=256):
        """Resistance of the tree path between u[e] and v[e] for every e: 1 / w summed over the links that separate them."""
        pre, end = self.pre, self.end
        out = np.zeros(len(u), dtype=self.dtype)
        for c0 in range(0, len(u), chunk):
            pu, pv = pre[u[c0:c0 + chunk], None], pre[v[c0:c0 + chunk], None]
            one = ((pre <= pu) & (pu <= end)) != ((pre <= pv) & (pv <= end))
            out[c0:c0 + chunk] = one.astype(self.dtype) @ self.rinv
        return out


def greedy(n, fi, fj, fw, ci, cj, cw, K, dtype=np.float64, P=None):
    """(order, gains, margins) as esp_free_restatement.greedy, every quantity of the recurrence carried in `dtype`."""
    P = plan(n, fi, fj, fw) if P is None else P
    S0 = Sigma0(n, P, dtype)
    su, sv, sw = P["seeds"]
    r = len(sw)
    u, v = np.asarray(ci), np.asarray(cj)
    cw = np.asarray(cw, dtype=dtype)
    m = len(cw)
    s = cw * S0.path_resistance(u, v)
    sel = np.zeros(m, dtype=bool)
    Z = np.zeros((r + K, n), dtype=dtype)         # the history, node indexing: the r seeds first
    cb = np.zeros(r + K, dtype=dtype)

    def column(j, a, b):
        alpha = cb[:j] * (Z[:j, a] - Z[:j, b])
        return S0.row(a, b).astype(dtype) - alpha @ Z[:j]

    for q in range(r):
        z = column(q, su[q], sv[q])
        w = dtype(sw[q])
        Z[q] = z
        cb[q] = w / (dtype(1) + w * (z[su[q]] - z[sv[q]]))
        s = s - cw * cb[q] * (z[u] - z[v]) ** 2
    order, gains, margins = [], [], []
    for k in range(K):
        masked = np.where(sel, -np.inf, s)
        e = int(np.argmax(masked))
        best = masked[e]
        masked[e] = -np.inf
        second = masked.max() if m - k > 1 else -np.inf
        margins.append(float((best - second) / abs(best)) if np.isfinite(second) and best != 0 else np.inf)
        z = column(r + k, u[e], v[e])
        Z[r + k] = z
        cb[r + k] = cw[e] / (dtype(1) + best)
        s = s - cw * cb[r + k] * (z[u] - z[v]) ** 2
        sel[e] = True
        order.append(e)
        gains.append(float(best))
    return np.array(order), np.array(gains), np.array(margins)


def shallow_case(seed, n=40000, r=200, m=20000):
    """A random recursive tree (node i hangs below a uniformly drawn earlier node: depth O(log n)), r extra fixed edges."""
    rng = np.random.default_rng(seed)
    ti = np.arange(1, n)
    tj = np.array([rng.integers(0, i) for i in range(1, n)])
    return _with_extras(rng, n, ti, tj, r, m)


def deep_case(seed, n=40000, r=200, m=20000):
    """A chain of n / 2 nodes with random branches hanging off it: every later node below a uniformly drawn earlier node."""
    rng = np.random.default_rng(seed)
    h = n // 2
    ti = np.arange(1, n)
    tj = np.concatenate([np.arange(h - 1), [rng.integers(0, i) for i in range(h, n)]])
    return _with_extras(rng, n, ti, tj, r, m)


def _with_extras(rng, n, ti, tj, r, m):
    perm = rng.permutation(n)                     # (node numbers carry no structure; node 0 is anywhere in the tree)
    ti, tj = perm[ti], perm[tj]
    tree = set(zip(np.minimum(ti, tj).tolist(), np.maximum(ti, tj).tolist()))
    xi, xj = [], []
    while len(xi) < r:                            # r distinct links outside the tree
        a, b = (int(t) for t in rng.integers(0, n, 2))
        key = (min(a, b), max(a, b))
        if a != b and key not in tree:
            tree.add(key)
            xi.append(a)
            xj.append(b)
    fi, fj = np.concatenate([ti, xi]), np.concatenate([tj, xj])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = rng.integers(0, n, m)
    cj = rng.integers(0, n, m)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, m)
