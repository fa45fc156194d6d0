"""NumPy restatement of the exchange on the log tree count (best-swap local search), written from the maths (for the tests; there
is no such solver anywhere else to port).  Built on the helpers of tests/esp_restatement.py and tests/esp_relax_restatement.py.

Node 0 pinned; S the selection; M = L_red(fixed) + sum_{e in S} w_e a_e a_e^T; Sigma = M^-1; r_ab = a_a^T Sigma a_b; s_e = w_e r_ee.
For e in S, f not in S:  Delta(e, f) = det(M - w_e a_e a_e^T + w_f a_f a_f^T) / det M = (1 - s_e)(1 + s_f) + w_e w_f r_ef^2.
A round takes the largest Delta (ties: lowest e, then lowest f) and stops when Delta - 1 <= min_gain.

Two implementations of the loop:
  * from_scratch: inv(M(S)) every round, Delta for all pairs by the formula;
  * incremental: Sigma0 = inv(L_red), the selection loaded as rank-1 updates in ascending index order, then per swap the
    removal (c = -w_e / (1 - s_e)) and the insertion (c = w_f / (1 + s_f')) as rank-1 updates of Sigma, the scores and the rows
    T = (Sigma a_e)^T of the selected edges, in the device's order; ratio = (1 - s_e)(1 + s_f').
and a brute force best_swap(g, sel) with the top two Delta and their pairs.
"""
import numpy as np

import esp_relax_restatement as X
import esp_restatement as R


def indicator(m, sel):
    x = np.zeros(m)
    x[np.asarray(sel, dtype=np.int64)] = 1.0
    return x


def naive_start(g, k):
    """The k heaviest candidates (ties: lowest index) -- NaiveGreedy's selection on weights without ties."""
    cw = np.asarray(g[6])
    return np.sort(np.lexsort((np.arange(len(cw)), -cw))[:k])


def greedy_start(g, k):
    return np.sort(R.greedy(*g, k)[0])


def columns(g, Sig):
    """Sigma a_e for every candidate as the columns of an (n' + 1) x m array; row n' (index -1: node 0) is 0."""
    u, v = np.asarray(g[4]) - 1, np.asarray(g[5]) - 1
    Sp = np.pad(Sig, ((0, 1), (0, 1)))
    return Sp[:, u] - Sp[:, v]


def delta_matrix(g, Sig, sel, unsel):
    """Delta(e, f) for e in sel (rows) and f in unsel (columns), and the scores s."""
    u, v = np.asarray(g[4]) - 1, np.asarray(g[5]) - 1
    w = np.asarray(g[6], dtype=np.float64)
    Z = columns(g, Sig)
    s = w * (Z[u, np.arange(len(w))] - Z[v, np.arange(len(w))])
    Zs = Z[:, sel]                                           # (n' + 1) x K
    r = Zs[u[unsel]].T - Zs[v[unsel]].T                      # K x (m - K): r_ef
    D = (1.0 - s[sel])[:, None] * (1.0 + s[unsel])[None, :] + (w[sel][:, None] * w[unsel][None, :]) * r * r
    return D, s


def top_two(D, sel, unsel):
    """((Delta, e, f) of the winner -- ties to the lowest e, then the lowest f --, (Delta, e, f) of the runner-up or None)."""
    flat = D.ravel()                                         # rows ascending in e, columns ascending in f: argmax = the tie rule
    a = int(np.argmax(flat))
    first = (float(flat[a]), int(sel[a // D.shape[1]]), int(unsel[a % D.shape[1]]))
    if flat.size < 2:
        return first, None
    rest = flat.copy()
    rest[a] = -np.inf
    b = int(np.argmax(rest))
    return first, (float(rest[b]), int(sel[b // D.shape[1]]), int(unsel[b % D.shape[1]]))


def best_swap(g, sel):
    """Brute force on inv(M(sel)): the top two Delta with their pairs."""
    m = len(g[6])
    sel = np.sort(np.asarray(sel, dtype=np.int64))
    unsel = np.setdiff1d(np.arange(m), sel)
    Sig = np.linalg.inv(X.M_of(g, indicator(m, sel)))
    D, _ = delta_matrix(g, Sig, sel, unsel)
    return top_two(D, sel, unsel)


def near_best(g, sel, rel):
    """Every pair (e, f) whose Delta lies within `rel` (relative) of the best one, the winner included."""
    m = len(g[6])
    sel = np.sort(np.asarray(sel, dtype=np.int64))
    unsel = np.setdiff1d(np.arange(m), sel)
    D, _ = delta_matrix(g, np.linalg.inv(X.M_of(g, indicator(m, sel))), sel, unsel)
    i, j = np.nonzero(D >= D.max() * (1.0 - rel))
    return [(int(sel[a]), int(unsel[b])) for a, b in zip(i, j)]


def separation(first, second):
    """Relative distance of the best and the second-best Delta (inf when there is one pair only)."""
    return np.inf if second is None else (first[0] - second[0]) / abs(first[0])


def from_scratch(g, sel0, max_swaps, min_gain=1e-9):
    """dict(out, in, ratios (the winners' Delta), separations (one per round, the stopping round included), selection, converged)."""
    sel = np.sort(np.asarray(sel0, dtype=np.int64))
    out = dict(out=[], ratios=[], separations=[], converged=0)
    out["in"] = []
    for _ in range(max_swaps):
        first, second = best_swap(g, sel)
        out["separations"].append(separation(first, second))
        if first[0] - 1.0 <= min_gain:
            out["converged"] = 1
            break
        out["out"].append(first[1]); out["in"].append(first[2]); out["ratios"].append(first[0])
        sel = np.sort(np.append(sel[sel != first[1]], first[2]))
    out["selection"] = sel
    return out


def incremental(g, sel0, max_swaps, min_gain=1e-9):
    """The same loop by rank-1 updates in the device's order.  dict as from_scratch plus `resistances` (the scores s of all
    candidates at the end); ratios = (1 - s_e)(1 + s_f')."""
    n, fi, fj, fw, ci, cj, cw = g
    u, v = np.asarray(ci) - 1, np.asarray(cj) - 1
    w = np.asarray(cw, dtype=np.float64)
    m = len(w)
    Sig, beta = R.initial_sigma(n, fi, fj, fw)
    assert beta == 0.0
    Sp = np.pad(Sig, ((0, 1), (0, 1)))                       # index -1 (node 0): a zero row and column
    s = R.scores(Sig, ci, cj, cw)
    rows = [int(e) for e in np.sort(np.asarray(sel0, dtype=np.int64))]
    in_sel = np.zeros(m, dtype=bool)

    def step(e, c_of):
        z = Sp[u[e]] - Sp[v[e]]
        c = c_of(s[e])
        Sp[:] -= c * np.outer(z, z)
        s[:] -= w * c * (z[u] - z[v]) ** 2
        return c, z

    for e in rows:
        step(e, lambda se, e=e: w[e] / (1.0 + se))
        in_sel[e] = True
    T = np.array([Sp[u[e]] - Sp[v[e]] for e in rows])
    out = dict(out=[], ratios=[], separations=[], converged=0)
    out["in"] = []
    for _ in range(max_swaps):
        sel = np.array(rows)
        order = np.argsort(sel)
        unsel = np.flatnonzero(~in_sel)
        Ts = T[order]
        r = Ts[:, u[unsel]] - Ts[:, v[unsel]]
        D = (1.0 - s[sel[order]])[:, None] * (1.0 + s[unsel])[None, :] + (w[sel[order]][:, None] * w[unsel][None, :]) * r * r
        first, second = top_two(D, sel[order], unsel)
        out["separations"].append(separation(first, second))
        if first[0] - 1.0 <= min_gain:
            out["converged"] = 1
            break
        _, e, f = first
        row = rows.index(e)
        ratio = 1.0 - s[e]
        c, z = step(e, lambda se: -w[e] / (1.0 - se))
        T -= c * np.outer(z[u[sel]] - z[v[sel]], z)
        in_sel[e] = False
        ratio *= 1.0 + s[f]
        den = 1.0 + s[f]
        c, z = step(f, lambda sf: w[f] / (1.0 + sf))
        T -= c * np.outer(z[u[sel]] - z[v[sel]], z)
        T[row] = z / den
        rows[row] = f
        in_sel[f] = True
        out["out"].append(e); out["in"].append(f); out["ratios"].append(ratio)
    out["selection"] = np.sort(np.array(rows))
    out["resistances"] = s.copy()
    return out


def log_ratio_check(g, sel, e, f):
    """(log det M' - log det M by the dense route, tolerance): the swap (e out, f in) from the selection `sel`, and what fp64
    allows for that difference -- the sum of esp_relax_restatement.F_tolerance at both selections (each 10 x the disagreement
    of dense LU and SuperLU, floored at 1e-13 |logdet|)."""
    m = len(g[6])
    x0 = indicator(m, sel)
    x1 = x0.copy()
    x1[e] = 0.0
    x1[f] = 1.0
    t0, _, l0 = X.F_tolerance(g, x0)
    t1, _, l1 = X.F_tolerance(g, x1)
    return l1 - l0, t0 + t1


# ---- graphs of the device tests ----
def twins(n=40, pairs=30, seed=8):
    """A random connected fixed graph with every candidate listed twice with equal weight: exact ties in every round."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    fi = perm[1:]
    fj = np.array([perm[rng.integers(0, k)] for k in range(1, n)])
    fw = rng.uniform(0.5, 2.0, n - 1)
    a = rng.integers(0, n, pairs)
    b = (a + rng.integers(1, n, pairs)) % n
    w = rng.uniform(0.5, 2.0, pairs)
    return n, fi, fj, fw, np.repeat(a, 2), np.repeat(b, 2), np.repeat(w, 2)


def awkward(n, m=301, seed=12):
    """n - 1 = 64 or 65 (ld = 64 or 128), m no multiple of 256, candidates touching node 0, candidate 5 a self-loop."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 3)])
    fj = np.concatenate([[perm[rng.integers(0, k)] for k in range(1, n)], rng.integers(0, n, n // 3)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = rng.integers(0, n, m)
    cj = (ci + rng.integers(1, n, m)) % n
    ci[:7:2] = 0
    cj[5] = ci[5]
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, m)
