"""NumPy restatement of GreedyEig's selection rule, written from the maths (for the tests; not a port of any implementation).

L_cur = the Laplacian of the fixed edges plus the picks so far.  Candidate e = (i, j, w) is worth lambda_2(L_cur + w a_e a_e^T)
(a_e = e_i - e_j); its supergradient bound is u_e = lambda_2(L_cur) + w (v_i - v_j)^2 with v the unit Fiedler vector of L_cur
(concavity of lambda_2: u_e >= the value).  A pick scans the unselected candidates in index order; a candidate replaces the
running best (initially 0, nobody) only if it exceeds it by more than 1e-8.

Two ways to the values:
  * brute force: numpy.linalg.eigvalsh of the dense L_cur + w a a^T per candidate;
  * secular: one eigh of L_cur = V diag(d) V^T per pick; the eigenvalues of the rank-one update are the roots of
    1 + w sum_i xi_i^2 / (d_i - mu), xi = V^T a; a is orthogonal to 1, so the zero eigenvalue stays and lambda_2 is the root in
    [d_1, d_2] (interlacing) -- found by bisection on that interval for all candidates at once (no root: xi_1 = 0, the value d_1).
"""
import numpy as np

TIE = 1e-8


def laplacian(n, i, j, w):
    i, j, w = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(w, dtype=np.float64)
    L = np.zeros((n, n))
    keep = i != j
    i, j, w = i[keep], j[keep], w[keep]
    np.add.at(L, (i, i), w)
    np.add.at(L, (j, j), w)
    np.add.at(L, (i, j), -w)
    np.add.at(L, (j, i), -w)
    return L


def norm_inf(L):
    return float(np.abs(L).sum(axis=1).max())


def norm_inf_with(L, ci, cj, cw):
    """||L + w a a^T||_inf per candidate."""
    ci, cj, cw = np.asarray(ci), np.asarray(cj), np.asarray(cw, dtype=np.float64)
    rows = np.abs(L).sum(axis=1)
    add = np.where(ci != cj, 2.0 * cw, 0.0)
    return np.maximum(rows.max(), np.maximum(rows[ci], rows[cj]) + add)


def fiedler(L):
    d, V = np.linalg.eigh(L)
    return float(d[1]), V[:, 1]


def bounds(L, ci, cj, cw):
    lam, v = fiedler(L)
    return lam + np.asarray(cw) * (v[np.asarray(ci)] - v[np.asarray(cj)]) ** 2


def values_brute(L, ci, cj, cw, skip=None):
    out = np.full(len(cw), np.nan)
    for e in range(len(cw)):
        if skip is not None and skip[e]:
            continue
        Le = L.copy()
        a, b, w = int(ci[e]), int(cj[e]), float(cw[e])
        if a != b:
            Le[a, a] += w; Le[b, b] += w; Le[a, b] -= w; Le[b, a] -= w
        out[e] = np.linalg.eigvalsh(Le)[1]
    return out


def values_secular(L, ci, cj, cw, skip=None):
    ci, cj, cw = np.asarray(ci), np.asarray(cj), np.asarray(cw, dtype=np.float64)
    d, V = np.linalg.eigh(L)
    d, V = d[1:], V[:, 1:]                       # the zero eigenvalue (vector 1) does not move: a is orthogonal to 1
    xi2 = (V[ci] - V[cj]) ** 2                   # m x (n - 1)
    lo = np.full(len(cw), d[0])
    hi = np.full(len(cw), d[1])
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 + cw * np.sum(xi2 / (d[None, :] - mid[:, None]), axis=1)
        up = ~(f < 0)                             # the root is below mid (f increases from -inf at d_1 to +inf at d_2)
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    out = 0.5 * (lo + hi)
    if skip is not None:
        out = np.where(skip, np.nan, out)
    return out


def scan(vals):
    """The index-order scan: (winner or -1, its value)."""
    best, best_l2 = -1, 0.0
    for e, x in enumerate(vals):
        if np.isfinite(x) and x > best_l2 + TIE:
            best, best_l2 = e, float(x)
    return best, best_l2


def greedy(n, fi, fj, fw, ci, cj, cw, K, method="secular", order=None):
    """K picks (or a replay of `order`).  Per pick: the values of all unselected candidates (NaN for the selected), the bounds,
    lambda_2 before the pick, ||L_e||_inf per candidate, the absolute gap between the best and the second-best value."""
    f = values_brute if method == "brute" else values_secular
    L = laplacian(n, fi, fj, fw)
    sel = np.zeros(len(cw), dtype=bool)
    out = dict(order=[], lam2=[], values=[], bounds=[], lam_before=[], norms=[], gaps=[])
    for k in range(K):
        vals = f(L, ci, cj, cw, skip=sel)
        e = int(order[k]) if order is not None else scan(vals)[0]
        assert e >= 0 and not sel[e]
        srt = np.sort(vals[~sel])
        out["gaps"].append(float(srt[-1] - srt[-2]) if len(srt) > 1 else np.inf)
        out["values"].append(vals)
        out["bounds"].append(np.where(sel, np.nan, bounds(L, ci, cj, cw)))
        out["lam_before"].append(fiedler(L)[0])
        out["norms"].append(norm_inf_with(L, ci, cj, cw))
        out["order"].append(e)
        out["lam2"].append(float(vals[e]))
        sel[e] = True
        L = L + laplacian(n, [ci[e]], [cj[e]], [cw[e]])
    for key in ("order", "lam2", "gaps", "lam_before"):
        out[key] = np.array(out[key])
    return out
