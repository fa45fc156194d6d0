"""NumPy restatement of the best-swap local search on lambda_2 (GreedyEig.exchange), written from the rules (for the tests; not a
port of any implementation).

S the selection (K candidates), L_S the Laplacian of the fixed edges plus S, tau = lambda_2(L_S) + min_gain.  A round looks at the
pairs (e in S, f outside S), worth lambda_2(L_S - w_e a_e a_e^T + w_f a_f a_f^T), scans them in (e ascending, f ascending) order with
a running value that starts at tau -- a pair replaces it only if it exceeds it by more than 1e-8 -- and swaps the pair the scan
ends on; no pair: converged.

  * ``brute``: every pair by numpy.linalg.eigvalsh, then the scan.
  * ``pruned``: the removal pairs (lambda_2(S - e), v^-e) first; by concavity of lambda_2 in the weights
    u(e, f) = lambda_2(S - e) + w_f (v^-e_i - v^-e_j)^2 >= the pair's value.  Rows e in decreasing order of their largest bound
    while that is above max(tau, top), top the largest value solved so far in the round; in a row the candidates in decreasing
    order of the bound, batch after batch, until a batch's first bound is below max(tau, top).  Then the same scan over the solved
    pairs.  Returns which pairs were solved.
The rows keep their places: the selection ascending at the start, a swap puts f where e was (this decides ties between rows only).
"""
import numpy as np

import eig_restatement as R

TIE = 1e-8


def edge_lap(n, i, j, w):
    return R.laplacian(n, [i], [j], [w])


def lap_of(g, sel):
    n, fi, fj, fw, ci, cj, cw = g
    sel = np.asarray(sel, dtype=np.int64)
    return R.laplacian(n, np.concatenate([fi, np.asarray(ci)[sel]]), np.concatenate([fj, np.asarray(cj)[sel]]),
                       np.concatenate([fw, np.asarray(cw)[sel]]))


def naive_start(g, k):
    return list(range(k))


def greedy_start(g, k):
    return sorted(int(e) for e in R.greedy(*g, k, method="brute")["order"])


def values_secular(L, ci, cj, cw, iters=64):
    """eig_restatement.values_secular's bisection (lambda_2 of L + w a a^T is the root of 1 + w sum_i xi_i^2 / (d_i - mu) between the
    two smallest non-zero eigenvalues of L) with 64 halvings instead of 200: the bracket is below 1e-19 of its width afterwards, and
    the large inputs take a quarter of the time."""
    ci, cj, cw = np.asarray(ci), np.asarray(cj), np.asarray(cw, dtype=np.float64)
    d, V = np.linalg.eigh(L)
    d, V = d[1:], V[:, 1:]
    xi2 = (V[ci] - V[cj]) ** 2
    lo, hi = np.full(len(cw), d[0]), np.full(len(cw), d[1])
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 + cw * np.sum(xi2 / (d[None, :] - mid[:, None]), axis=1)
        up = ~(f < 0)
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return 0.5 * (lo + hi)


def scan(pairs, tau):
    """pairs: dict (e, f) -> value.  The (e, f)-order scan: (winner or None, its value)."""
    best, running = None, tau
    for key in sorted(pairs):
        if pairs[key] > running + TIE:
            best, running = key, float(pairs[key])
    return best, running


def brute_round(g, rows, min_gain=0.0):
    """All K (m - K) values of one round: dict(lam, tau, values {(e, f): value}, swap, value, best, second, norm)."""
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    L = lap_of(g, rows)
    lam = R.fiedler(L)[0]
    tau = lam + min_gain
    insel = np.zeros(m, dtype=bool)
    insel[rows] = True
    vals = {}
    norm = 0.0
    for e in rows:
        Le = L - edge_lap(n, ci[e], cj[e], cw[e])
        x = R.values_brute(Le, ci, cj, cw, skip=insel)
        norm = max(norm, float(np.nanmax(np.where(insel, np.nan, R.norm_inf_with(Le, ci, cj, cw)))))
        for f in np.flatnonzero(~insel):
            vals[(int(e), int(f))] = float(x[f])
    swap, value = scan(vals, tau)
    srt = np.sort(np.array(list(vals.values())))
    return dict(lam=lam, tau=tau, values=vals, swap=swap, value=value, best=float(srt[-1]), second=float(srt[-2]) if len(srt) > 1 else -np.inf,
                norm=norm)


def removal_pairs(g, rows):
    """[(lambda_2(S - e), its unit Fiedler vector)] per row."""
    n, fi, fj, fw, ci, cj, cw = g
    L = lap_of(g, rows)
    return [R.fiedler(L - edge_lap(n, ci[e], cj[e], cw[e])) for e in rows]


def bound_matrix(g, rows, pairs=None):
    """u(e, f) for every row and every candidate, -inf for the selected f."""
    n, fi, fj, fw, ci, cj, cw = g
    pairs = removal_pairs(g, rows) if pairs is None else pairs
    insel = np.zeros(len(cw), dtype=bool)
    insel[rows] = True
    U = np.empty((len(rows), len(cw)))
    for r, (lam, v) in enumerate(pairs):
        U[r] = np.where(insel, -np.inf, lam + np.asarray(cw) * (v[np.asarray(ci)] - v[np.asarray(cj)]) ** 2)
    return U


def one_pair_bounds(g, rows):
    """lambda_2(S) - g_e + g_f, g the supergradient of lambda_2 at S: the cheaper bound (also valid, by the same concavity)."""
    n, fi, fj, fw, ci, cj, cw = g
    lam, v = R.fiedler(lap_of(g, rows))
    gr = np.asarray(cw) * (v[np.asarray(ci)] - v[np.asarray(cj)]) ** 2
    return lam - gr[np.asarray(rows)][:, None] + gr[None, :]


def pruned_round(g, rows, min_gain=0.0, batch=512, method="brute"):
    """One round by the pruning rules: dict(lam, tau, values {(e, f): value} of the solved pairs, swap, value, top, U)."""
    n, fi, fj, fw, ci, cj, cw = g
    ci, cj, cw = np.asarray(ci), np.asarray(cj), np.asarray(cw, dtype=np.float64)
    m = len(cw)
    f_values = R.values_brute if method == "brute" else values_secular
    L = lap_of(g, rows)
    lam = R.fiedler(L)[0]
    tau = lam + min_gain
    U = bound_matrix(g, rows)
    insel = np.zeros(m, dtype=bool)
    insel[rows] = True
    unsel = np.flatnonzero(~insel)
    rowmax = U.max(axis=1)
    top = -np.inf
    vals = {}
    for r in np.argsort(-rowmax, kind="stable"):
        if not rowmax[r] > max(tau, top):
            break
        e = rows[r]
        Le = L - edge_lap(n, ci[e], cj[e], cw[e])
        ord_ = unsel[np.argsort(-U[r, unsel], kind="stable")]
        for q in range(0, len(ord_), batch):
            if U[r, ord_[q]] < max(tau, top):
                break
            fs = ord_[q:q + batch]
            x = f_values(Le, ci[fs], cj[fs], cw[fs])
            for f, val in zip(fs, x):
                vals[(int(e), int(f))] = float(val)
            top = max(top, float(np.max(x)))
    swap, value = scan(vals, tau)
    return dict(lam=lam, tau=tau, values=vals, swap=swap, value=value, top=top, U=U)


def _run(round_fn, g, start, max_swaps, min_gain, **kw):
    rows = sorted(int(e) for e in start)
    out = dict(swaps=[], lambda2=[], rounds=[], converged=False)
    while True:
        if len(out["swaps"]) >= max_swaps:
            out["lambda2"].append(R.fiedler(lap_of(g, rows))[0])
            break
        r = round_fn(g, rows, min_gain, **kw)
        out["rounds"].append(r)
        out["lambda2"].append(r["lam"])
        if r["swap"] is None:
            out["converged"] = True
            break
        e, f = r["swap"]
        rows[rows.index(e)] = f
        out["swaps"].append((e, f))
    out["selection"] = sorted(rows)
    out["lambda2"] = np.array(out["lambda2"])
    return out


def brute(g, start, max_swaps, min_gain=0.0):
    """dict(swaps [(out, in)], lambda2 (swaps + 1 values), rounds (brute_round per round, the stopping one included), converged,
    selection)."""
    return _run(brute_round, g, start, max_swaps, min_gain)


def pruned(g, start, max_swaps, min_gain=0.0, batch=512, method="brute"):
    """The same dict; a round's ``values`` holds the solved pairs only."""
    return _run(pruned_round, g, start, max_swaps, min_gain, batch=batch, method=method)
