"""NumPy restatement of GreedyEig's batched eigen-solver and of the drivers around it, written from the header comments of
mac_amd/csrc/eig.h and eig_exchange.h (for the tests; not a port of any kernel).  It exists to count: the device reports, per pick
or per exchange round, the operator applications it spent (one per column per iteration in which the column is still active after
the residual test).  Everything that decides a value is computed with the sparse L_cur on the device, so a wrong preconditioner
leaves every value right -- and shows only in these counts.

One column (``solve_columns``, all columns of a batch at once):
    x <- the start vector;  per iteration  lambda = x^T L_e x,  r = L_e x - lambda x,
    res = ||r||_1 / (2 max(maxdeg, max(deg_U, deg_V) + w));
    the best residual and the number of iterations in a row that have not halved it are kept;  a candidate column stops when
    res < 1e-8, a polish when res < 1e-8 and three iterations in a row have not halved the best residual;  500 iterations at most;
    w = centre(ext(M r[1:])) (ext: a zero for node 0), made orthogonal to x and normalised;  p made orthogonal to x and w and
    normalised;  either is dropped when what is left of it is at most 1e-12 of it (squared norms: rounding noise);
    Rayleigh-Ritz of L_e on {x, w, p} (numpy.linalg.eigh of the 3 x 3 Gram matrix, a dropped direction decoupled);
    p <- y_1 w + y_2 p,  x <- y_0 x + p, centred and normalised.

The preconditioner M:
    ``Exact``    the plain operation: the inverse of the reduced Laplacian L_e[1:, 1:] of the column's own graph, float64
                 (``extended=True``: inverted and applied in numpy.longdouble).  What the counts are pinned to.
    ``Composed`` the device's algebra: Sigma of the folded state, minus the pending block Zb diag(cb) Zb^T, minus the column's own
                 c_e z_e z_e^T (z_e = Sigma_cur a_e, c_e = w_e / (1 + w_e a_e^T z_e)); a fold when ``fold`` columns are pending.
                 ``damage=`` breaks one term:
                     no_cand              the c_e z_e z_e^T term is dropped
                     no_pending           the pending block is ignored by the application
                     no_fold              a fold discards its columns
                     fold_tail            a fold loses its last column
                     pad_rows             the rows n'..ld (Sigma = identity there, r = 0) are carried as live entries: the same
                                          numbers by construction -- the counts cannot see the padding
                     removal_as_addition  (exchange) c is computed with +w for a negated copy
                     no_trial_column      (exchange) a row's downdate is missing from the pending block
"""
import functools

import numpy as np

import eig_exchange_restatement as E
import eig_restatement as R

TOL = 1e-8
MAXIT = 500
DAMAGES = ("no_cand", "no_pending", "no_fold", "fold_tail", "pad_rows", "removal_as_addition", "no_trial_column")


class NotConverged(Exception):
    """A column hit the iteration cap (MACHIP_NOT_CONVERGED on the device)."""


# ---- inputs (the generators of tests/test_eig_gpu.py) ----
def chain_er(n, p, seed):
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < p
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def random_general(n=200, mc=300, seed=4):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, mc), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, mc + 20)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, mc + 20)


def incidence(n, U, V):
    """a_e = e_U - e_V per column, node 0 dropped: (n - 1) x B (U == V: a zero column)."""
    A = np.zeros((n, len(U)))
    cols = np.arange(len(U))
    A[U, cols] += 1.0
    A[V, cols] -= 1.0
    return A[1:]


def _inverse_extended(stack):
    """Gauss-Jordan inverse of a stack of symmetric positive definite matrices in numpy.longdouble (no pivoting needed)."""
    A = np.array(stack, dtype=np.longdouble)
    B, k, _ = A.shape
    inv = np.zeros_like(A)
    inv[:, np.arange(k), np.arange(k)] = 1.0
    for p in range(k):
        d = A[:, p, p][:, None].copy()
        A[:, p, :] /= d
        inv[:, p, :] /= d
        f = A[:, :, p].copy()
        f[:, p] = 0.0
        inv -= f[:, :, None] * inv[:, p, :][:, None, :]
        A -= f[:, :, None] * A[:, p, :][:, None, :]
    return inv


# ---- the preconditioners ----
class Exact:
    """M = (L_e[1:, 1:])^-1 of every column's own graph.  The state calls are no-ops: the graph is all it needs."""
    fold = None

    def __init__(self, extended=False):
        self.extended = extended
        self.pending = 0

    def reset(self, L0):
        self.pending = 0

    def push(self, n, u, v, w): pass
    def fold_now(self): pass
    def trial(self, n, u, v, w): pass
    def drop(self): pass

    def columns(self, L, U, V, w):
        n = L.shape[0]
        A = incidence(n, U, V)
        stack = L[1:, 1:][None, :, :] + np.asarray(w)[:, None, None] * (A.T[:, :, None] * A.T[:, None, :])
        if self.extended:
            Minv = _inverse_extended(stack)
            return lambda act, Rr: np.einsum("bij,jb->ib", Minv[act], Rr.astype(np.longdouble)).astype(np.float64)
        state = [np.arange(len(U)), np.linalg.inv(stack)]      # the columns still held (they only ever retire), their inverses

        def apply(act, Rr):
            if len(act) != len(state[0]):
                keep = np.isin(state[0], act)
                state[0], state[1] = state[0][keep], state[1][keep]
            return np.matmul(state[1], Rr.T[:, :, None])[:, :, 0].T
        return apply


class Composed:
    """The device's algebra, one term of which ``damage`` breaks."""

    def __init__(self, fold, damage=None, ld=None):
        assert damage is None or damage in DAMAGES
        self.fold, self.damage, self.ld = fold, damage, ld

    @property
    def pending(self):
        return len(self.cb)

    def _pad(self, A):
        """pad_rows: rows n'..ld of a matrix of node-space columns as explicit zeros."""
        if self.damage != "pad_rows":
            return A
        return np.vstack([A, np.zeros((self.S.shape[0] - A.shape[0], A.shape[1]))])

    def reset(self, L0):
        S = np.linalg.inv(L0[1:, 1:])
        if self.damage == "pad_rows":
            ld = self.ld if self.ld is not None else (S.shape[0] + 63) // 64 * 64
            P = np.eye(ld)
            P[:S.shape[0], :S.shape[0]] = S
            S = P
        self.S, self.Zb, self.cb = S, [], []

    def _z(self, A):
        Z = self.S @ A
        for z, c in zip(self.Zb, self.cb):
            Z -= z[:, None] * (c * (z @ A))[None, :]
        return Z

    def _c(self, w, s):
        if self.damage == "removal_as_addition":
            w = np.abs(w)
        return w / (1.0 + w * s)

    def _append(self, n, u, v, w):
        A = self._pad(incidence(n, [u], [v]))
        z = self._z(A)[:, 0]
        self.Zb.append(z)
        self.cb.append(float(self._c(np.float64(w), float(A[:, 0] @ z))))

    def push(self, n, u, v, w):
        self._append(n, u, v, w)
        if self.pending == self.fold:
            self.fold_now()

    def fold_now(self):
        cols = list(zip(self.Zb, self.cb))
        if self.damage == "no_fold":
            cols = []
        elif self.damage == "fold_tail":
            cols = cols[:-1]
        for z, c in cols:
            self.S = self.S - c * np.outer(z, z)
        self.Zb, self.cb = [], []

    def trial(self, n, u, v, w):
        self._tried = self.damage != "no_trial_column"
        if self._tried:
            self._append(n, u, v, w)

    def drop(self):
        if self._tried:
            self.Zb.pop(); self.cb.pop()

    def columns(self, L, U, V, w):
        n = L.shape[0]
        A = self._pad(incidence(n, U, V))
        Z = self._z(A)
        cc = self._c(np.asarray(w, dtype=np.float64), np.sum(A * Z, axis=0))
        if self.damage == "no_cand":
            cc = np.zeros_like(cc)
        S = self.S
        Zb = np.array(self.Zb).T if self.Zb and self.damage != "no_pending" else None
        cb = np.array(self.cb)

        def apply(act, Rr):
            Rr = self._pad(Rr)
            T = S @ Rr
            if Zb is not None:
                T -= Zb @ (cb[:, None] * (Zb.T @ Rr))
            T -= Z[:, act] * (cc[act] * np.sum(Z[:, act] * Rr, axis=0))[None, :]
            return T[:n - 1]
        return apply


# ---- the solver ----
def _lmul(L, X, U, V, w, cols):
    Y = L @ X
    d = w * (X[U, cols] - X[V, cols])
    Y[U, cols] += d
    Y[V, cols] -= d
    return Y


def solve_columns(L, U, V, w, start, apply, polish=False, apply_noise=0.0, rng=None):
    """The columns (U_b, V_b, w_b) on the graph L (U == V: L itself) from ``start`` (n, or n x B).  dict(lam, X, napp, iters)."""
    U, V, w = np.asarray(U, dtype=np.int64), np.asarray(V, dtype=np.int64), np.asarray(w, dtype=np.float64)
    n, B = L.shape[0], len(w)
    deg = np.diag(L)
    md = np.maximum(deg.max(), np.where(U != V, np.maximum(deg[U], deg[V]) + w, -np.inf))
    X = np.array(np.broadcast_to(start[:, None] if np.ndim(start) == 1 else start, (n, B)), dtype=np.float64)
    P = np.zeros((n, B))
    lam, rbest, stall = np.zeros(B), np.full(B, np.inf), np.zeros(B, dtype=np.int64)
    iters = np.zeros(B, dtype=np.int64)
    act = np.arange(B)
    tol = 0.0 if polish else TOL
    napp = 0
    for it in range(MAXIT + 2):
        Xa = X[:, act]
        ca = np.arange(len(act))
        LX = _lmul(L, Xa, U[act], V[act], w[act], ca)
        la = np.sum(Xa * LX, axis=0)
        Rs = LX - la * Xa
        res = np.abs(Rs).sum(axis=0) / (2.0 * md[act])
        lam[act] = la
        better = res < 0.5 * rbest[act]
        rbest[act] = np.where(better, res, rbest[act])
        stall[act] = np.where(better, 0, stall[act] + 1)
        done = (res < tol) | ((res < TOL) & (stall[act] >= 3))
        if np.any(~done & ((it >= MAXIT) | ~(res == res))):
            raise NotConverged(f"{int(np.sum(~done))} columns after {it} iterations")
        keep = ~done
        act, Xa, LX, Rs, la = act[keep], Xa[:, keep], LX[:, keep], Rs[:, keep], la[keep]
        if len(act) == 0:
            break
        napp += len(act)
        iters[act] += 1
        ca = np.arange(len(act))
        T = apply(act, Rs[1:])
        if apply_noise:
            T = T * (1.0 + apply_noise * rng.standard_normal(T.shape))
        W = np.vstack([np.zeros((1, len(act))), T])
        W -= W.mean(axis=0)
        ww0 = np.sum(W * W, axis=0)
        W -= np.sum(Xa * W, axis=0) * Xa
        ww = np.sum(W * W, axis=0)
        wi = np.where(ww > 1e-12 * ww0, 1.0 / np.sqrt(np.where(ww > 0.0, ww, 1.0)), 0.0)
        W *= wi
        Pa = P[:, act]
        if it > 0:
            pp0 = np.sum(Pa * Pa, axis=0)
            Pa = Pa - np.sum(Xa * Pa, axis=0) * Xa - np.sum(W * Pa, axis=0) * W
            pp = np.sum(Pa * Pa, axis=0)
            pi = np.where(pp > 1e-12 * pp0, 1.0 / np.sqrt(np.where(pp > 0.0, pp, 1.0)), 0.0)
            Pa = Pa * pi
        else:
            pi = np.zeros(len(act))
        LW = _lmul(L, W, U[act], V[act], w[act], ca)
        LP = _lmul(L, Pa, U[act], V[act], w[act], ca)
        xlw, xlp, wlw = np.sum(LX * W, axis=0), np.sum(LX * Pa, axis=0), np.sum(W * LW, axis=0)
        wlp, plp = np.sum(LW * Pa, axis=0), np.sum(Pa * LP, axis=0)
        big = 4.0 * (np.abs(la) + np.abs(wlw) + np.abs(plp)) + 1.0
        now, nop = wi == 0.0, pi == 0.0
        G = np.empty((len(act), 3, 3))
        G[:, 0, 0] = la
        G[:, 0, 1] = G[:, 1, 0] = np.where(now, 0.0, xlw)
        G[:, 0, 2] = G[:, 2, 0] = np.where(nop, 0.0, xlp)
        G[:, 1, 2] = G[:, 2, 1] = np.where(now | nop, 0.0, wlp)
        G[:, 1, 1] = np.where(now, big, wlw)
        G[:, 2, 2] = np.where(nop, big, plp)
        y = np.linalg.eigh(G)[1][:, :, 0]
        D = y[:, 1] * W + y[:, 2] * Pa
        P[:, act] = D
        Xn = y[:, 0] * Xa + D
        Xn -= Xn.mean(axis=0)
        Xn /= np.sqrt(np.sum(Xn * Xn, axis=0))
        X[:, act] = Xn
    return dict(lam=lam, X=X, napp=napp, iters=iters)


def _perturbed(v, eps, rng):
    if not eps:
        return v
    x = v + eps * rng.standard_normal(v.shape) * np.linalg.norm(v) / np.sqrt(len(v))
    x -= x.mean()
    return x / np.linalg.norm(x)


# ---- machip_eig::select ----
def select(g, K, batch=512, M=None, apply_noise=0.0, start_noise=0.0, seed=0):
    """K picks.  dict(order, lam2, solved, applications, pending (at the start of each pick), decisions: per pick the (bound of the
    batch's first candidate, top) of every batch after the first)."""
    n, fi, fj, fw, ci, cj, cw = g
    ci, cj, cw = np.asarray(ci, dtype=np.int64), np.asarray(cj, dtype=np.int64), np.asarray(cw, dtype=np.float64)
    M = Exact() if M is None else M
    rng = np.random.default_rng(seed)
    kw = dict(apply_noise=apply_noise, rng=rng)
    m = len(cw)
    L = R.laplacian(n, fi, fj, fw)
    M.reset(L)
    lam, v = R.fiedler(L)
    sel = np.zeros(m, dtype=bool)
    out = dict(order=[], lam2=[], solved=[], applications=[], pending=[], decisions=[])
    for k in range(K):
        out["pending"].append(M.pending)
        u = lam + cw * (v[ci] - v[cj]) ** 2
        unsel = np.flatnonzero(~sel)
        order = unsel[np.argsort(-u[unsel], kind="stable")]
        top, napp, nsolved = -np.inf, 0, 0
        l2 = np.full(m, np.nan)
        last, lastX, dec = np.zeros(0, dtype=np.int64), None, []
        for q in range(0, len(order), batch):
            if q:
                dec.append((float(u[order[q]]), float(top)))
            if u[order[q]] < top:
                break
            es = order[q:q + batch]
            r = solve_columns(L, ci[es], cj[es], cw[es], _perturbed(v, start_noise, rng), M.columns(L, ci[es], cj[es], cw[es]), **kw)
            l2[es] = r["lam"]
            top = max(top, float(r["lam"].max()))
            napp += r["napp"]; nsolved += len(es)
            last, lastX = es, r["X"]
        best = R.scan(l2)[0]
        assert best >= 0, f"no candidate raises lambda_2 at pick {k}"
        at = np.flatnonzero(last == best)
        start = lastX[:, at[0]] if len(at) else v
        one = ([ci[best]], [cj[best]], [cw[best]])
        r = solve_columns(L, *one, start, M.columns(L, *one), polish=True, **kw)
        napp += r["napp"]
        lam, v = float(r["lam"][0]), r["X"][:, 0]
        M.push(n, ci[best], cj[best], cw[best])
        sel[best] = True
        L = L + E.edge_lap(n, ci[best], cj[best], cw[best])
        out["order"].append(int(best)); out["lam2"].append(lam); out["solved"].append(nsolved); out["applications"].append(napp)
        out["decisions"].append(dec)
    for key in ("order", "lam2", "solved", "applications", "pending"):
        out[key] = np.array(out[key])
    return out


# ---- round 0 of eig_exchange ----
def exchange_round0(g, start, batch=512, M=None, min_gain=0.0, apply_noise=0.0, start_noise=0.0, seed=0):
    """dict(swap, value, solved, applications, removal, pairs (the solved ones), pending (when the rows are tried), decisions:
    (bound, max(tau, top)) of every row visit and of every batch)."""
    n, fi, fj, fw, ci, cj, cw = g
    ci, cj, cw = np.asarray(ci, dtype=np.int64), np.asarray(cj, dtype=np.int64), np.asarray(cw, dtype=np.float64)
    M = Exact() if M is None else M
    rng = np.random.default_rng(seed)
    kw = dict(apply_noise=apply_noise, rng=rng)
    m = len(cw)
    rows = sorted(int(e) for e in start)
    K = len(rows)
    ra = np.array(rows)
    M.reset(R.laplacian(n, fi, fj, fw))
    for e in rows:
        M.push(n, ci[e], cj[e], cw[e])
    L = E.lap_of(g, rows)
    lam, v = R.fiedler(L)
    if M.fold is not None and M.pending > 0 and M.pending + 2 > M.fold:
        M.fold_now()
    tau = lam + min_gain
    napp, nsolved = 0, 0
    Vr, lamr = np.zeros((n, K)), np.zeros(K)
    for q in range(0, K, batch):
        rs = ra[q:q + batch]
        r = solve_columns(L, ci[rs], cj[rs], -cw[rs], _perturbed(v, start_noise, rng), M.columns(L, ci[rs], cj[rs], -cw[rs]), **kw)
        Vr[:, q:q + batch], lamr[q:q + batch] = r["X"], r["lam"]
        napp += r["napp"]
    insel = np.zeros(m, dtype=bool)
    insel[ra] = True
    unsel = np.flatnonzero(~insel)
    U = np.where(insel[None, :], -np.inf, lamr[:, None] + cw[None, :] * (Vr[ci, :] - Vr[cj, :]).T ** 2)
    rowmax = U.max(axis=1)
    top = -np.inf
    pairs, dec = {}, []
    last_row, last, lastX = -1, np.zeros(0, dtype=np.int64), None
    pending_at_rows = M.pending
    for r_ in np.argsort(-rowmax, kind="stable"):
        dec.append((float(rowmax[r_]), float(max(tau, top))))
        if not rowmax[r_] > max(tau, top):
            break
        e = rows[r_]
        M.trial(n, ci[e], cj[e], -cw[e])
        Le = L - E.edge_lap(n, ci[e], cj[e], cw[e])
        order = unsel[np.argsort(-U[r_, unsel], kind="stable")]
        for q in range(0, len(order), batch):
            dec.append((float(U[r_, order[q]]), float(max(tau, top))))
            if U[r_, order[q]] < max(tau, top):
                break
            fs = order[q:q + batch]
            r = solve_columns(Le, ci[fs], cj[fs], cw[fs], _perturbed(Vr[:, r_], start_noise, rng), M.columns(Le, ci[fs], cj[fs], cw[fs]), **kw)
            for f, val in zip(fs, r["lam"]):
                pairs[(int(e), int(f))] = float(val)
            top = max(top, float(r["lam"].max()))
            napp += r["napp"]; nsolved += len(fs)
            last_row, last, lastX = r_, fs, r["X"]
        M.drop()
    swap, value = E.scan(pairs, tau)
    if swap is not None:
        e, f = swap
        row = rows.index(e)
        M.push(n, ci[e], cj[e], -cw[e])
        M.push(n, ci[f], cj[f], cw[f])
        Ln = L - E.edge_lap(n, ci[e], cj[e], cw[e]) + E.edge_lap(n, ci[f], cj[f], cw[f])
        at = np.flatnonzero(last == f) if last_row == row else []
        none = ([0], [0], [0.0])
        r = solve_columns(Ln, *none, lastX[:, at[0]] if len(at) else Vr[:, row], M.columns(Ln, *none), polish=True, **kw)
        napp += r["napp"]
        value = float(r["lam"][0])
    return dict(swap=swap, value=value, solved=nsolved, applications=napp, removal=K, pairs=pairs, pending=pending_at_rows,
                decisions=dec, tau=tau)


# ---- what the tests pin: per input, the exact counts and the smallest damage ----
def greedy_variants(fold, K):
    """{damage: the picks it can differ at} for a greedy run (a variant that is active nowhere is left out; with fold = 1 a fold's
    last column is its only one, so fold_tail is no_fold)."""
    k = np.arange(K)
    act = {"no_cand": k >= 0, "no_pending": k % fold > 0, "no_fold": k >= fold}
    if fold > 1:
        act["fold_tail"] = k >= fold
    return {d: a for d, a in act.items() if a.any()}


def excess(ref, run_variant, active):
    """A_variant - A_ref on the active entries (inf where the variant did not converge: the suite sees that already), nan elsewhere."""
    try:
        a = np.atleast_1d(run_variant()).astype(np.float64)
    except NotConverged:
        a = np.full(len(ref), np.inf)
    return np.where(active, a - ref, np.nan)


# ---- the inputs the two test modules share, and what is computed from them once per process ----
K_PICKS = 10
K_XCH = 8
FOLDS = (1, 3, 16)
GREEDY_CASES = [(name, fold, 512) for name in ("chain150", "general150", "chain129") for fold in FOLDS] + [("chain150", 3, 64)]


@functools.lru_cache(maxsize=None)
def graph(name):
    """chain150: ld = 192, padding rows.  general150: a tree plus 75 fixed edges, the dense form.  chain129: n' = ld = 128, no
    padding rows.  chain40: the exchange's pinned input."""
    return {"chain150": lambda: chain_er(150, 0.02, 3), "general150": lambda: random_general(150, 200, 4),
            "chain129": lambda: chain_er(129, 0.02, 3), "chain40": lambda: chain_er(40, 0.1, 1)}[name]()


def prune_tol(g):
    """What the neighbouring tests allow a device value to be off by where a decision hangs on it: 1e-8 + 2e-8 ||L||_inf (L with
    every candidate in: above every L_e's norm)."""
    n, fi, fj, fw, ci, cj, cw = g
    return 1e-8 + 2e-8 * R.norm_inf(R.laplacian(n, np.concatenate([fi, ci]), np.concatenate([fj, cj]), np.concatenate([fw, cw])))


@functools.lru_cache(maxsize=None)
def greedy_exact(name, batch):
    return select(graph(name), K_PICKS, batch=batch)


@functools.lru_cache(maxsize=None)
def greedy_reference(name, fold, batch):
    """dict(run: the exact replay, A: its applications per pick, excess: {damage: A_damaged - A on the picks it is active at}, D:
    the smallest excess of any active variant per pick)."""
    run = greedy_exact(name, batch)
    A = run["applications"].astype(np.float64)
    ex = {d: excess(A, lambda: select(graph(name), K_PICKS, batch=batch, M=Composed(fold, d))["applications"], act)
          for d, act in greedy_variants(fold, K_PICKS).items()}
    return dict(run=run, A=A, excess=ex, D=np.nanmin(np.array(list(ex.values())), axis=0))


@functools.lru_cache(maxsize=None)
def exchange_start():
    return tuple(E.greedy_start(graph("chain40"), K_XCH))


@functools.lru_cache(maxsize=None)
def exchange_exact():
    return exchange_round0(graph("chain40"), exchange_start())


def exchange_variants(fold):
    """The variants round 0 can differ under.  The trial column is a pending column, so no_pending is active whatever the fold;
    a fold happens while the selection is loaded (fold <= K) or at the start of the round."""
    pend = K_XCH % fold
    folds = fold <= K_XCH or (pend > 0 and pend + 2 > fold)
    return ["no_cand", "no_pending", "removal_as_addition", "no_trial_column"] + (["no_fold"] if folds else []) + (["fold_tail"] if folds and fold > 1 else [])


@functools.lru_cache(maxsize=None)
def exchange_reference(fold):
    """The same for round 0 of the exchange on chain40 from the greedy's K = 8 (one entry instead of one per pick)."""
    run = exchange_exact()
    A = np.array([float(run["applications"])])
    ex = {d: excess(A, lambda: exchange_round0(graph("chain40"), exchange_start(), M=Composed(fold, d))["applications"], np.array([True]))
          for d in exchange_variants(fold)}
    return dict(run=run, A=A, excess=ex, D=np.nanmin(np.array(list(ex.values())), axis=0))
