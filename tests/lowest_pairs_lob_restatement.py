"""NumPy restatement of the preconditioned deflated columns of machip_lowest_pairs (mac_amd/csrc/solver_pairs_lob.h, DESIGN section
25), written from the headers.  Test infrastructure only.

Column c >= 1 is the block-size-1 LOBPCG of tests/lob_restatement.py (its recurrence, its Rayleigh-Ritz, its host loop of chunks,
forecasts and explicit checks) in the complement of the locked block Q = [1/sqrt(n), v_0 .. v_{c-1}]:
    start       column c of the start block, projected twice against Q, normalised, checked (a warm block passes with 0 iterations)
    iteration   w = M^-1 r, then  w <- w - Q (Q^T w);  L w is the product of the projected w
    check       x projected twice against Q, normalised, a fresh product, ||L x - rq x||_1 / ||L||_inf < tol accepts the column;
                otherwise the recurrence restarts from that x, at most 12 times
M^-1 is the reference preconditioner of lob_restatement (`ExactInverse` at sigma = 1e-8 ||L||_inf, `TriExact` at 2.5e-7 ||L||_inf).
Column 0 is the same iteration with Q = [1/sqrt(n)] (on the device: the handle's Fiedler solve).

Per column the restatement returns the iteration count at the chunk end the solve stopped on (J_ref), the restarts and the drift
max |Q^T x| / ||x|| over the iterates.  Damaged variants:
    no_projection               the column never projects: not its start, not w, not x before a check
    skip_last_locked            every projection leaves out the newest locked column
    project_once_at_start_only  the start vector is projected once; nothing afterwards (w, x before a check)
"""
import collections
import math

import numpy as np
import scipy.sparse as sp

import lob_restatement as LR
import lowest_pairs_restatement as R

VARIANTS = (None, "no_projection", "skip_last_locked", "project_once_at_start_only")
OK, NOT_CONVERGED = 0, 1


def _proj(x, Q):
    return x - Q @ (Q.T @ x) if Q.shape[1] else x


def _check(L, v, Q, times):
    y = v
    for _ in range(times):
        y = _proj(y, Q)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = y / np.linalg.norm(y)
    Ly = L @ y
    rq = float(y @ Ly)
    return y, Ly, rq, float(np.abs(Ly - rq * y).sum())


def column(L, apply, Qfull, x0, wb, lob_chunk=16, tol=LR.TOL, cap=LR.LOB_CAP, variant=None):
    """One column in the complement of Qfull (n x nq).  dict(iters, restarts, lam, v, res, drift, converged)."""
    assert variant in VARIANTS
    scale = LR.norm_inf(L)
    Q = Qfull[:, :-1] if variant == "skip_last_locked" and Qfull.shape[1] > 1 else Qfull
    none = Qfull[:, :0]
    Qs = none if variant == "no_projection" else Q                                           # the start's
    Qw = none if variant in ("no_projection", "project_once_at_start_only") else Q          # w's and the checks'
    y, Ly, rq, r1 = _check(L, np.asarray(x0, dtype=np.float64), Qs, 1 if variant == "project_once_at_start_only" else 2)
    drift = [float(np.abs(Qfull.T @ y).max())]
    out = dict(iters=0, restarts=0, lam=rq, v=y, res=r1 / scale, drift=drift[0], converged=True)
    if out["res"] < tol:
        return out
    cap = min(LR.LOB_CAP, cap)
    chunk0 = 4 if wb else min(32, max(1, lob_chunk))
    ltarget = math.log(max(tol * scale, 1e-300))
    dev = LR._Recurrence(L, lambda r: _proj(apply(r), Qw), True, None, 0.0)
    it_enq = restarts = 0
    est_of = {}
    while True:
        est_of[it_enq] = dev.start(y, Ly, rq)
        pend, hist = collections.deque(), collections.deque()
        bad_at = {}
        to_go, check, ramp = 1e18, False, (2 if wb else 4)
        while not check:
            near = to_go < 2.0 * chunk0
            depth = 1 if (near or wb) else 2
            while len(pend) < depth and it_enq < cap:
                chunk = min(chunk0, ramp)
                ramp = min(chunk0, ramp * 2)
                if near:
                    chunk = min(chunk, max(2, int(0.75 * to_go) + 1))
                chunk = min(chunk, cap - it_enq)
                for _ in range(chunk):
                    it_enq += 1
                    est_of[it_enq] = dev.step()
                    with np.errstate(invalid="ignore", divide="ignore"):
                        drift.append(float(np.abs(Qfull.T @ dev.x).max() / np.linalg.norm(dev.x)))
                bad_at[it_enq] = dev.bad
                pend.append(it_enq)
            if not pend:
                break
            jend = pend.popleft()
            est, bad = est_of[jend], bad_at[jend]
            if est > 0.0:
                hist.append((jend, math.log(est)))
                while len(hist) > 2 and hist[1][0] <= jend - 48:
                    hist.popleft()
                to_go = 1e18
                if hist[0][0] < jend:
                    slope = (hist[0][1] - hist[-1][1]) / (jend - hist[0][0])
                    if slope > 1e-7:
                        to_go = max(0.0, (hist[-1][1] - ltarget) / slope)
            if bad or not est == est or est < tol * scale or jend >= cap:
                check = True
        y, Ly, rq, r1 = _check(L, dev.x, Qw, 2)
        out.update(iters=it_enq, restarts=restarts, lam=rq, v=y, res=r1 / scale, drift=float(np.nanmax(drift)))
        if not rq == rq:
            out["converged"] = False
            return out
        if out["res"] < tol:
            return out
        restarts += 1
        if it_enq >= cap or restarts > 12:
            out["converged"] = False
            return out


def preconditioner(L, exact):
    sg = (1e-8 if exact else 2.5e-7) * LR.norm_inf(L)
    return LR.ExactInverse(L, sg) if exact else LR.TriExact(L, sg)


def lowest_pairs(L, q, exact, X0=None, lob_chunk=16, tol=LR.TOL, variant=None, cap=LR.LOB_CAP):
    """(lams, V, info) in sorted order as find_lowest_pairs(method="lobpcg") returns them; info adds J_ref (= steps), drift and rank0, the rank of column 0.
    The variant damages columns 1 .. q-1 only."""
    L = sp.csr_matrix(L, dtype=np.float64)
    n = L.shape[0]
    assert 1 <= q <= min(16, n - 1)
    lnorm = R.lnorm_inf(L)
    X0 = R.reference_block(n, q) if X0 is None else np.asarray(X0, dtype=np.float64)
    M = preconditioner(L, exact)
    Q = np.full((n, 1), 1.0 / np.sqrt(n))
    cols = []
    for c in range(q):
        o = column(L, M.apply, Q, X0[:, c], exact, lob_chunk=lob_chunk, tol=tol, cap=cap, variant=variant if c else None)
        cols.append(o)
        Q = np.column_stack([Q, o["v"]])
    lams = np.array([o["lam"] for o in cols])
    order = np.argsort(lams, kind="stable")
    first_rank = int(np.sum(lams < lams[0] - tol * lnorm))
    pick = lambda k, dt=float: np.array([cols[c][k] for c in order], dtype=dt)
    info = {"residual": pick("res"), "steps": pick("iters", int), "restarts": pick("restarts", int), "J_ref": pick("iters", int),
            "status": np.array([OK if cols[c]["converged"] else NOT_CONVERGED for c in order]), "drift": pick("drift"),
            "rank0": int(np.nonzero(order == 0)[0][0]), "reordered": int(first_rank != 0), "first_rank": first_rank, "gap": float(lams[order][1] - lams[order][0]) if q >= 2 else None}
    return lams[order], Q[:, 1:][:, order], info


# ---- the inputs the host and the GPU tests share ----
# tri_n2048_s30 stands in for lob_restatement's tri_n2000_s30 (tridiagonal tier, c = 2): on that one this restatement itself restarts
# twice in one column (658 iterations, the recurrence's residual undershoots the true one), and the route asserts allow no restart;
# 2 048 is the largest n at c = 2, every thread busy, and the restatement runs it in 130 to 233 iterations without a restart
SYNTH = ("n257_s63", "n1024_s64", "n1025_s65_kinds", "n4096_s129", "n4097_s65", "n16384_s65", "n16385_s129", "tri_n300_s30", "tri_n2048_s30")
OWN = {"tri_n2048_s30": lambda: LR._case("tri_n2048_s30", 2048, 30, 0.5, 22, exact=False, options=LR.TRI_OPTS, note="tridiagonal, c = 2, full")}
GOLDEN = {"g2o_intel": ("x_init", 4), "g2o_sphere2500": ("ones", 5)}
SMALL = {"c64": 4, "p300": 4, "k5": 4}
Input = collections.namedtuple("Input", "name case L q exact lob_chunk s")


def golden(name):
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False))


def _as_case(name, n, fi, fj, fw, ci, cj, cw, x):
    i32 = lambda a: np.asarray(a).astype(np.int32)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    return LR.Case(name, int(n), i32(fi), i32(fj), f64(fw), i32(ci), i32(cj), f64(cw), f64(x), None, True, {}, (), 0, "")


def closures_upper(L):
    """Stored off-band entries of the upper triangle of a matrix without duplicated pairs."""
    return int(sp.triu(sp.csr_matrix(L), 2).nnz)


_INPUTS = {}


def problem(name):
    """Input(name, case, L, q, exact, lob_chunk, s): the handle's edge lists and x (a lob_restatement Case), the matrix, the columns
    asked for, the tier the library takes (exact: the graph has closures and woodbury is on), its chunk length, and the closures as
    the library counts them (one per stored off-band entry of the assembly: lob_restatement.closures_of)."""
    if name in _INPUTS:
        return _INPUTS[name]
    if name in SYNTH:
        cs = OWN[name]() if name in OWN else LR.case(name)
        out = Input(name, cs, LR.laplacian(cs), 4, cs.exact, cs.options.get("lob_chunk", 16), len(LR.closures_of(cs)[0]))
    else:
        if name in GOLDEN:
            which, q = GOLDEN[name]
            g = golden(name)
            x = np.asarray(g["x_init"], dtype=np.float64) if which == "x_init" else np.ones(len(g["cw"]))
            cs = _as_case(name, g["n"], g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"], x)
            L = R.laplacian(*R.golden_graph(g, x))
        else:      # one edge is the candidate at x = 1, the others are fixed: the last edge off the chain, so that the fixed edges hold
            n, i, j, w = R.small_graphs()[name]      # the whole chain and the handle is chain-like (a pure chain: its last edge)
            q = SMALL[name]
            off = np.nonzero(np.abs(np.asarray(i) - np.asarray(j)) > 1)[0]
            k = int(off[-1]) if len(off) else len(i) - 1
            fx = np.arange(len(i)) != k
            cs = _as_case(name, n, i[fx], j[fx], w[fx], i[k:k + 1], j[k:k + 1], w[k:k + 1], np.ones(1))
            L = R.laplacian(n, i, j, w)
        s = len(LR.closures_of(cs)[0])
        out = Input(name, cs, L, q, s > 0, 16, s)
    _INPUTS[name] = out
    return out


_REF = {}


def reference(name):
    """The undamaged restatement's result on problem(name), computed once."""
    if name not in _REF:
        I = problem(name)
        _REF[name] = lowest_pairs(I.L, I.q, I.exact, lob_chunk=I.lob_chunk)
    return _REF[name]


# ---- what both test files assert of a result ----
def eigsh_lowest(L, q):
    """The q + 1 lowest eigenvalues by shift-invert Lanczos, as lob_restatement.lambda2_reference computes lambda_2."""
    import scipy.sparse.linalg as spla
    shift = 1e-6 * R.lnorm_inf(L)
    w = spla.eigsh((sp.csr_matrix(L) + shift * sp.identity(L.shape[0])).tocsc(), k=q + 1, sigma=0, which="LM", return_eigenvectors=False)
    return np.sort(w) - shift


def assert_values(name, L, lams, V, info, tol=1e-8):
    """assert_pairs up to n = 4 097; above: eigenvalues against eigsh to tol ||L||_inf, the recomputed stop-rule residual,
    orthonormality and orthogonality to the constant vector with assert_pairs' bounds."""
    n, q = V.shape
    if n <= 4097:
        R.assert_pairs(name, L, lams, V, info, tol)
        return
    lnorm = R.lnorm_inf(L)
    ev = eigsh_lowest(L, q)
    assert np.all(info["status"] == R.OK) and np.all(info["residual"] < tol), (name, info)
    for c in range(q):
        assert R.stop_rule_residual(L, lams[c], V[:, c], lnorm) < tol, (name, c)
        assert abs(lams[c] - ev[c + 1]) <= tol * lnorm, (name, c, lams[c], ev[c + 1])
    assert np.all(np.diff(lams) >= 0)
    assert np.abs(V.T @ V - np.eye(q)).max() <= 64 * n * R.EPS
    assert np.abs(V.sum(axis=0)).max() / np.sqrt(n) <= 64 * n * R.EPS
