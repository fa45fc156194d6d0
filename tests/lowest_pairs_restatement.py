"""NumPy restatement of machip_lowest_pairs (mac_amd/csrc/solver_pairs.h): the q lowest non-trivial
eigenpairs of a graph Laplacian by sequential deflation with locking.  Test infrastructure only; independent of oracle/.

Column c runs a plain three-term Lanczos recurrence on L, every new vector projected ONCE against the locked block
Q = [1/sqrt(n), v_0 .. v_{c-1}], the basis kept and never re-orthogonalised against itself.  The host looks at the records a chunk
of steps at a time: smallest Ritz pair (theta, s) of T_J, estimate |s_{J-1}| ||u_J||_1 of the residual's 1-norm (in exact arithmetic
the residual of the Ritz vector IS s_{J-1} u_J).  When the estimate is below a quarter of the tolerance, or the sequence has ended
(breakdown, the complement exhausted, the basis full), the Ritz vector is formed, projected twice, normalised and checked
explicitly: ||L v - rho v||_1 / ||L||_inf < tol.  A sequence that ends without a passing check restarts from its Ritz vector.

The restatement's column 0 is the same iteration with Q = [1/sqrt(n)] alone, or a pair the caller passes in (`col0`): the
library's column 0 is its existing Fiedler solve.
"""
import numpy as np
import scipy.sparse as sp
from scipy.linalg import eigh_tridiagonal

CHUNK = 16            # kPairsChunk: steps between two looks at the records
SLACK = 0.25          # the explicit check is tried once the estimate is below SLACK * tol * ||L||_inf
OK, NOT_CONVERGED = 0, 1


def lnorm_inf(L):
    return float(abs(sp.csr_matrix(L)).sum(axis=1).max())


def reference_block(n, q):
    """RandomState(7).normal(size=(q, n)).T: its first four columns are the reference's start block for every q."""
    return np.asarray(np.random.RandomState(7).normal(size=(q, n))).T


def stop_rule_residual(L, lam, v, lnorm=None):
    lnorm = lnorm_inf(L) if lnorm is None else lnorm
    v = v / np.linalg.norm(v)
    return float(np.abs(L @ v - lam * v).sum() / lnorm)


def _project(x, Q):
    return x - Q @ (Q.T @ x)


def _smallest(alpha, beta):
    """Smallest eigenpair of the tridiagonal (alpha[0..J), beta[1..J))."""
    J = len(alpha)
    if J == 1:
        return float(alpha[0]), np.ones(1)
    w, S = eigh_tridiagonal(alpha, beta[1:J], select="i", select_range=(0, 0))
    return float(w[0]), S[:, 0]


def _column(L, Q, x, tol, lnorm, max_steps, cap, jmax):
    """One deflated column.  Returns (lam, v, residual, steps, restarts, status)."""
    n = L.shape[0]
    tiny = 1e-13 * lnorm
    steps = restarts = 0
    slack = SLACK
    best = None
    while True:
        u = _project(_project(x, Q), Q)
        U = [u]                                   # the basis is kept UNNORMALISED: column j = u_j, v_j = u_j / beta_j
        beta = [float(np.linalg.norm(u))]
        alpha = []
        if not beta[0] > tiny:
            raise ValueError("start vector lies in the locked block")
        ended, J = False, 0
        Jmax = min(cap - 1, jmax)
        while True:
            ch = min(CHUNK, Jmax - J, max_steps - steps)
            for _ in range(ch):
                j = len(alpha)
                inv = 1.0 / beta[j] if beta[j] > tiny else 0.0
                v = U[j] * inv
                t = L @ v
                a = float(t @ v)
                w = t - a * v
                if j > 0 and beta[j - 1] > tiny:
                    w = w - beta[j] * (U[j - 1] / beta[j - 1])
                w = _project(w, Q)                # the NEW vector, not L v alone: what v_j, v_{j-1} carry of Q would grow as (alpha / beta)^j
                alpha.append(a)
                U.append(w)
                beta.append(float(np.linalg.norm(w)))
            steps += ch
            Jn = len(alpha)
            J = Jn
            for jj in range(1, Jn + 1):           # breakdown: the sequence ended at the first negligible beta
                if beta[jj] <= tiny:
                    J, ended = jj, True
                    break
            ended = ended or J >= Jmax or steps >= max_steps
            theta, s = _smallest(np.array(alpha[:J]), np.array(beta[:J + 1]))
            est = abs(s[J - 1]) * float(np.abs(U[J]).sum())
            if not (ended or est < slack * tol * lnorm):
                continue
            y = sum((s[k] / beta[k]) * U[k] for k in range(J))
            y = _project(_project(y, Q), Q)
            y = y / np.linalg.norm(y)
            Ly = L @ y
            rq = float(y @ Ly)
            res = float(np.abs(Ly - rq * y).sum())
            best = (rq, y, res / lnorm)          # the last explicitly checked vector is what a capped column reports
            if res < tol * lnorm:
                return rq, y, res / lnorm, steps, restarts, OK
            if ended:
                break
            slack = min(slack, 0.5 * est / res * slack) if res > 0 else slack     # the estimate was optimistic by res / est
        if steps >= max_steps:
            return best[0], best[1], best[2], steps, restarts, NOT_CONVERGED
        x = y
        restarts += 1


def lowest_pairs(L, q, X0=None, tol=1e-8, max_steps=0, vcap=0, col0=None):
    """(lams, V, info) as mac_amd.utils.fiedler.find_lowest_pairs returns them."""
    L = sp.csr_matrix(L, dtype=np.float64)
    n = L.shape[0]
    assert 1 <= q <= min(16, n - 1)
    lnorm = lnorm_inf(L)
    X0 = reference_block(n, q) if X0 is None else np.asarray(X0, dtype=np.float64)
    max_steps = max_steps if max_steps > 0 else max(2000, 20 * n)
    cap = min(n + 10, 16384) if vcap <= 0 else max(4, vcap)
    Q = np.full((n, 1), 1.0 / np.sqrt(n))
    lams, res, steps, restarts, status = [], [], [], [], []
    for c in range(q):
        if c == 0 and col0 is not None:
            lam, v = float(col0[0]), np.asarray(col0[1], dtype=np.float64)
            out = (lam, v, stop_rule_residual(L, lam, v, lnorm), 0, 0, OK)
        else:
            out = _column(L, Q, X0[:, c], tol, lnorm, max_steps, cap, n - 1 - c)
        lams.append(out[0]); res.append(out[2]); steps.append(out[3]); restarts.append(out[4]); status.append(out[5])
        Q = np.column_stack([Q, out[1]])
    order = np.argsort(np.array(lams), kind="stable")
    first_rank = int(np.sum(np.array(lams) < lams[0] - tol * lnorm))      # ties within the stop rule's resolution count for column 0
    lams = np.array(lams)[order]
    info = {"residual": np.array(res)[order], "steps": np.array(steps)[order], "restarts": np.array(restarts)[order],
            "status": np.array(status)[order], "reordered": int(first_rank != 0), "first_rank": first_rank,
            "gap": float(lams[1] - lams[0]) if q >= 2 else None}
    return lams, Q[:, 1:][:, order], info


# ---- the graphs the host and the GPU tests share: name -> (n, edges i, edges j, weights) ----

def _er(n, seed):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.random((n, n)) < 12.0 / n, 1)
    i, j = np.nonzero(A)
    return n, i, j, 0.5 + rng.random(len(i))


def _petersen():
    i = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    j = [1, 2, 3, 4, 0, 5, 6, 7, 8, 9, 7, 8, 9, 5, 6]
    return 10, np.array(i), np.array(j), np.ones(15)


def mirror_graph():
    """Two identical random clusters joined through a middle vertex with a pendant on it (tests/test_gpu_parity.py,
    test_landscape_start_keeps_a_floor_under_every_entry; same seed): v_2 vanishes exactly where the landscape peaks."""
    rng = np.random.default_rng(5)
    nc = 300
    A = np.triu(rng.random((nc, nc)) < 0.08, 1)
    ai, aj = np.nonzero(A)
    m_, p_ = 2 * nc, 2 * nc + 1
    return (2 * nc + 2, np.concatenate([ai, ai + nc, [0, nc, m_]]), np.concatenate([aj, aj + nc, [m_, m_, p_]]),
            np.concatenate([np.ones(2 * len(ai)), [0.02, 0.02, 0.5]]))


def small_graphs():
    k5 = np.array([(a, b) for a in range(5) for b in range(a + 1, 5)])
    return {
        "k5": (5, k5[:, 0], k5[:, 1], np.ones(10)),
        "petersen": _petersen(),
        "star20": (20, np.zeros(19, dtype=int), np.arange(1, 20), np.ones(19)),
        "c64": (64, np.arange(64), (np.arange(64) + 1) % 64, np.ones(64)),
        "p300": (300, np.arange(299), np.arange(1, 300), np.ones(299)),
        "er257": _er(257, 11),
        "er1000": _er(1000, 12),
    }


def laplacian(n, i, j, w):
    i, j, w = np.asarray(i), np.asarray(j), np.asarray(w, dtype=np.float64)
    W = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    return (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()


def golden_graph(g, x):
    """L(x) of a golden's edge lists: fixed edges plus x_k w_k on the candidates with x_k > 1e-10."""
    keep = np.asarray(x) > 1e-10
    return (int(g["n"]), np.concatenate([g["fi"], g["ci"][keep]]), np.concatenate([g["fj"], g["cj"][keep]]),
            np.concatenate([g["fw"], (np.asarray(x) * g["cw"])[keep]]))


# ---- what both test files assert of a result ----

EPS = 2.0 ** -52
_DENSE = {}


def dense_spectrum(name, L):
    """(ev, E, ||L||_inf) by dense eigh, computed once per graph and shared."""
    if name not in _DENSE:
        ev, E = np.linalg.eigh(sp.csr_matrix(L).toarray())
        _DENSE[name] = (ev, E, lnorm_inf(L))
    return _DENSE[name]


def assert_pairs(name, L, lams, V, info, tol=1e-8):
    """Status and residual (reported and recomputed), eigenvalues rank by rank, order, orthogonality, and the eigenspaces by
    Davis-Kahan with the MEASURED residual: for a column whose cluster (eigenvalues within 1e-6 ||L|| of a neighbour) has
    spectral distance gap to everything outside it, ||(I - E E^T) v||_2 <= residual ||L|| / gap + 64 n eps.  A cluster cut
    by q is checked by eigenvalue and residual only."""
    L = sp.csr_matrix(L)
    n, q = V.shape
    ev, E, lnorm = dense_spectrum(name, L)
    assert ev[1] > 1e-9 * lnorm, (name, "not connected", ev[:3])
    assert np.all(info["status"] == OK), (name, info)
    assert np.all(info["residual"] < tol), (name, info["residual"])
    for c in range(q):
        assert abs(np.linalg.norm(V[:, c]) - 1.0) <= 64 * n * EPS
        r = stop_rule_residual(L, lams[c], V[:, c], lnorm)
        assert r < tol, (name, c, r)
        assert abs(lams[c] - ev[c + 1]) <= tol * lnorm, (name, c, lams[c], ev[c + 1])       # |rho - nearest ev| <= ||r||_2 <= ||r||_1 < tol ||L||
    assert np.all(np.diff(lams) >= 0), (name, lams)
    assert np.abs(V.T @ V - np.eye(q)).max() <= 64 * n * EPS, (name, np.abs(V.T @ V - np.eye(q)).max())
    assert np.abs(V.sum(axis=0)).max() / np.sqrt(n) <= 64 * n * EPS, (name, np.abs(V.sum(axis=0)).max())
    c = 0
    while c < q:
        lo = hi = c + 1                                   # cluster [lo, hi] of eigenvalue indices around column c
        while lo > 1 and ev[lo] - ev[lo - 1] <= 1e-6 * lnorm:
            lo -= 1
        while hi + 1 < n and ev[hi + 1] - ev[hi] <= 1e-6 * lnorm:
            hi += 1
        if hi <= q:                                       # (a cluster cut by q: eigenvalue and residual only)
            gap = min(ev[lo] - ev[lo - 1], ev[hi + 1] - ev[hi] if hi + 1 < n else np.inf)
            Ec = E[:, lo:hi + 1]
            for k in range(lo - 1, hi):
                out = np.linalg.norm(V[:, k] - Ec @ (Ec.T @ V[:, k]))
                assert out <= info["residual"][k] * lnorm / gap + 64 * n * EPS, (name, k, out, info["residual"][k], gap)
        c = hi
