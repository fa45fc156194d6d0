"""NumPy/SciPy restatement of MAC's preconditioned eigen-solver (mac_amd/csrc/solver_lob.h `solve_lob`, precond.h, woodbury.h), written
by reading those headers (for the tests; not a port of any kernel).  It exists to count: everything the suite compares -- lambda_2,
the Fiedler vector, the residual -- is decided by the sparse L(x); the preconditioner only proposes search directions, so a kernel
of it can be subtly wrong with every value right.  What a wrong preconditioner costs is iterations, and `stats.lanczos_steps` of a
solve in mode 6 / 7 is the number of iterations the host had enqueued when the solve ended.

The iteration (`solve`): block-size-1 LOBPCG on span{x, w - mean, p - mean}.
    start: the vector given to set_start, mean removed, normalised; Lx, theta = x.Lx, r = Lx - theta x
    per iteration: w = M^-1 r;  Lw = L w;  the 15 sums xx xw xp ww wp pp | xLx xLw xLp wLw wLp pLp | Sx Sw Sp of the UNCENTRED vectors;
        the 3 x 3 Rayleigh-Ritz of `lob_rayleigh_ritz` (Gram matrix = sums - n mean mean^T, scaled to unit diagonal, factored R^T R;
        `bad` unless q11 = 1 - r01^2 > 1e-14; p dropped unless q22 > 1e-12 and it is not the first iteration since a (re)start;
        smallest eigenpair of R^-T (D A D) R^-1 -- numpy.linalg.eigh here, a Rayleigh-quotient iteration with a Jacobi fall-back on
        the device: the same pair --; coefficients z = D R^-1 y with z0 >= 0);
        p <- z1 (w - mw) + z2 (p - mp),  Lp <- z1 Lw + z2 Lp,  x <- z0 (x - mx) + p,  Lx <- z0 Lx + Lp,  r <- Lx - theta x,
        and the record est_j = ||r_j||_1 of every iterate j.
    host: chunks of iterations; at the end of a chunk the host reads est of that iterate and stops iterating when
        est < tol ||L||_inf (or on `bad`, or at the cap); the forecast `to_go` from the slope of log est over the last <= 48 iterations
        shortens the chunks near the end (`near`) and decides whether a second chunk is already enqueued (`depth`).  Exact
        preconditioner: chunks 2, 4, 4, ... (shortened when near), depth 1.  Tridiagonal one: chunks of `lob_chunk` after a ramp
        4, 8, ...; the tests run it with lob_chunk = 1, one iteration per chunk, depth 2 until near.
        Then the explicit check: x mean-removed and normalised again, a fresh product, res = ||Lx - rq x||_1 / ||L||_inf < tol ends
        the solve; otherwise the recurrence restarts from that x (p = 0) -- at most 12 times.
    The count is `it_enq`, a chunk end: device and restatement are compared chunk end against chunk end.

The preconditioner M^-1 (sigma = 1e-8 ||L||_inf exact, 2.5e-7 ||L||_inf tridiagonal):
    `ExactInverse`   the plain operation the exact mode stands for: (L + sigma I)^-1 r in float64, a dense inverse up to n = 4 097,
                     scipy's sparse LU above (`extended=True`: Gauss-Jordan inverse and product in numpy.longdouble).
    `TriExact`       the tridiagonal of L with the full diagonal, + sigma I, solved by LAPACK's banded solver.
    `Composed`       the device's algebra, one term of which `damage` breaks:  T = L U by the continued fraction
                     u_e = b_e - a_e^2 / u_(e-1), forward and backward substitution, and under the exact preconditioner
                     y = T^-1 r, g = U^T y, h = C^-1 g, w = y - Z h with Z = T^-1 U, C = D^-1 + U^T Z, C^-1 by Gauss-Jordan steps
                     over 32-row pivot blocks of the matrix padded with an identity to whole 64 x 64 tiles (ld).
                     Damages, named after the kernel they mirror (e = c t is the first unknown of thread t, 64 c w of wave w;
                     c = ceil(n / 1024) up to n = 16 384, 4 above):
                         wb_cols_one_endpoint   k_wb_cols / k_wb_big_*: one column of Z built from e_i alone
                         wb_cols_fwd_carry      k_wb_cols / k_wb_big_*: the forward carry lost at one thread border, in every column of Z
                         wb_cols_bwd_carry      k_wb_cols / k_wb_big_*: the backward carry lost at one wave border, in every column of Z
                         wb_cap_no_dinv         k_wb_cap: one 1 / (x_k w_k) left out of C's diagonal
                         wb_extract_no_fixed    k_wb_extract: closures that are fixed off-chain edges left out of U
                         gj_tile_zero           k_gj_step: one off-diagonal 64 x 64 tile of C^-1 zero (ld >= 128)
                         gj_last_step           k_gj_step: the last 32-row pivot step skipped (s > ld - 32: else that block is padding)
                         wb_h_tail              k_wb_h: the entries of h past the last whole 64 dropped (s not a multiple of 64)
                         wb_w_segment           k_wb_w: one 16-row segment of the solver's layout left at y
                         tri_fwd_carry          k_tri_solve / k_lob_fused / k_tri_big_*: the forward carry of y = T^-1 r lost at one thread border
                         tri_bwd_carry          k_tri_solve / k_lob_fused / k_tri_big_*: its backward carry lost at one wave border
                         tri_factor_cut         k_tri_factor / k_tri_factor_big: the pivot recurrence restarted at every wave border
                         tri_diag_swapped       k_tri_band / k_tri_factor: the chain-only diagonal where the full one belongs, and the
                                                full one where the chain-only one belongs (exact preconditioner)
                     and in the iteration itself  rr_w_mean:  k_lob_update / k_lob_fused form p and x from w, not from w - mean(w)
                     (the Gram matrix of lob_rayleigh_ritz still takes the mean out).

Closures are counted as the library counts them (k_wb_extract): one per stored off-band entry of the upper triangle.  The assembly
keeps one entry per ACTIVE candidate (x_k > 1e-10) and one per fixed pair, so a duplicated candidate pair is two closures with the
same end points -- two rank-one terms, the same operator as one closure of the summed weight --, and a candidate at x = 0 is none.

`cases()` lists the inputs, `reference(name)` returns J_ref (the count with the undamaged reference preconditioner), the
per-iterate est, the excess J_variant - J_ref of every applicable damaged variant (inf: the variant ran into its cap
J_ref + max(64, J_ref), was handed to Lanczos, or broke down) and D = the smallest of them (a capped variant counts with the cap's
excess, which can only make D smaller) among the case's `pins`; `table(name)` adds the excess of every other applicable variant.
A case without pins (s = 1: most damages cost 0 to 2 iterations of 6) has no D and is kept as a mode / value case only.
"""
import collections
import functools
import math

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

TOL = 1e-8
LOB_CAP = 100000
X_TOL = 1e-10
WB_DAMAGES = ("wb_cols_one_endpoint", "wb_cols_fwd_carry", "wb_cols_bwd_carry", "wb_cap_no_dinv", "wb_extract_no_fixed", "gj_tile_zero",
              "gj_last_step", "wb_h_tail", "wb_w_segment")
TRI_DAMAGES = ("tri_fwd_carry", "tri_bwd_carry", "tri_factor_cut", "tri_diag_swapped")
RR_DAMAGES = ("rr_w_mean",)
KERNELS = {      # kernel of section 1 of the issue -> the variants that mirror it
    "k_wb_cols / k_wb_big_*": ("wb_cols_one_endpoint", "wb_cols_fwd_carry", "wb_cols_bwd_carry"), "k_wb_cap": ("wb_cap_no_dinv",),
    "k_wb_extract": ("wb_extract_no_fixed",),
    "k_gj_step": ("gj_tile_zero", "gj_last_step"), "k_wb_h": ("wb_h_tail",), "k_wb_w": ("wb_w_segment",),
    "k_tri_solve / k_tri_big_*": ("tri_fwd_carry", "tri_bwd_carry"), "k_tri_factor / k_tri_factor_big": ("tri_factor_cut",),
    "k_tri_band / chain_only": ("tri_diag_swapped",), "k_lob_update / k_lob_fused": ("rr_w_mean",),
}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name n fi fj fw ci cj cw x start exact options pins s note")


def _case(name, n, s, decades, seed, exact=True, options=None, pins=(), kinds=False, note="", cw_decades=1.5, nfixed=0):
    """A chain of n nodes with seeded log-uniform weights over `decades` and s closures (stored off-band entries) of weights over
    `cw_decades`, x in [0.2, 1].  kinds: a closure at node 0 and one at node n - 1, a span-2 closure, `nfixed` fixed off-chain
    edges, a duplicated candidate pair (two closures), five candidates at x = 0 (none)."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = 10.0 ** rng.uniform(0.0, decades, n - 1)
    pairs = set()
    if kinds:
        pairs.update([(0, int(rng.integers(n // 3, n // 2))), (int(rng.integers(n // 2, 2 * n // 3)), n - 1), (n // 4, n // 4 + 2)])
    while len(pairs) < s - (1 if kinds else 0):
        a, b = sorted(int(v) for v in rng.integers(0, n, 2))
        if b - a > 1:
            pairs.add((a, b))
    pairs = sorted(pairs)
    pi = np.array([p[0] for p in pairs]); pj = np.array([p[1] for p in pairs])
    pw = 10.0 ** rng.uniform(0.0, cw_decades, len(pairs))
    x = rng.uniform(0.2, 1.0, len(pairs))
    ci, cj, cw = pi, pj, pw
    if kinds:
        fx = rng.permutation(np.arange(3, len(pairs)))[:nfixed]          # (never one of the three special pairs)
        keep = np.setdiff1d(np.arange(len(pairs)), fx)
        fi = np.append(fi, pi[fx]); fj = np.append(fj, pj[fx]); fw = np.append(fw, pw[fx])
        d = int(keep[len(keep) // 2])                                     # the duplicated pair
        zi = rng.integers(0, n - 3, 5)                                    # candidates at x = 0
        ci = np.concatenate([pi[keep], [pi[d]], zi]); cj = np.concatenate([pj[keep], [pj[d]], zi + 3])
        cw = np.concatenate([pw[keep], 10.0 ** rng.uniform(0.0, cw_decades, 6)])
        x = np.concatenate([x[keep], [rng.uniform(0.2, 1.0)], np.zeros(5)])
        perm = rng.permutation(len(x))
        ci, cj, cw, x = ci[perm], cj[perm], cw[perm], x[perm]
    start = rng.standard_normal(n)
    return Case(name, n, fi.astype(np.int32), fj.astype(np.int32), fw, ci.astype(np.int32), cj.astype(np.int32), cw, x, start, exact,
                dict(options or {}), tuple(pins), s, note)


TRI_OPTS = {"woodbury": 0, "lob_chunk": 1}
_WB = ("wb_cap_no_dinv", "wb_w_segment", "wb_cols_bwd_carry", "tri_bwd_carry", "tri_diag_swapped")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case.  Exact preconditioner: chain weights over 3 decades, the chain lengths at which a kernel changes form and the
    closure counts at which the capacitance matrix gains a tile row.  Tridiagonal: closure-poor, chain weights within half a decade.
    `pins`: the variants the case is there to pin -- D is the smallest excess among them; tests/test_lob_precond_host.py asserts
    D >= 8 and >= 0.1 J_ref for them and prints the excess of every other applicable variant next to them.  A case without pins is
    a mode / value case."""
    out = [
        _case("n257_s63", 257, 63, 3, 11, pins=_WB + ("rr_w_mean", "gj_last_step", "wb_h_tail"),
              note="c = 1, most threads idle; ld 64, both 32-row pivot steps live"),
        _case("n1024_s64", 1024, 64, 3, 12, pins=_WB + ("rr_w_mean", "tri_factor_cut", "gj_last_step"), note="c = 1, every thread busy; ld 64 full"),
        _case("n1025_s65_kinds", 1025, 65, 3, 13, kinds=True, nfixed=24,
              pins=_WB + ("rr_w_mean", "tri_factor_cut", "gj_tile_zero", "wb_h_tail", "wb_extract_no_fixed"), note="c = 2; ld 128; every closure kind"),
        _case("n4096_s129", 4096, 129, 3, 14, pins=_WB + ("rr_w_mean", "tri_factor_cut", "gj_tile_zero"), note="c = 4: k_lob_fused; ld 192"),
        _case("n4097_s65", 4097, 65, 3, 15, pins=_WB + ("rr_w_mean", "tri_factor_cut", "gj_tile_zero", "wb_h_tail"),
              note="c = 5: three separate kernels; ld 128"),
        _case("n16384_s65", 16384, 65, 3, 16, pins=_WB + ("tri_factor_cut", "gj_tile_zero", "wb_h_tail"), note="c = 16, the last single-workgroup size"),
        _case("n16385_s129", 16385, 129, 3, 17, pins=_WB + ("tri_factor_cut", "gj_tile_zero"), note="k_tri_*_big / k_wb_big_*; ld 192"),
        _case("n257_s1", 257, 1, 3, 18, note="s = 1: no off-diagonal tile; most damages cost 0-2 iterations of 6 -- mode / value only"),
        _case("n300_s64_tier", 300, 64, 3, 19, options={"wb_max": 64}, note="wb_max = 64, s = 64: the exact preconditioner, built at once"),
        _case("n300_s65_tier", 300, 65, 0.5, 20, exact=False, options={"wb_max": 64},
              note="wb_max = 64, s = 65: the tridiagonal preconditioner first, and it converges (many closures: no pin)"),
        _case("n300_s65_off", 300, 65, 0.5, 20, exact=False, options={"woodbury": 0}, note="woodbury = 0 (many closures: no pin)"),
        _case("tri_n300_s30", 300, 30, 0.5, 22, exact=False, options=TRI_OPTS, cw_decades=0.5,
              pins=("tri_fwd_carry", "tri_bwd_carry", "tri_diag_swapped", "rr_w_mean"), note="tridiagonal, c = 1"),
        _case("tri_n2000_s30", 2000, 30, 0.5, 22, exact=False, options=TRI_OPTS,
              pins=("tri_bwd_carry", "tri_factor_cut", "tri_diag_swapped", "rr_w_mean"), note="tridiagonal, c = 2"),
        _case("tri_n16385_s30", 16385, 30, 0.5, 21, exact=False, options=TRI_OPTS,
              pins=TRI_DAMAGES + RR_DAMAGES, note="tridiagonal, k_tri_factor_big / k_tri_big_*"),
    ]
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def golden_cases():
    """Inputs of tests/test_gpu_parity.py that are pinned too: intel with its first 1 000 (of 785: all) candidates active, every third
    at 0.37, from the reference's start vector -- test_exact_chain_plus_closures_preconditioner."""
    import os
    from mac_amd.utils.fiedler import reference_start_block
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2o_intel.npz"), allow_pickle=False))
    n = int(g["n"])
    x = np.zeros(len(g["cw"])); x[: min(len(x), 1000)] = 1.0
    x[::3] *= 0.37
    intel = Case("intel_1000", n, g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"], x, reference_start_block(n)[:, 0].copy(), True, {},
                 _WB + ("tri_factor_cut", "gj_tile_zero", "wb_h_tail"), 785, "intel.g2o: n = 1 728, c = 2, ld 832")
    return {intel.name: intel}


def case(name):
    return cases()[name] if name in cases() else golden_cases()[name]


PAIRS = {      # option pairs that must agree on one input (tests/test_lob_precond_gpu.py)
    "lob_fuse": [("n4096_s129", {"lob_fuse": 0})],
    "gj_look_min": [("n1024_s64", {"gj_look_min": 64}), ("n1025_s65_kinds", {"gj_look_min": 64}), ("n4096_s129", {"gj_look_min": 64})],
}


def closures_of(case):
    """(ui, uj, uc, fixed) in the order k_wb_extract lists them: by row, then column, a fixed entry before the candidates' (by index)."""
    rows = []
    acc = {}
    for a, b, w in zip(case.fi, case.fj, case.fw):
        a, b = (int(a), int(b)) if a < b else (int(b), int(a))
        if b - a > 1:
            acc[(a, b)] = acc.get((a, b), 0.0) + float(w)
    rows += [(a, b, -1, w, True) for (a, b), w in acc.items()]
    for k, (a, b, w, xk) in enumerate(zip(case.ci, case.cj, case.cw, case.x)):
        a, b = (int(a), int(b)) if a < b else (int(b), int(a))
        if xk > X_TOL and b - a > 1:
            rows.append((a, b, k, float(xk) * float(w), False))
    rows.sort(key=lambda r: r[:3])
    return (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64),
            np.array([r[3] for r in rows]), np.array([r[4] for r in rows], dtype=bool))


def laplacian(case):
    n = case.n
    act = case.x > X_TOL
    i = np.concatenate([case.fi, case.ci[act]]).astype(np.int64); j = np.concatenate([case.fj, case.cj[act]]).astype(np.int64)
    w = np.concatenate([case.fw, (case.x * case.cw)[act]])
    keep = i != j
    i, j, w = i[keep], j[keep], w[keep]
    A = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    return (sp.diags(np.asarray(A.sum(axis=1)).ravel()) - A).tocsr()


def norm_inf(L):
    return float(abs(L).sum(axis=1).max())


def layout_c(n):
    return 4 if n > 16384 else (n + 1023) // 1024


# ---- preconditioners ------------------------------------------------------------------------------------------------------------
def _inverse_extended(A):
    """Gauss-Jordan inverse of a symmetric positive definite matrix in numpy.longdouble (no pivoting needed)."""
    A = np.array(A, dtype=np.longdouble)
    k = A.shape[0]
    inv = np.eye(k, dtype=np.longdouble)
    for p in range(k):
        d = A[p, p]
        A[p] /= d
        inv[p] /= d
        f = A[:, p].copy()
        f[p] = 0.0
        inv -= f[:, None] * inv[p][None, :]
        A -= f[:, None] * A[p][None, :]
    return inv


class ExactInverse:
    def __init__(self, L, sigma, extended=False):
        n = L.shape[0]
        M = (L + sigma * sp.identity(n)).tocsc()
        if extended:
            inv = _inverse_extended(M.toarray())
            self.apply = lambda r: (inv @ r.astype(np.longdouble)).astype(np.float64)
        elif n <= 4097:
            inv = np.linalg.inv(M.toarray())
            self.apply = lambda r: inv @ r
        else:
            self.apply = spla.splu(M).solve


class TriExact:
    def __init__(self, L, sigma):
        n = L.shape[0]
        ab = np.zeros((3, n))
        ab[1] = L.diagonal() + sigma
        off = L.diagonal(1)
        ab[0, 1:] = off; ab[2, :-1] = off
        self.apply = lambda r: sla.solve_banded((1, 1), ab, r)


def gj_inverse(C, ld, skip_last=False):
    """C^-1 by in-place Gauss-Jordan steps over 32-row pivot blocks of C padded with an identity to ld x ld (woodbury.h)."""
    s = C.shape[0]
    A = np.eye(ld)
    A[:s, :s] = C
    for kb in range(0, ld, 32):
        if skip_last and kb == ld - 32:
            break
        K = slice(kb, kb + 32)
        P = np.linalg.inv(A[K, K])
        AiK, AKj = A[:, K].copy(), A[K, :].copy()
        A = A - AiK @ P @ AKj
        A[:, K] = -AiK @ P
        A[K, :] = P @ AKj
        A[K, K] = P
    return A[:s, :s]


def tri_solver(n, a, b, damage=None):
    """T = tridiag(a, b, a) = L U by the continued fraction, and the solve: forward sweep y_e = r_e - l_e y_(e-1), backward sweep
    x_e = y_e / u_e - cu_e x_(e+1) (LAPACK's banded solver on the two bidiagonal factors).  damage: one of the tri_* terms."""
    c = layout_c(n)
    t_mid = ((n + c - 1) // c) // 2 | 1                     # a thread in the middle that is not the first of its wave
    w_mid = max(1, ((n - 1) // (64 * c)) // 2)              # a wave in the middle (wave 1 where there are only two or three)
    assert t_mid % 64 and c * t_mid < n and 64 * c * w_mid < n
    cut = set(range(64 * c, n, 64 * c)) if damage == "tri_factor_cut" else ()
    l = np.zeros(n); dinv = np.zeros(n)
    rinv = 0.0
    for e in range(n):
        if e in cut:
            rinv = 0.0
        l[e] = a[e] * rinv
        u = b[e] - a[e] * a[e] * rinv
        assert u > 0.0
        rinv = 1.0 / u
        dinv[e] = rinv
    cu = np.append(a[1:], 0.0) * dinv
    if damage == "tri_fwd_carry":
        l[c * t_mid] = 0.0
    if damage == "tri_bwd_carry":
        cu[64 * c * w_mid - 1] = 0.0
    fab = np.ones((2, n)); fab[1, :-1] = l[1:]
    bab = np.ones((2, n)); bab[0, 1:] = cu[:-1]
    return lambda r: sla.solve_banded((0, 1), bab, (sla.solve_banded((1, 0), fab, r).T * dinv).T)


class Composed:
    """The device's algebra (exact=True: chain-only T + Woodbury correction; False: the tridiagonal of L alone); `damage` breaks one
    term.  Under the exact preconditioner tri_fwd_carry / tri_bwd_carry hit the solve of the application (k_tri_solve, k_lob_fused,
    k_tri_big_*) and wb_cols_fwd_carry / wb_cols_bwd_carry the column solves (k_wb_cols, k_wb_big_*); the factor serves both."""

    def __init__(self, case, L, sigma, exact, damage=None):
        assert damage is None or damage in WB_DAMAGES + TRI_DAMAGES
        n = self.n = case.n
        c = layout_c(n)
        a = np.zeros(n); a[1:] = L.diagonal(-1)                 # a_e = L[e, e-1]
        chain_only = exact != (damage == "tri_diag_swapped")
        b = (-(a + np.append(a[1:], 0.0)) if chain_only else L.diagonal()) + sigma
        fdam = damage if damage == "tri_factor_cut" else None
        self.tsolve = tri_solver(n, a, b, damage if damage in ("tri_fwd_carry", "tri_bwd_carry") else fdam)
        zsolve = tri_solver(n, a, b, {"wb_cols_fwd_carry": "tri_fwd_carry", "wb_cols_bwd_carry": "tri_bwd_carry"}.get(damage, fdam))
        self.s = 0
        if not exact:
            self.apply = self.tsolve
            return
        ui, uj, uc, fixed = closures_of(case)
        if damage == "wb_extract_no_fixed":
            assert fixed.any()
            ui, uj, uc = ui[~fixed], uj[~fixed], uc[~fixed]
        s = self.s = len(ui)
        ld = (s + 63) // 64 * 64
        U = np.zeros((n, s))
        U[ui, np.arange(s)] = 1.0
        U[uj, np.arange(s)] -= 1.0
        rhs = U.copy()
        if damage == "wb_cols_one_endpoint":
            rhs[uj[s // 2], s // 2] = 0.0
        Z = zsolve(rhs)
        Cm = U.T @ Z
        dd = 1.0 / uc
        if damage == "wb_cap_no_dinv":
            dd[s // 3] = 0.0
        Cm[np.arange(s), np.arange(s)] += dd
        if damage == "gj_last_step":
            assert s > ld - 32
        Ci = gj_inverse(Cm, ld, skip_last=damage == "gj_last_step")
        if damage == "gj_tile_zero":
            assert ld >= 128
            Ci = Ci.copy(); Ci[64:128, 0:64] = 0.0
        seg = None
        if damage == "wb_w_segment":          # 16 consecutive rows of the chunk-transposed layout: unknowns (t0 + q) c, q < 16
            t0 = (((n + c - 1) // c) // 2) // 16 * 16
            seg = (t0 + np.arange(16)) * c
            assert seg.max() < n
        tail = s // 64 * 64
        if damage == "wb_h_tail":
            assert tail < s

        def apply(r):
            y = self.tsolve(r)
            h = Ci @ (y[ui] - y[uj])
            if damage == "wb_h_tail":
                h[tail:] = 0.0
            w = y - Z @ h
            if seg is not None:
                w[seg] = y[seg]
            return w
        self.apply = apply


# ---- the iteration --------------------------------------------------------------------------------------------------------------
def rayleigh_ritz(s, n, havep):
    """lob_rayleigh_ritz: (z0, z1, z2, theta, mx, mw, mp, bad)."""
    dn = float(n)
    mx, mw, mp = s[12] / dn, s[13] / dn, s[14] / dn
    G00, G01, G02 = s[0] - dn * mx * mx, s[1] - dn * mx * mw, s[2] - dn * mx * mp
    G11, G12, G22 = s[3] - dn * mw * mw, s[4] - dn * mw * mp, s[5] - dn * mp * mp
    z0 = 1.0 / math.sqrt(G00) if G00 > 0.0 else 0.0
    theta = s[6] / G00 if G00 > 0.0 else 0.0
    if not G00 > 0.0 or not G11 > 0.0:
        return z0, 0.0, 0.0, theta, mx, mw, mp, True
    k3 = havep and G22 > 0.0
    d = np.array([1.0 / math.sqrt(G00), 1.0 / math.sqrt(G11), 1.0 / math.sqrt(G22) if k3 else 0.0])
    r01, r02, g12 = G01 * d[0] * d[1], G02 * d[0] * d[2], G12 * d[1] * d[2]
    q11 = 1.0 - r01 * r01
    if not q11 > 1e-14:
        return z0, 0.0, 0.0, theta, mx, mw, mp, True
    ir11 = 1.0 / math.sqrt(q11)
    r12 = (g12 - r01 * r02) * ir11
    q22 = 1.0 - r02 * r02 - r12 * r12
    if k3 and not q22 > 1e-12:
        k3 = False
    ir22 = 1.0 / math.sqrt(q22) if k3 else 0.0
    i01 = -r01 * ir11
    i12 = -r12 * ir11 * ir22 if k3 else 0.0
    i02 = -(r01 * i12 + r02 * ir22) if k3 else 0.0
    Ri = np.array([[1.0, i01, i02], [0.0, ir11, i12], [0.0, 0.0, ir22]])
    As = np.array([[s[6], s[7], s[8]], [s[7], s[9], s[10]], [s[8], s[10], s[11]]]) * np.outer(d, d)
    k = 3 if k3 else 2
    Cm = (Ri.T @ As @ Ri)[:k, :k]
    val, vec = np.linalg.eigh((Cm + Cm.T) / 2)
    y = np.zeros(3); y[:k] = vec[:, 0]
    z = d * (Ri @ y)
    if z[0] < 0.0:
        z = -z
    if not np.all(np.isfinite(z)):
        return z0, 0.0, 0.0, theta, mx, mw, mp, True
    return z[0], z[1], z[2] if k3 else 0.0, float(val[0]), mx, mw, mp, False


class _Recurrence:
    def __init__(self, L, apply, w_mean, rng, apply_noise):
        self.L, self.apply, self.w_mean, self.rng, self.apply_noise = L, apply, w_mean, rng, apply_noise
        self.n = L.shape[0]

    def start(self, x, Lx, rq):
        self.x, self.Lx, self.p, self.Lp = x.copy(), Lx.copy(), np.zeros(self.n), np.zeros(self.n)
        self.theta, self.havep, self.bad = rq, False, False
        self.r = Lx - rq * x
        return float(np.abs(self.r).sum())

    def step(self):
        x, p, Lx, Lp = self.x, self.p, self.Lx, self.Lp
        w = self.apply(self.r)
        if self.apply_noise:
            w = w * (1.0 + self.apply_noise * self.rng.standard_normal(self.n))
        Lw = self.L @ w
        s = [x @ x, x @ w, x @ p, w @ w, w @ p, p @ p, x @ Lx, x @ Lw, x @ Lp, w @ Lw, w @ Lp, p @ Lp, x.sum(), w.sum(), p.sum()]
        z0, z1, z2, th, mx, mw, mp, bad = rayleigh_ritz(s, self.n, self.havep)
        self.bad = self.bad or bad
        if not self.w_mean:          # rr_w_mean: the update forgets the subtraction; the Gram matrix (lob_rayleigh_ritz) is intact
            mw = 0.0
        self.p = z1 * (w - mw) + z2 * (p - mp)
        self.Lp = z1 * Lw + z2 * Lp
        self.x = z0 * (x - mx) + self.p
        self.Lx = z0 * Lx + self.Lp
        self.theta, self.havep = th, True
        self.r = self.Lx - th * self.x
        return float(np.abs(self.r).sum())


def _check(L, v):
    y = v - v.mean()
    with np.errstate(invalid="ignore", divide="ignore"):          # (a damaged variant can break down: rq is NaN then, as on the device)
        y = y / np.linalg.norm(y)
    Ly = L @ y
    rq = float(y @ Ly)
    return y, Ly, rq, float(np.abs(Ly - rq * y).sum())


def solve(L, apply, start, wb, lob_chunk=16, tol=TOL, cap=LOB_CAP, w_mean=True, apply_noise=0.0, start_noise=0.0, seed=0):
    """solve_lob.  Returns iters (= it_enq), restarts, lam, res, est (the record of every iterate), converged."""
    rng = np.random.default_rng(seed)
    scale = norm_inf(L)
    v = np.asarray(start, dtype=np.float64)
    if start_noise:
        v = v + start_noise * np.linalg.norm(v) / math.sqrt(len(v)) * rng.standard_normal(len(v))
    y, Ly, rq, r1 = _check(L, v)
    out = dict(iters=0, restarts=0, lam=rq, res=r1 / scale, est=[r1], converged=True)
    if out["res"] < tol:
        return out
    cap = min(LOB_CAP, cap)
    chunk0 = 4 if wb else min(32, max(1, lob_chunk))
    ltarget = math.log(max(tol * scale, 1e-300))
    dev = _Recurrence(L, apply, w_mean, rng, apply_noise)
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
        y, Ly, rq, r1 = _check(L, dev.x)
        out.update(iters=it_enq, restarts=restarts, lam=rq, res=r1 / scale, est=[est_of[j] for j in range(it_enq + 1)])
        if not rq == rq:
            out["converged"] = False
            return out
        if out["res"] < tol:
            return out
        restarts += 1
        if it_enq >= cap or restarts > 12:
            out["converged"] = False
            return out


# ---- references -----------------------------------------------------------------------------------------------------------------
def sigma_of(case, L):
    return (1e-8 if case.exact else 2.5e-7) * norm_inf(L)


def applicable(case):
    """The variants whose term exists on this input."""
    if not case.exact:
        return TRI_DAMAGES + RR_DAMAGES
    s = len(closures_of(case)[0])
    ld = (s + 63) // 64 * 64
    out = ["wb_cols_one_endpoint", "wb_cols_fwd_carry", "wb_cols_bwd_carry", "wb_cap_no_dinv", "wb_w_segment",
           "tri_fwd_carry", "tri_bwd_carry", "tri_factor_cut", "tri_diag_swapped", "rr_w_mean"]
    if closures_of(case)[3].any():
        out.append("wb_extract_no_fixed")
    if ld >= 128:
        out.append("gj_tile_zero")
    if s > ld - 32:
        out.append("gj_last_step")
    if s % 64:
        out.append("wb_h_tail")
    return tuple(out)


def run(case, M=None, damage=None, **kw):
    """One solve of `case`: M = None -> the reference preconditioner, or the device's algebra with `damage`."""
    L = laplacian(case)
    sg = sigma_of(case, L)
    w_mean = damage != "rr_w_mean"
    if M is None:
        if damage is None or damage in RR_DAMAGES:
            M = ExactInverse(L, sg) if case.exact else TriExact(L, sg)
        else:
            M = Composed(case, L, sg, case.exact, damage)
    return solve(L, M.apply, case.start, case.exact, lob_chunk=case.options.get("lob_chunk", 16), w_mean=w_mean, **kw)


def _excess(case, J, variants):
    extra = max(64, J)
    out = {}
    for d in variants:
        r = run(case, damage=d, cap=J + extra)
        out[d] = float(r["iters"] - J) if r["converged"] else math.inf
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """J_ref, est, restarts, lam, res, s of the undamaged reference run; excess of the case's pins and D, their smallest (None: no pins)."""
    case_ = case(name)
    ref = run(case_)
    assert ref["converged"]
    J = ref["iters"]
    out = dict(J_ref=J, est=np.array(ref["est"]), restarts=ref["restarts"], lam=ref["lam"], res=ref["res"], s=len(closures_of(case_)[0]),
               excess={}, D=None)
    if case_.pins:
        assert set(case_.pins) <= set(applicable(case_))
        out["excess"] = _excess(case_, J, case_.pins)
        out["D"] = float(min(min(out["excess"].values()), max(64, J)))
    return out


@functools.lru_cache(maxsize=None)
def table(name):
    """variant -> excess for every applicable variant of the case (the pins among them)."""
    case_, ref = case(name), reference(name)
    out = dict(ref["excess"])
    out.update(_excess(case_, ref["J_ref"], [d for d in applicable(case_) if d not in out]))
    return out


def lambda2_reference(case):
    """lambda_2 by a dense eigh (n <= 4 097) or scipy's shift-invert Lanczos (above)."""
    L = laplacian(case)
    if case.n <= 4097:
        return float(sla.eigh(L.toarray(), eigvals_only=True, subset_by_index=[1, 1])[0])
    shift = 1e-6 * norm_inf(L)
    w = spla.eigsh((L + shift * sp.identity(case.n)).tocsc(), k=2, sigma=0, which="LM", return_eigenvectors=False)
    return float(np.sort(w)[1] - shift)
