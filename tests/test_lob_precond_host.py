"""The inputs of tests/test_lob_precond_gpu.py discriminate: on each pinned input, breaking one term of MAC's chain / Woodbury
preconditioner costs iterations far beyond what rounding can move -- shown here without a GPU, on the NumPy restatement
(tests/lob_restatement.py), so that the device test cannot pass by accident.  A seed that loses a condition fails here.

Per pinned case:  J_ref = the iterations (the host's enqueued count at the end of the solve) of the restatement with the reference
preconditioner -- a float64 inverse of L + sigma I, or LAPACK's banded solve of tridiag(L) + sigma I --;  D = the smallest excess
J_variant - J_ref among the case's pins, the damaged variants it is there to pin (a variant that runs into its cap
J_ref + max(64, J_ref), breaks down or is handed to Lanczos counts as infinite -- as max(64, J_ref) for D).  Asserted:
    D >= 8 and D >= 0.1 J_ref                                          (measured: 20 at the least, 0.21 J_ref at the least)
    restarts == 0 in the reference run
    |J_noise - J_ref| <= D / 8 with every application perturbed by 1e-13 relative and the start by 1e-9   (measured: 0 everywhere)
    the same for the device's own algebra with no term broken (continued-fraction LU, Woodbury correction, blocked Gauss-Jordan
    inverse): it is the same operator                                   (measured: 0 everywhere)
    the same for a numpy.longdouble inverse and application on the smallest input
    every kernel of the path has a pin of its own in at least one case.

What the counts cannot see, and the table printed here shows next to the pins (excess in iterations):
    one column of Z built from e_i alone: -2 .. 8, whichever column.  T^-1 e_j is a constant vector 1 / (n sigma) plus a term of the size of the
        column itself; the constant leaves with the mean of w, the rest is a rank-one error that costs the iteration a step or two.
        k_wb_cols / k_wb_big_* are pinned through their lost backward carry instead, which every column feels.
    a forward carry lost at one thread border: -3 .. 12 under the exact preconditioner, in the application or in the columns of Z (the partial sum that goes missing comes
        back as a constant from the backward sweep, 1 / sigma times it, and leaves with the mean); visible only on the closure-poor
        tridiagonal inputs n = 300 and n = 16 385.
    the mean of w left in by the update: 0 to 2 on n = 16 384, 16 385 and intel (under the exact preconditioner w has no mean
        to speak of: 1^T (L + sigma I)^-1 r = 1^T r / sigma); pinned on the other inputs.
    s = 1: most damages cost 0 to 2 iterations of 6 (the columns, the carries, the diagonal).  n257_s1 is a mode / value case, and so are the tier cases; a tridiagonal
        case with many closures would be one too (the closures, not T, decide the count there) and none is pinned.
Under the tridiagonal preconditioner the count itself is erratic from seed to seed (40 to 245 iterations at n = 300, a damaged
variant 48 iterations FASTER on one seed): the three pinned inputs are seeds on which the pins cost 36 iterations or more."""
import numpy as np
import pytest

import lob_restatement as Q

PINNED = [name for name, c in Q.cases().items() if c.pins] + list(Q.golden_cases())


def test_case_list_covers_the_shapes_and_closure_kinds():
    cs = Q.cases()
    ns = {c.n for c in cs.values() if c.exact}
    assert {257, 1024, 1025, 4096, 4097, 16384, 16385} <= ns
    assert {Q.reference(n)["s"] for n in PINNED if n in cs and cs[n].exact} == {63, 64, 65, 129} and Q.reference("n257_s1")["s"] == 1
    assert {c.n for c in cs.values() if c.pins and not c.exact} == {300, 2000, 16385}
    k = cs["n1025_s65_kinds"]
    ui, uj, uc, fixed = Q.closures_of(k)
    assert ui.min() == 0 and uj.max() == k.n - 1 and np.any(uj - ui == 2) and fixed.sum() == 24
    assert np.sum(k.x == 0.0) == 5                                              # candidates at x = 0: no closure
    pairs = list(zip(ui.tolist(), uj.tolist()))
    assert len(pairs) == 65 and len(set(pairs)) == 64                           # the duplicated pair: two closures, the same end points
    for c in cs.values():
        s = len(Q.closures_of(c)[0])
        assert s == c.s and (s + 63) // 64 * 64 == {1: 64, 20: 64, 30: 64, 63: 64, 64: 64, 65: 128, 129: 192}[s]
    assert cs["n300_s64_tier"].options == {"wb_max": 64} and int((cs["n300_s64_tier"].x > Q.X_TOL).sum()) == 64
    assert cs["n300_s65_tier"].options == {"wb_max": 64} and int((cs["n300_s65_tier"].x > Q.X_TOL).sum()) == 65


@pytest.mark.parametrize("name", PINNED)
def test_every_pin_costs_iterations_and_noise_costs_none(name):
    case, ref = Q.case(name), Q.reference(name)
    tab = Q.table(name)
    print(f"{name} ({case.note}): J_ref {ref['J_ref']}, s {ref['s']}, D {ref['D']}")
    for d, ex in tab.items():
        print(f"    {'pin ' if d in case.pins else '    '}{d:22s} {ex}")
    assert ref["restarts"] == 0 and ref["res"] < Q.TOL
    assert ref["D"] >= 8 and ref["D"] >= 0.1 * ref["J_ref"]
    L = Q.laplacian(case)
    runs = {"noise": Q.run(case, apply_noise=1e-13, start_noise=1e-9, seed=1),
            "device's algebra": Q.run(case, M=Q.Composed(case, L, Q.sigma_of(case, L), case.exact))}
    if case.n == min(c.n for c in Q.cases().values()) and case.exact:
        runs["longdouble"] = Q.run(case, M=Q.ExactInverse(L, Q.sigma_of(case, L), extended=True))
    for tag, r in runs.items():
        print(f"    {tag}: deviation {r['iters'] - ref['J_ref']}, D / 8 {ref['D'] / 8}")
        assert r["converged"] and r["restarts"] == 0 and abs(r["iters"] - ref["J_ref"]) <= ref["D"] / 8


def test_every_kernel_has_a_pin_of_its_own():
    pinned_by = {k: [] for k in Q.KERNELS}
    for name in PINNED:
        ref = Q.reference(name)
        for k, variants in Q.KERNELS.items():
            for d in variants:
                if d in ref["excess"]:
                    assert ref["excess"][d] >= max(8, 0.1 * ref["J_ref"])
                    pinned_by[k].append((name, d, ref["excess"][d]))
    print("kernel: (case, variant, excess)")
    for k, got in pinned_by.items():
        print(f"    {k}: {got}")
        assert got, k
    cs = {n: Q.case(n) for n in PINNED}
    big = [n for n, d, _ in pinned_by["k_wb_cols / k_wb_big_*"] if cs[n].n > 16384]
    assert big                                                                   # k_wb_big_* itself, not only k_wb_cols<C>
    assert any(cs[n].n > 16384 and not cs[n].exact for n, d, _ in pinned_by["k_tri_solve / k_tri_big_*"])
    assert any(cs[n].n > 16384 for n, d, _ in pinned_by["k_tri_factor / k_tri_factor_big"])
    assert {d for n, d, _ in pinned_by["k_gj_step"]} == {"gj_tile_zero", "gj_last_step"}
    fused = [n for n, d, _ in pinned_by["k_lob_update / k_lob_fused"] if cs[n].exact and Q.layout_c(cs[n].n) <= 4]
    assert fused and any(Q.layout_c(cs[n].n) > 4 for n, d, _ in pinned_by["k_lob_update / k_lob_fused"])


def test_mode_value_cases_are_what_they_are_meant_to_be():
    """s = 1 cannot be pinned: the restatement's own table says so.  The tier cases converge under the tridiagonal preconditioner
    long before the solve would escalate (1 500 iterations)."""
    case = Q.cases()["n257_s1"]
    J = Q.reference("n257_s1")["J_ref"]
    ex = Q._excess(case, J, Q.applicable(case))
    print("n257_s1: J_ref", J, ex)
    assert not case.pins and min(ex.values()) < 8
    for name in ("n300_s65_tier", "n300_s65_off"):
        assert Q.reference(name)["J_ref"] < 1500 and Q.reference(name)["restarts"] == 0


def test_blocked_gauss_jordan_and_extended_inverse_are_inverses():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((129, 129))
    A = B @ B.T + 129 * np.eye(129)
    assert np.max(np.abs(Q.gj_inverse(A, 192) @ A - np.eye(129))) < 1e-12
    assert np.max(np.abs(Q._inverse_extended(A).astype(np.float64) @ A - np.eye(129))) < 1e-13


def test_rayleigh_ritz_restatement_finds_the_smallest_pair_of_the_pencil():
    rng = np.random.default_rng(1)
    n = 40
    B = rng.standard_normal((n, n)); B -= B.mean(axis=0); A = B @ B.T          # A 1 = 0, as L 1 = 0
    V = rng.standard_normal((n, 3))
    x, w, p = V.T
    s = [x @ x, x @ w, x @ p, w @ w, w @ p, p @ p, x @ A @ x, x @ A @ w, x @ A @ p, w @ A @ w, w @ A @ p, p @ A @ p, x.sum(), w.sum(), p.sum()]
    z0, z1, z2, th, mx, mw, mp, bad = Q.rayleigh_ritz(s, n, True)
    Vc = V - V.mean(axis=0)
    import scipy.linalg as sla
    val, vec = sla.eigh(V.T @ A @ V, Vc.T @ Vc)          # (the sums hold A-products of the uncentred vectors: the same numbers)
    assert not bad and abs(th - val[0]) <= 1e-12 * abs(val[0])
    y = Vc @ np.array([z0, z1, z2])
    assert abs(np.linalg.norm(y) - 1.0) < 1e-12 and z0 >= 0.0
