"""The inputs of tests/test_eig_precond_gpu.py discriminate: on each of them, breaking any one term of GreedyEig's preconditioner
costs operator applications far beyond what rounding can move -- shown here without a GPU, on the NumPy restatement
(tests/eig_lobpcg_restatement.py), so that the device test cannot pass by accident.

Per input and per pick (or exchange round) k:  A_ref[k] = the applications of the restatement with the exact preconditioner (a
float64 inverse of every column's own reduced Laplacian);  D[k] = the smallest excess over A_ref[k] of any damaged variant that can
differ at k (no_cand everywhere; no_pending where columns are pending; no_fold / fold_tail from the first fold on; in the exchange
also removal_as_addition and no_trial_column; a variant that runs into the 500-iteration cap counts as infinite -- the suite sees
MACHIP_NOT_CONVERGED already).  Asserted, as conditions on the inputs (a seed that loses one fails here):
    D[k] >= 0.05 A_ref[k]                                                  (measured: 0.092 at the least)
    |A_noise[k] - A_ref[k]| <= D[k] / 20, the application perturbed by 1e-13 relative and every start vector by 1e-9
                                                                            (measured: 3 applications at the most, D / 20 >= 12.75)
    the same for a numpy.longdouble inverse and application on the smallest input (the exchange's; measured: 0 of D / 20 = 41)
    the device's algebra with no term broken stays inside D / 20 as well (it is the same operator), padding rows carried or not
    batch 64 and the exchange round: every prune decision is at least 100 tol away from flipping (tol = 1e-8 + 2e-8 ||L||_inf,
    the neighbouring tests' allowance for a device value), so the set of solved columns is pinned."""
import numpy as np
import pytest

import eig_lobpcg_restatement as Q


def _show(tag, ref, noise=None):
    print(tag, "A_ref", ref["A"].astype(int).tolist(), "D", ref["D"].tolist())
    for d, ex in ref["excess"].items():
        print("   ", d, ex.tolist())
    if noise is not None:
        print("    noise", noise.tolist())


@pytest.mark.parametrize("name,fold,batch", Q.GREEDY_CASES)
def test_every_broken_term_costs_at_least_a_twentieth_of_the_exact_count(name, fold, batch):
    ref = Q.greedy_reference(name, fold, batch)
    _show(f"{name} fold {fold} batch {batch}:", ref)
    assert len(ref["D"]) == Q.K_PICKS and np.all(ref["D"] >= 0.05 * ref["A"])
    picks = ref["run"]["order"]
    assert len(set(picks.tolist())) == Q.K_PICKS
    if batch == 512:
        assert np.array_equal(ref["run"]["solved"], len(Q.graph(name)[6]) - np.arange(Q.K_PICKS))      # one batch: every unselected candidate
    # the variants that are active: each of them somewhere, all of them for fold = 3
    assert "no_cand" in ref["excess"] and (fold != 3 or set(ref["excess"]) == {"no_cand", "no_pending", "no_fold", "fold_tail"})


@pytest.mark.parametrize("name,batch", sorted({(n, b) for n, f, b in Q.GREEDY_CASES}))
def test_rounding_size_noise_moves_the_counts_by_far_less(name, batch):
    g = Q.graph(name)
    A = Q.greedy_exact(name, batch)["applications"]
    noisy = Q.select(g, Q.K_PICKS, batch=batch, apply_noise=1e-13, start_noise=1e-9, seed=1)
    composed = Q.select(g, Q.K_PICKS, batch=batch, M=Q.Composed(3))
    padded = Q.select(g, Q.K_PICKS, batch=batch, M=Q.Composed(3, "pad_rows"))
    D = np.min([Q.greedy_reference(n, f, b)["D"] for n, f, b in Q.GREEDY_CASES if (n, b) == (name, batch)], axis=0)
    for tag, r in (("noise", noisy), ("device's algebra", composed), ("padding rows carried", padded)):
        dev = r["applications"] - A
        print(f"{name} batch {batch} {tag}: deviation {dev.tolist()}, D / 20 {(D / 20).tolist()}")
        assert np.array_equal(r["order"], Q.greedy_exact(name, batch)["order"]) and np.array_equal(r["solved"], Q.greedy_exact(name, batch)["solved"])
        assert np.all(np.abs(dev) <= D / 20)


@pytest.mark.parametrize("name", ["chain150", "general150", "chain129", "chain40"])
def test_picks_are_pinned_by_the_margins_of_the_scan(name):
    """The device test asserts the restatement's picks.  A pick is the outcome of the index-order scan, whose every comparison is
    `value > running best + 1e-8`.  A value that meets the stop rule is the Rayleigh quotient of a unit vector with
    ||r||_2 <= ||r||_1 < 1e-8 ||L_e||_inf, so it is within q_e = (1e-8 ||L_e||_inf)^2 / (lambda_3 - lambda_2)(L_e) of lambda_2(L_e)
    (the quadratic bound for a Rayleigh quotient next to an isolated eigenvalue).  Every comparison that is closer than 1e-6 to
    flipping keeps at least 10 max(q_e, q_best) -- five times the error of its two sides together (measured: 20 at the least, on
    chain150; 1e3 and more on the other inputs).  The eigh-based restatement and the iteration's agree on the picks."""
    import eig_restatement as R
    g = Q.graph(name)
    n, fi, fj, fw, ci, cj, cw = g
    K = Q.K_XCH if name == "chain40" else Q.K_PICKS
    r = R.greedy(*g, K)
    L = R.laplacian(n, fi, fj, fw)

    def q_of(e):
        Le = L + R.laplacian(n, [ci[e]], [cj[e]], [cw[e]])
        d = np.linalg.eigvalsh(Le)
        return (1e-8 * R.norm_inf(Le)) ** 2 / (d[2] - d[1])
    worst = np.inf
    for k in range(K):
        best, best_l2 = -1, 0.0
        for e, x in enumerate(r["values"][k]):
            if not np.isfinite(x):
                continue
            d = abs(x - (best_l2 + R.TIE))
            if d < 1e-6:
                q = max(q_of(e), q_of(best) if best >= 0 else 0.0)
                worst = min(worst, d / q)
                assert d >= 10 * q, (k, e, d, q)
            if x > best_l2 + R.TIE:
                best, best_l2 = e, float(x)
        assert best == r["order"][k]
        L = L + R.laplacian(n, [ci[best]], [cj[best]], [cw[best]])
    print(f"{name}: picks {r['order'].tolist()}, smallest margin / error bound over the close comparisons {worst:.3g}")
    if name == "chain40":
        assert sorted(r["order"].tolist()) == list(Q.exchange_start())
    else:
        assert np.array_equal(r["order"], Q.greedy_exact(name, 512)["order"])


def test_batch_64_prunes_with_margins_that_pin_the_solved_set():
    g = Q.graph("chain150")
    run = Q.greedy_exact("chain150", 64)
    tol = Q.prune_tol(g)
    margins = [abs(u - top) for dec in run["decisions"] for u, top in dec]
    unselected = len(g[6]) - np.arange(Q.K_PICKS)
    print("solved", run["solved"].tolist(), "of", unselected.tolist(), "smallest margin / tol", min(margins) / tol)
    assert len(margins) >= Q.K_PICKS and min(margins) >= 100 * tol
    assert np.all(run["solved"] <= unselected) and np.any(run["solved"] < unselected)      # the pruning is used
    assert np.array_equal(run["order"], Q.greedy_exact("chain150", 512)["order"])


@pytest.mark.parametrize("fold", Q.FOLDS)
def test_exchange_round_discriminates_and_is_pinned(fold):
    g = Q.graph("chain40")
    ref = Q.exchange_reference(fold)
    run = ref["run"]
    _show(f"chain40 exchange fold {fold}:", ref)
    assert ref["D"][0] >= 0.05 * ref["A"][0]
    assert {"removal_as_addition", "no_trial_column", "no_cand", "no_pending"} <= set(ref["excess"])
    tol = Q.prune_tol(g)
    margins = [abs(u - top) for u, top in run["decisions"]]
    print("swap", run["swap"], "solved", run["solved"], "smallest margin / tol", min(margins) / tol)
    assert run["swap"] is not None and run["removal"] == Q.K_XCH and min(margins) >= 100 * tol
    # the trial column lands next to pending columns for the default fold
    assert Q.exchange_round0(g, Q.exchange_start(), M=Q.Composed(16))["pending"] == Q.K_XCH


def test_exchange_round_noise_and_extended_precision_stay_inside():
    g, start = Q.graph("chain40"), Q.exchange_start()
    A = Q.exchange_exact()["applications"]
    D = min(Q.exchange_reference(fold)["D"][0] for fold in Q.FOLDS)
    runs = {"noise": Q.exchange_round0(g, start, apply_noise=1e-13, start_noise=1e-9, seed=1),
            "longdouble": Q.exchange_round0(g, start, M=Q.Exact(extended=True))}
    for fold in Q.FOLDS:
        runs[f"device's algebra, fold {fold}"] = Q.exchange_round0(g, start, M=Q.Composed(fold))
    for tag, r in runs.items():
        print(f"chain40 exchange {tag}: deviation {r['applications'] - A}, D / 20 {D / 20}")
        assert r["swap"] == Q.exchange_exact()["swap"] and r["solved"] == Q.exchange_exact()["solved"]
        assert abs(r["applications"] - A) <= D / 20


def test_two_node_polish_keeps_its_vector():
    """n = 2: the space orthogonal to 1 is span{x}, so what is left of w after the projection is rounding residue; normalised
    instead of dropped it is a second copy of x, the Gram matrix is singular and x <- x - x (most weights below ran into NaN
    before eig.h dropped w by the rule it drops p by)."""
    import eig_restatement as R
    rng = np.random.default_rng(0)
    none = ([0], [0], [0.0])
    for _ in range(50):
        w = float(rng.uniform(0.5, 2.0))
        L = R.laplacian(2, [1], [0], [w])
        x = rng.standard_normal(2)
        x -= x.mean()
        x /= np.linalg.norm(x)
        r = Q.solve_columns(L, *none, x, Q.Exact().columns(L, *none), polish=True)
        assert abs(r["lam"][0] - 2 * w) <= 1e-14 * w and np.allclose(np.abs(r["X"][:, 0]), np.sqrt(0.5), rtol=0, atol=1e-15) and r["iters"][0] <= 4


def test_extended_precision_inverse_is_an_inverse():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((3, 12, 12))
    A = B @ B.transpose(0, 2, 1) + 12 * np.eye(12)
    assert np.max(np.abs(Q._inverse_extended(A).astype(np.float64) @ A - np.eye(12))) < 1e-14
