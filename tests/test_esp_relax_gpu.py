"""The relaxation of GreedyESP's problem on the GPU (mac_amd/csrc/esp_relax.h) against its NumPy restatement
(tests/esp_relax_restatement.py), through the public class ``ESPRelaxation`` and the handle ``_lib.Esp``.

Tolerances.  F: on every graph and x the test computes log det M(x) on the CPU by two independent routes (dense LAPACK LU and
sparse SuperLU); their disagreement d is what fp64 allows, and the device -- a blocked elimination without pivoting, which sums
in a third order -- gets 10 max(d, 1e-13 |logdet M(x)|) (esp_relax_restatement.F_tolerance; nothing is hard-coded).  Gradient:
1e-10 of its largest entry, the tolerance test_esp_gpu.py::test_resistances_after_create_match_dense_inverse uses for the same
quantity.  Every figure is printed before it is asserted (run with -s to see them).
"""
import numpy as np
import pytest

from conftest import load_golden
import esp_relax_restatement as X
from mac_amd import _lib
from mac_amd.optimization.frankwolfe import frank_wolfe
from mac_amd.solvers import MAC, ESPRelaxation, GreedyESP, NaiveGreedy
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-10


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def graph(case):
    if case == "petersen":
        return X.petersen()
    if case == "general500":
        return X.random_general()
    if case == "disconnected":
        return X.disconnected()
    return arrays(load_golden("g2o_" + case))


def relax_of(g):
    n, fi, fj, fw, ci, cj, cw = g
    return ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n)


def naive(g, k):
    return NaiveGreedy(edges(g[4], g[5], g[6])).subset(k)


def check_F(tag, F_dev, F_ref, tol, d):
    print(f"{tag}: F_dev={F_dev:.15g} F_ref={F_ref:.15g} |err|={abs(F_dev - F_ref):.3e} tol={tol:.3e} d={d:.3e}")
    assert abs(F_dev - F_ref) <= tol


def check_grad(tag, g_dev, g_ref):
    err, top = float(np.max(np.abs(g_dev - g_ref))), float(np.max(np.abs(g_ref)))
    print(f"{tag}: max|grad err|={err:.3e} max g={top:.6g} rel={err / top:.3e} tol={GRAD_RTOL:.0e}")
    assert err <= GRAD_RTOL * top


# ---- 1. value and gradient ----
@pytest.mark.parametrize("case", ["petersen", "general500", "disconnected", "intel", "sphere2500"])
def test_value_and_gradient_match_the_restatement(case):
    g = graph(case)
    m = len(g[6])
    relax = relax_of(g)
    dev = relax._dev
    assert dev.info()["beta"] == (1e-4 if case == "disconnected" else 0.0)
    ld0 = X.logdet_dense(X.M_of(g, np.zeros(m)))
    # x = 0
    F, gr = relax.problem(np.zeros(m))
    assert F == 0.0 and relax.evaluate_objective(np.zeros(m)) == 0.0
    check_grad(f"{case} x=0", gr, X.gradient(g, np.zeros(m)))
    # x = the indicator of a greedy run on the same handle
    k = max(1, m // 3)
    order, gain, _ = dev.select([k])
    wr = dev.weighted_resistances()
    x = np.zeros(m); x[order] = 1.0
    F, gr = relax.problem(x)
    tol, d, ld = X.F_tolerance(g, x)
    check_F(f"{case} x=greedy({k}) vs restatement", F, X.objective(g, x, ld0), tol, d)
    check_F(f"{case} x=greedy({k}) vs sum log1p(gains)", F, float(np.sum(np.log1p(gain))), tol, d)
    check_grad(f"{case} x=greedy({k}) vs restatement", gr, X.gradient(g, x))
    check_grad(f"{case} x=greedy({k}) vs weighted_resistances", gr, wr)
    # seeded fractional x
    x = np.random.default_rng(17).random(m)
    F, gr = relax.problem(x)
    tol, d, ld = X.F_tolerance(g, x)
    check_F(f"{case} x=fractional", F, X.objective(g, x, ld0), tol, d)
    check_grad(f"{case} x=fractional", gr, X.gradient(g, x))
    assert relax.evaluate_objective(x) == F


# ---- 2. teacher forcing: the device evaluates the restatement's own iterates ----
def test_teacher_forcing_on_the_restated_iterates_of_intel():
    g = graph("intel")
    m = len(g[6])
    k = m // 2
    run = X.frank_wolfe(g, k, naive(g, k), max_iters=20)
    assert len(run["F"]) == 20
    print("restated margins:", " ".join(f"{v:.2e}" for v in run["margin"]))
    dev = relax_of(g)._dev
    left_out = 0
    for t in range(20):
        x, s = run["iterates"][t], run["vertex"][t]
        tol, d, _ = X.F_tolerance(g, x)
        F, gr = dev.relax_eval(x)
        check_F(f"iterate {t}", F, run["F"][t], tol, d)
        check_grad(f"iterate {t}", gr, run["grad"][t])
        one = dev.relax_run(k, x, max_iters=1, gap_tol=0.0, grad_tol=0.0)      # step 2 / (2 + 0) = 1: the iterate it returns is the vertex
        assert one["iters"] == 1 and one["f"][0] == F
        # the dual value inherits F's error and the gradient's against s - x (entries in [-1, 1])
        dtol = tol + GRAD_RTOL * float(np.max(run["grad"][t])) * float(np.sum(np.abs(s - x)))
        print(f"iterate {t}: dual_dev={one['dual'][0]:.15g} dual_ref={run['dual'][t]:.15g} tol={dtol:.3e}")
        if run["margin"][t] > 1e-8:
            assert np.array_equal(one["x"] > 0.5, s > 0.5)
            assert abs(one["dual"][0] - run["dual"][t]) <= dtol
        else:
            left_out += 1
    assert left_out <= 2


# ---- 3. free-running solve ----
@pytest.mark.parametrize("pct", [0.2, 0.5])
def test_free_running_solve_bounds_every_selection_and_follows_the_restatement(pct):
    g = graph("intel")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    k = int(pct * m)
    x0 = naive(g, k)
    relax = relax_of(g)
    rounded, unrounded, upper = relax.solve(k, x0)
    trace = list(relax.trace)
    tol = X.F_tolerance(g, unrounded)[0]
    ge = GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n)
    greedy_x, _ = ge.subset(k)
    mac_x = MAC(edges(fi, fj, fw), edges(ci, cj, cw), n).solve(k, x0)[0]
    Fg, Fr, Fm = (relax.evaluate_objective(v) for v in (greedy_x, rounded, mac_x))
    print(f"K={k}: upper={upper:.12g} F(greedy)={Fg:.12g} F(rounded)={Fr:.12g} F(MAC rounded)={Fm:.12g} "
          f"F(unrounded)={trace[-1][0]:.12g} iterations={len(trace)} tol={tol:.3e}")
    assert upper >= Fg - tol and upper >= Fr - tol and upper >= Fm - tol
    assert rounded.sum() == k and set(np.unique(rounded)) <= {0.0, 1.0}
    ups = [t[1] for t in trace]
    assert all(a >= b for a, b in zip(ups, ups[1:])) and ups[-1] == upper
    assert unrounded.min() >= 0.0 and unrounded.max() <= 1.0 and unrounded.sum() <= k * (1 + 1e-12)
    run = X.frank_wolfe(g, k, x0, max_iters=20)
    agreed = next((t for t, v in enumerate(run["margin"]) if v <= 1e-8), len(run["margin"]))     # vertices are pinned before this
    ref_up = np.minimum.accumulate(run["dual"])
    for t in range(min(agreed + 1, len(trace), len(run["F"]))):
        print(f"K={k} it {t}: F_dev={trace[t][0]:.15g} F_ref={run['F'][t]:.15g} upper_dev={trace[t][1]:.15g} upper_ref={ref_up[t]:.15g}")
        assert abs(trace[t][0] - run["F"][t]) <= tol * (1 + t)
    if agreed == len(run["margin"]):
        # Did every LP vertex of the device agree with the restatement's?  The update x + gamma (s - x) is the same two-rounding
        # expression on both sides, so with equal vertices the final iterates are equal to the last bits, while a vertex that
        # differs at iteration t moves an entry of the final iterate by gamma_t prod_{j > t} (1 - gamma_j) >= 2 / (20 * 21).
        assert len(trace) == len(run["F"])
        print(f"K={k}: max|x_dev - x_ref|={np.max(np.abs(unrounded - run['x'])):.3e}")
        assert np.max(np.abs(unrounded - run["x"])) <= 1e-12
        assert abs(trace[-1][0] - run["F"][-1]) <= tol * (1 + len(trace))
        print(f"K={k}: |upper_dev - upper_ref|={abs(upper - run['upper']):.3e} bound={tol * (1 + len(trace)):.3e}")
        assert abs(upper - run["upper"]) <= tol * (1 + len(trace))


# ---- 4. determinism, coexistence with the greedy, shortcut, errors ----
def test_two_solves_are_bit_identical():
    g = graph("intel")
    k = len(g[6]) // 5
    x0 = naive(g, k)
    a = relax_of(g)
    r1 = a.solve(k, x0)
    t1 = list(a.trace)
    r2 = a.solve(k, x0)
    b = relax_of(g)
    r3 = b.solve(k, x0)
    for r, t in ((r2, a.trace), (r3, b.trace)):
        assert np.array_equal(r1[0], r[0]) and np.array_equal(r1[1], r[1]) and r1[2] == r[2] and t1 == t


@pytest.mark.parametrize("case", ["general500", "intel"])
def test_greedy_selection_after_relaxation_calls_is_that_of_a_fresh_handle(case):
    g = graph(case)
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    ks = [m // 10, m // 4, m // 2]
    fresh = GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n)
    res0, sel0, _ = fresh.subsets_lazy(ks)
    used = GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n)
    used._dev.relax_eval(np.random.default_rng(1).random(m))
    used._dev.relax_run(ks[1], naive(g, ks[1]), max_iters=3)
    res1, sel1, _ = used.subsets_lazy(ks)
    used._dev.relax_eval(np.zeros(m))
    res2, sel2, _ = used.subsets_lazy(ks)
    for res, sel in ((res1, sel1), (res2, sel2)):
        assert all(np.array_equal(a, b) for a, b in zip(res0, res)) and sel0 == sel
    assert np.array_equal(fresh.last_gains, used.last_gains)
    assert used.info() == fresh.info()


def test_budget_of_all_candidates_takes_the_shortcut():
    g = graph("petersen")
    m = len(g[6])
    relax = relax_of(g)
    rounded, unrounded, upper = relax.solve(m, np.ones(m))
    assert np.array_equal(rounded, np.ones(m)) and np.array_equal(unrounded, np.ones(m))
    assert upper == relax.evaluate_objective(np.ones(m)) and upper > 0


def test_error_paths():
    g = graph("petersen")
    m = len(g[6])
    dev = relax_of(g)._dev
    # (the binding turns MACHIP_BAD_ARG into an AssertionError that carries machip_last_error, as for every other entry point)
    for bad in (np.full(m, 1.5), np.full(m, -1e-3), np.full(m, np.nan), np.full(m, np.inf)):
        with pytest.raises(AssertionError, match=r"BAD_ARG.*\[0, 1\]"):
            dev.relax_eval(bad)
        with pytest.raises(AssertionError, match=r"BAD_ARG.*\[0, 1\]"):
            dev.relax_run(2, bad)
    for k in (0, -1, m + 1):
        with pytest.raises(AssertionError, match="BAD_ARG.*k must be"):
            dev.relax_run(k, np.zeros(m))
    with pytest.raises(AssertionError):
        dev.relax_eval(np.zeros(m + 1))
    assert dev.relax_eval(np.zeros(m))[0] == 0.0                     # the handle is still good
    # the smallest n the relaxation's limit rejects: a chain (which the greedy accepts up to 32 768), no candidates
    n = 16385
    big = _lib.Esp(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1), [], [], [])
    assert big.info()["form"] == "chain"
    with pytest.raises(AssertionError, match="BAD_ARG.*16384"):
        big.relax_eval(np.zeros(0))
    with pytest.raises(AssertionError, match="BAD_ARG.*16384"):
        big.relax_run(1, np.zeros(0))
    big.close()


def many_parallel_candidates(n=200, pairs=20000, seed=31):
    """A chain of 200 nodes with 40 000 candidates: 20 000 random pairs, each listed twice with the same weight -- more than the
    32 768 keys the one-launch select takes, and exact ties in every gradient."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    a = rng.integers(0, n, pairs); b = (a + rng.integers(2, n - 1, pairs)) % n
    w = rng.uniform(0.5, 2.0, pairs)
    return n, fi, fj, fw, np.repeat(a, 2), np.repeat(b, 2), np.repeat(w, 2)


def test_lp_vertex_of_the_multi_launch_select_with_exact_ties():
    """m = 40 000 > 32 768: the select runs as k_sel_init + six k_sel_pass + k_sel_ties on the handle's own state.  Every candidate
    has an exact twin, so an odd k cuts a pair: the vertex must be the top-k of the device's own gradient with ties to the lowest
    index, and -- where the restated margin between distinct values allows -- the restatement's."""
    g = many_parallel_candidates()
    m = len(g[6])
    assert m > 32768
    k = 4001
    dev = relax_of(g)._dev
    x = np.random.default_rng(3).random(m) * (k / m)
    F, gr = dev.relax_eval(x)
    assert np.array_equal(gr[0::2], gr[1::2])                      # twins score the same bits
    one = dev.relax_run(k, x, max_iters=1, gap_tol=0.0, grad_tol=0.0)      # step 1: the iterate returned is the vertex
    s_dev = (one["x"] > 0.5).astype(np.float64)
    s_own = X.lp_vertex(gr, k)
    assert s_dev.sum() == k and np.array_equal(s_dev, s_own)
    cut = np.nonzero(s_dev[0::2] != s_dev[1::2])[0]
    assert len(cut) == 1 and s_dev[2 * cut[0]] == 1.0 and s_dev[2 * cut[0] + 1] == 0.0      # the pair that k cuts: lower index in
    assert one["f"][0] == F and one["dual"][0] == F + dev.relax_inner(gr, s_own - x)
    g_ref = X.gradient(g, x)
    check_grad("parallel40000", gr, g_ref)
    distinct = np.sort(g_ref[0::2])[::-1]
    margin = (distinct[k // 2 - 1] - distinct[k // 2]) / distinct[0], (distinct[k // 2] - distinct[k // 2 + 1]) / distinct[0]
    print(f"parallel40000: restated margins around the cut pair {margin[0]:.2e} {margin[1]:.2e}")
    if min(margin) > 1e-8:
        assert np.array_equal(s_dev, X.lp_vertex(g_ref, k))
    # |g|: every entry within GRAD_RTOL max g, so the norm within that times sqrt(m)
    assert abs(one["gnorm"][0] - np.linalg.norm(g_ref)) <= GRAD_RTOL * np.max(g_ref) * np.sqrt(m)


# ---- 5. the same evaluation under the package's own Frank-Wolfe driver ----
def driver_and_solve(**kw):
    g = graph("petersen")
    k = 3
    x0 = naive(g, k)
    relax = relax_of(g)
    _, unrounded, upper = relax.solve(k, x0, max_iters=20, relative_duality_gap_tol=1e-4, grad_norm_tol=1e-8)
    if kw.pop("device_inner", False):
        kw["inner"] = relax.inner
    x, u = frank_wolfe(x0, relax.problem, lambda gr: X.lp_vertex(gr, k), maxiter=20, relative_duality_gap_tol=1e-4, grad_norm_tol=1e-8, **kw)
    print(f"upper solve={upper!r} driver={float(u)!r} diff={upper - u:.3e}; max|x diff|={np.max(np.abs(x - unrounded)):.3e}")
    return x, u, unrounded, upper


def test_frank_wolfe_driver_on_problem_reproduces_the_iterate_of_solve_bit_for_bit():
    x, _, unrounded, _ = driver_and_solve(device_inner=True)
    assert np.array_equal(x, unrounded)
    x, _, unrounded, _ = driver_and_solve()          # (the iterate does not depend on how the dual value is summed)
    assert np.array_equal(x, unrounded)


def test_frank_wolfe_driver_on_problem_reproduces_the_upper_bound_of_solve_bit_for_bit():
    """F and the gradient are the same device evaluation in the driver and in ``solve``; the dual value F + g.(s - x) is too once
    the driver sums g.(s - x) through ``ESPRelaxation.inner`` (machip_esp_relax_inner: the device, in the order of the loop's own
    reduction).  With the driver's default, NumPy's dot product, the same six products are summed in another order and the
    upper bound agreed to one unit in the last place only (measured on an MI355X: 6.228878550903139 vs 6.22887855090314)."""
    _, u, _, upper = driver_and_solve(device_inner=True)
    assert u == upper


def test_inner_sums_in_the_order_of_the_loop_on_a_long_vector():
    """One Frank-Wolfe iteration of intel from a fractional x: the dual value of machip_esp_relax_run against
    F + inner(g, s - x) formed on the host from machip_esp_relax_eval's F and gradient -- equal bits, 785 products."""
    g = graph("intel")
    m = len(g[6])
    k = m // 5
    dev = relax_of(g)._dev
    x = np.random.default_rng(23).random(m) * (k / m)
    F, gr = dev.relax_eval(x)
    one = dev.relax_run(k, x, max_iters=1, gap_tol=0.0, grad_tol=0.0)
    s = X.lp_vertex(gr, k)
    assert one["f"][0] == F
    assert one["dual"][0] == F + dev.relax_inner(gr, s - x)
    assert abs(dev.relax_inner(gr, s - x) - gr @ (s - x)) <= 1e-12 * np.abs(gr) @ np.abs(s - x)
