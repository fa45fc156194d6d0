"""The edge-space relaxation on the GPU (mac_amd/csrc/esp_relax_edge.h; ``ESPRelaxation(edge_space=True)``, a handle made with
``matrix_free=True, edge_relax=True``) against its two NumPy restatements -- node space (tests/esp_relax_restatement.py) and edge
space (tests/esp_edge_restatement.py) --, against the node form on the device, and beyond the node form's limit.

Tolerances are the node form's (tests/test_esp_relax_gpu.py).  F: 10 max(d, 1e-13 |logdet M(x)|) with d the disagreement of two
CPU routes for the same quantity, computed per graph and x (esp_relax_restatement.F_tolerance; beyond the limit d is the
disagreement of the sparse route and the edge restatement).  Gradient: 1e-10 of its largest entry.  Every figure is printed before
it is asserted (run with -s to see them).

Free-running solves (test 5) are compared free-running, not teacher-forced: the restated LP margins of intel from the naive
start are at least 2.3e-5 (K = 20 %) and 7.2e-6 (K = 50 %) of the largest gradient entry over all 20 iterations, five orders of
magnitude above the gradient tolerance, so both forms choose the restatement's vertices and their iterates stay together.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from conftest import load_golden
import esp_edge_restatement as E
import esp_relax_restatement as X
import esp_restatement as R
from mac_amd import _lib
from mac_amd.optimization.frankwolfe import frank_wolfe
from mac_amd.solvers import ESPRelaxation, GreedyESP, NaiveGreedy
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-10


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def single12():
    """The 12-node chain with one candidate: ld = 64 with 63 identity rows."""
    n, fi, fj, fw, ci, cj, cw = E.awkward12()
    return n, fi, fj, fw, ci[6:7], cj[6:7], cw[6:7]


@functools.lru_cache(maxsize=None)
def graph(case):
    if case == "awkward12":
        return E.awkward12()
    if case == "single12":
        return single12()
    if case == "er64":
        return X.chain_er(64, 0.03, 14)        # m = 64: ld = 64 without padding
    if case == "er65":
        return X.chain_er(65, 0.03, 54)        # m = 65: ld = 128, one row into the second tile
    return arrays(load_golden("g2o_" + case))


def relax_of(g, edge_space=True):
    n, fi, fj, fw, ci, cj, cw = g
    return ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n, edge_space=edge_space)


def naive(g, k):
    return NaiveGreedy(edges(g[4], g[5], g[6])).subset(k)


def check_F(tag, F_dev, F_ref, tol, d):
    print(f"{tag}: F_dev={F_dev:.15g} F_ref={F_ref:.15g} |err|={abs(F_dev - F_ref):.3e} tol={tol:.3e} d={d:.3e}")
    assert abs(F_dev - F_ref) <= tol


def check_grad(tag, g_dev, g_ref):
    err, top = float(np.max(np.abs(g_dev - g_ref))), float(np.max(np.abs(g_ref)))
    print(f"{tag}: max|grad err|={err:.3e} max g={top:.6g} rel={err / top:.3e} tol={GRAD_RTOL:.0e}")
    assert err <= GRAD_RTOL * top


@functools.lru_cache(maxsize=None)
def restated_intel_run():
    """The restatement's 20 iterates of intel at K = 50 % from the naive start (the node form's teacher-forcing input)."""
    g = graph("intel")
    k = len(g[6]) // 2
    run = X.frank_wolfe(g, k, naive(g, k), max_iters=20)
    assert len(run["F"]) == 20
    return k, run


# ---- 1. value and gradient against both restatements ----
@pytest.mark.parametrize("case,m_want,ld_want", [("awkward12", 10, 64), ("single12", 1, 64), ("er64", 64, 64), ("er65", 65, 128),
                                                 ("kitti_05", 66, 128), ("intel", 785, 832)])
def test_value_and_gradient_match_both_restatements(case, m_want, ld_want):
    g = graph(case)
    m = len(g[6])
    assert m == m_want
    relax = relax_of(g)
    dev = relax._dev
    assert dev.relax_info() == dict(form="edge", ld=ld_want) and dev.info()["form"] == "chain_free"
    ld0 = X.logdet_dense(X.M_of(g, np.zeros(m)))
    # x = 0: N = I, every pivot is 1
    F, gr = relax.problem(np.zeros(m))
    print(f"{case} x=0: F={F!r}")
    assert F == 0.0 and relax.evaluate_objective(np.zeros(m)) == 0.0
    check_grad(f"{case} x=0 vs node restatement", gr, X.gradient(g, np.zeros(m)))
    check_grad(f"{case} x=0 vs edge restatement", gr, E.gradient(g, np.zeros(m)))
    # x = the indicator of a greedy run on the same handle
    k = max(1, m // 3)
    order, gain, _ = dev.select([k])
    wr = dev.weighted_resistances()
    x = np.zeros(m); x[order] = 1.0
    F, gr = relax.problem(x)
    tol, d, _ = X.F_tolerance(g, x)
    check_F(f"{case} x=greedy({k}) vs node restatement", F, X.objective(g, x, ld0), tol, d)
    check_F(f"{case} x=greedy({k}) vs edge restatement", F, E.objective(g, x), tol, d)
    check_F(f"{case} x=greedy({k}) vs sum log1p(gains)", F, float(np.sum(np.log1p(gain))), tol, d)
    check_grad(f"{case} x=greedy({k}) vs node restatement", gr, X.gradient(g, x))
    check_grad(f"{case} x=greedy({k}) vs edge restatement", gr, E.gradient(g, x))
    check_grad(f"{case} x=greedy({k}) vs weighted_resistances", gr, wr)
    # seeded uniform x, and the wild x (30 % exact zeros, the rest 10^U(-14, 0))
    for tag, x in (("uniform", np.random.default_rng(17).random(m)), ("wild", E.wild_x(m))):
        F, gr = relax.problem(x)
        tol, d, _ = X.F_tolerance(g, x)
        check_F(f"{case} x={tag} vs node restatement", F, X.objective(g, x, ld0), tol, d)
        check_F(f"{case} x={tag} vs edge restatement", F, E.objective(g, x), tol, d)
        check_grad(f"{case} x={tag} vs node restatement", gr, X.gradient(g, x))
        check_grad(f"{case} x={tag} vs edge restatement", gr, E.gradient(g, x))
        assert relax.evaluate_objective(x) == F
    if case == "awkward12":
        assert gr[5] == 0.0                                                   # the self-loop: its column of G is zero


# ---- 2. edge form against node form on the device ----
def test_edge_form_agrees_with_the_node_form_on_the_device():
    g = graph("intel")
    m = len(g[6])
    edge, node = relax_of(g), relax_of(g, edge_space=False)
    assert node._dev.relax_info() == dict(form="node", ld=0)
    x = np.random.default_rng(17).random(m)
    Fe, ge = edge.problem(x)
    Fn, gn = node.problem(x)
    tol, d, _ = X.F_tolerance(g, x)
    check_F("intel edge vs node on the device", Fe, Fn, tol, d)
    check_grad("intel edge vs node on the device", ge, gn)
    ie, ino = edge.info(), node.info()
    print("info:", ie, ino)
    assert (ie["relax_form"], ie["relax_ld"]) == ("edge", 832) and (ino["relax_form"], ino["relax_ld"]) == ("node", 1728)


# ---- 3. beyond the node form's limit ----
def long_chain(n=16385, cands=300, seed=41):
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    a = rng.integers(0, n, cands); b = rng.integers(0, n, cands)
    a[0], b[0] = 0, 7000                         # one candidate at node 0
    a[1], b[1] = n - 1, 0                        # one spanning the whole chain (given hi first)
    return n, fi, fj, fw, a, b, rng.uniform(0.5, 2.0, cands)


def test_beyond_the_node_forms_limit_matches_sparse_solves():
    from scipy.sparse.linalg import splu
    g = long_chain()
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    assert n == 16385 and m == 300
    x = np.random.default_rng(43).random(m)
    Mx = X.M_of(g, x, sparse=True)
    ldx = R.logdet_sparse(Mx)
    F_sparse = ldx - R.logdet_sparse(X.M_of(g, np.zeros(m), sparse=True))
    F_edge = E.objective(g, x)
    d = abs(F_sparse - F_edge)
    tol = 10.0 * max(d, 1e-13 * abs(ldx))
    A = np.zeros((n, m))
    ar = np.arange(m)
    np.add.at(A, (ci, ar), 1.0)
    np.add.at(A, (cj, ar), -1.0)
    A = A[1:]
    g_sparse = cw * np.einsum("ij,ij->j", A, splu(Mx).solve(A))
    relax = relax_of(g)
    assert relax._dev.relax_info() == dict(form="edge", ld=320)
    F, gr = relax.problem(x)
    print(f"chain16385: logdet M(x)={ldx:.15g}")
    check_F("chain16385 vs sparse LU", F, F_sparse, tol, d)
    check_F("chain16385 vs edge restatement", F, F_edge, tol, d)
    check_grad("chain16385 vs sparse solves", gr, g_sparse)
    check_grad("chain16385 vs edge restatement", gr, E.gradient(g, x))
    F0, g0 = relax.problem(np.zeros(m))
    assert F0 == 0.0
    k = 100
    rounded, unrounded, upper = relax.solve(k, naive(g, k), max_iters=5)
    print(f"chain16385 K={k}: upper={upper:.12g} F(rounded)={relax.evaluate_objective(rounded):.12g}")
    assert upper >= relax.evaluate_objective(rounded) and rounded.sum() == k
    # the node form still refuses this graph
    plain = relax_of(g, edge_space=False)
    with pytest.raises(AssertionError, match="BAD_ARG.*16384"):
        plain.problem(x)
    with pytest.raises(AssertionError, match="BAD_ARG.*16384"):
        plain._dev.relax_run(k, x)


# ---- 4. teacher forcing ----
def test_teacher_forcing_on_the_restated_iterates_of_intel_every_vertex():
    g = graph("intel")
    k, run = restated_intel_run()
    print("restated margins:", " ".join(f"{v:.2e}" for v in run["margin"]))
    assert min(run["margin"]) > 1e4 * GRAD_RTOL          # the reference alone stays inside this condition
    dev = relax_of(g)._dev
    for t in range(20):
        x, s = run["iterates"][t], run["vertex"][t]
        tol, d, _ = X.F_tolerance(g, x)
        F, gr = dev.relax_eval(x)
        check_F(f"iterate {t}", F, run["F"][t], tol, d)
        check_grad(f"iterate {t}", gr, run["grad"][t])
        one = dev.relax_run(k, x, max_iters=1, gap_tol=0.0, grad_tol=0.0)      # step 2 / (2 + 0) = 1: the iterate it returns is the vertex
        assert one["iters"] == 1 and one["f"][0] == F
        dtol = tol + GRAD_RTOL * float(np.max(run["grad"][t])) * float(np.sum(np.abs(s - x)))
        print(f"iterate {t}: dual_dev={one['dual'][0]:.15g} dual_ref={run['dual'][t]:.15g} tol={dtol:.3e}")
        assert np.array_equal(one["x"] > 0.5, s > 0.5)
        assert abs(one["dual"][0] - run["dual"][t]) <= dtol


# ---- 5. free-running solve ----
@pytest.mark.parametrize("pct", [0.2, 0.5])
def test_free_running_solve_bounds_every_selection_and_follows_the_node_form(pct):
    g = graph("intel")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    k = int(pct * m)
    x0 = naive(g, k)
    relax, node = relax_of(g), relax_of(g, edge_space=False)
    rounded, unrounded, upper = relax.solve(k, x0)
    trace = list(relax.trace)
    _, _, upper_n = node.solve(k, x0)
    trace_n = list(node.trace)
    greedy_x, _ = GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n).subset(k)
    Fr, Fg, Fnv = (relax.evaluate_objective(v) for v in (rounded, greedy_x, x0))
    print(f"K={k}: upper={upper:.15g} node upper={upper_n:.15g} F(rounded)={Fr:.12g} F(greedy)={Fg:.12g} F(naive)={Fnv:.12g} "
          f"F(unrounded)={trace[-1][0]:.15g} node F(unrounded)={trace_n[-1][0]:.15g} iterations={len(trace)}/{len(trace_n)}")
    assert upper >= Fr and upper >= Fg and upper >= Fnv
    assert rounded.sum() == k and set(np.unique(rounded)) <= {0.0, 1.0}
    ups = [t[1] for t in trace]
    assert all(a >= b for a, b in zip(ups, ups[1:])) and ups[-1] == upper
    assert unrounded.min() >= 0.0 and unrounded.max() <= 1.0 and unrounded.sum() <= k * (1 + 1e-12)
    assert len(trace) == len(trace_n)
    print(f"K={k}: rel |F - F_node|={abs(trace[-1][0] - trace_n[-1][0]) / abs(trace_n[-1][0]):.3e} "
          f"rel |upper - upper_node|={abs(upper - upper_n) / abs(upper_n):.3e} bound=1e-9")
    assert abs(trace[-1][0] - trace_n[-1][0]) <= 1e-9 * abs(trace_n[-1][0])
    assert abs(upper - upper_n) <= 1e-9 * abs(upper_n)


# ---- 6. determinism ----
def test_two_solves_are_bit_identical():
    g = graph("intel")
    k = len(g[6]) // 5
    x0 = naive(g, k)
    a, b = relax_of(g)._dev, relax_of(g)._dev
    r1 = a.relax_run(k, x0)
    r2 = a.relax_run(k, x0)
    r3 = b.relax_run(k, x0)
    assert r1["iters"] > 1
    for r in (r2, r3):
        assert r["iters"] == r1["iters"] and r["upper"] == r1["upper"] and np.array_equal(r["x"], r1["x"])
        for key in ("f", "dual", "gnorm"):
            assert np.array_equal(r[key], r1[key]), key


# ---- 7. the greedy survives ----
def test_relaxation_calls_leave_the_greedy_state_alone():
    g = graph("intel")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    k = m // 4
    dev = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free=True, edge_relax=True)
    fresh = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free=True)
    order0, gain0, _ = fresh.select([k])
    wr0 = fresh.weighted_resistances()
    order, gain, _ = dev.select([k])
    before = dev.weighted_resistances().copy()
    info = dev.info()
    assert info["pending"] == k
    dev.relax_eval(np.random.default_rng(1).random(m))
    dev.relax_run(k, naive(g, k), max_iters=3)
    after = dev.weighted_resistances()
    assert np.array_equal(before, after) and np.array_equal(before, wr0) and dev.info() == info
    order2, gain2, _ = dev.select([k])
    assert np.array_equal(order2, order0) and np.array_equal(gain2, gain0)
    assert np.array_equal(order, order0) and np.array_equal(gain, gain0)
    assert np.array_equal(dev.weighted_resistances(), wr0)


# ---- 8. the same evaluation under the package's own Frank-Wolfe driver ----
def test_frank_wolfe_driver_reproduces_solve_bit_for_bit_on_kitti_05():
    g = graph("kitti_05")
    k = len(g[6]) // 3
    x0 = naive(g, k)
    relax = relax_of(g)
    _, unrounded, upper = relax.solve(k, x0, max_iters=20, relative_duality_gap_tol=1e-4, grad_norm_tol=1e-8)
    x, u = frank_wolfe(x0, relax.problem, lambda gr: X.lp_vertex(gr, k), maxiter=20, relative_duality_gap_tol=1e-4, grad_norm_tol=1e-8,
                       inner=relax.inner)
    print(f"upper solve={upper!r} driver={float(u)!r}; max|x diff|={np.max(np.abs(x - unrounded)):.3e}")
    assert np.array_equal(x, unrounded) and u == upper


# ---- 9. shortcut and error paths ----
def test_budget_of_all_candidates_takes_the_shortcut():
    g = graph("awkward12")
    m = len(g[6])
    relax = relax_of(g)
    rounded, unrounded, upper = relax.solve(m, np.ones(m))
    assert np.array_equal(rounded, np.ones(m)) and np.array_equal(unrounded, np.ones(m))
    assert upper == relax.evaluate_objective(np.ones(m)) and upper > 0
    assert relax.trace == []


def small_case_still_right(dev, g):
    m = len(g[6])
    x = np.random.default_rng(5).random(m)
    F, gr = dev.relax_eval(x)
    assert abs(F - E.objective(g, x)) <= X.F_tolerance(g, x)[0]
    assert np.max(np.abs(gr - E.gradient(g, x))) <= GRAD_RTOL * np.max(gr)


def test_error_paths():
    g = graph("awkward12")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    dev = relax_of(g)._dev
    for bad in (np.full(m, 1.5), np.full(m, -1e-3), np.full(m, np.nan), np.full(m, np.inf)):
        with pytest.raises(AssertionError, match=r"BAD_ARG.*\[0, 1\]"):
            dev.relax_eval(bad)
        with pytest.raises(AssertionError, match=r"BAD_ARG.*\[0, 1\]"):
            dev.relax_run(2, bad)
    for k in (0, m + 1):
        with pytest.raises(AssertionError, match="BAD_ARG.*k must be"):
            dev.relax_run(k, np.zeros(m))
    small_case_still_right(dev, g)
    # the flag's combinations: BAD_ARG that names it, no handle, through the raw C call
    lib = _lib.load()
    i32, f64, p_i32, p_f64 = _lib.i32, _lib.f64, _lib.p_i32, _lib.p_f64

    def create(fi, fj, fw, flags):
        h = C.c_void_p()
        st = lib.machip_esp_create(0, n, len(fw), p_i32(i32(fi)), p_i32(i32(fj)), p_f64(f64(fw)), m, p_i32(i32(ci)), p_i32(i32(cj)),
                                   p_f64(f64(cw)), 0, flags, C.byref(h))
        msg = _lib.last_error()
        if st == _lib.OK:
            lib.machip_esp_destroy(h)
        return st, msg, h.value

    st, msg, h = create(fi, fj, fw, _lib.ESP_EDGE_RELAX)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "MACHIP_ESP_MATRIX_FREE" in msg and not h
    st, msg, h = create(fi, fj, fw, _lib.ESP_EDGE_RELAX | _lib.ESP_MATRIX_FREE | _lib.ESP_SPANNING_TREE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "MACHIP_ESP_SPANNING_TREE" in msg and not h
    st, msg, h = create(np.append(fi, 0), np.append(fj, 6), np.append(fw, 1.0), _lib.ESP_EDGE_RELAX | _lib.ESP_MATRIX_FREE)     # a chord: not the chain
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "needs a chain" in msg and not h
    small_case_still_right(dev, g)
    # more candidates than the m x m inverse takes: refused at the first relaxation call, before anything is allocated
    big_m = 16385
    rng = np.random.default_rng(7)
    big = _lib.Esp(n, fi, fj, fw, rng.integers(0, n, big_m), rng.integers(0, n, big_m), rng.uniform(0.5, 2.0, big_m),
                   matrix_free=True, edge_relax=True)
    for call in (lambda: big.relax_eval(np.zeros(big_m)), lambda: big.relax_run(5, np.zeros(big_m)),
                 lambda: big.relax_inner(np.zeros(big_m), np.zeros(big_m))):
        t0 = time.perf_counter()
        with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_EDGE_RELAX.*16384"):
            call()
        dt = time.perf_counter() - t0
        print(f"m = {big_m}: refused in {dt * 1e3:.2f} ms")
        assert dt < 0.5                                                  # (a host check: no allocation, no launch)
    order, gain, _ = big.select([3])                                     # the greedy of that handle is not limited by m
    assert len(set(order.tolist())) == 3
    big.close()
    small_case_still_right(dev, g)
    small_case_still_right(relax_of(g)._dev, g)
