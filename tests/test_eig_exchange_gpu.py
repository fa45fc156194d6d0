"""GreedyEig.exchange on the GPU (mac_amd/csrc/eig_exchange.h) against the NumPy restatement of its rules
(tests/eig_exchange_restatement.py).

Tolerances (those of tests/test_eig_gpu.py).  The device's stop rule is ||L v - lambda v||_1 / ||L||_inf < 1e-8 with ||v||_2 = 1, so a
reported value is within tolL = 1e-8 ||L||_inf of an eigenvalue of its L.  The scan has a tie tolerance of 1e-8, so a device swap
may fall short of the round's maximum by 1e-8 + 2 tolL (the solver's error on both sides).  A sequence is pinned only where the
restatement's gaps are at least 100 times that (tests/test_eig_exchange_host.py checks the same on the CPU).  Against MAC's Lanczos
solver (an independent solver with the same stop rule) the tolerance is 1e-8 ||L||_inf as well."""
import functools

import numpy as np
import pytest

from conftest import load_golden
import eig_exchange_restatement as E
import eig_restatement as R
from mac_amd import _lib
from mac_amd.solvers import MAC
from test_eig_gpu import arrays, chain_er, edges, petersen, random_general
import test_eig_gpu

pytestmark = pytest.mark.gpu

_made = []


def eig_of(*a, **kw):
    ge = test_eig_gpu.eig_of(*a, **kw)
    _made.append(ge)
    return ge


def mac_of(g):
    n, fi, fj, fw, ci, cj, cw = g
    mac = MAC(edges(fi, fj, fw), edges(ci, cj, cw), n)
    _made.append(mac)
    return mac


@pytest.fixture(autouse=True)
def no_handle_outlives_its_test():
    """Every handle a test of this module makes is destroyed when the test ends: nothing of it (streams, events, device memory) is
    left in the process for the modules that run afterwards."""
    yield
    for obj in _made:
        inner = getattr(obj, "_greedy_eig", None)
        if inner is not None:
            inner._dev.close()
        obj._dev.close()
    _made.clear()


def indices(sol):
    return [int(e) for e in np.flatnonzero(sol)]


def tol_of(g, sel):
    return 1e-8 * R.norm_inf(E.lap_of(g, sel))


@functools.lru_cache(maxsize=None)
def pinned():
    """chain_er(40, 0.1, 1), K = 8 from the greedy's own selection: (graph, start, the brute-force run, tol)."""
    g = chain_er(40, 0.1, 1)
    start = indices(eig_of(*g).subset(8)[0])
    run = E.brute(g, start, 100)
    return g, start, run, 1e-8 + 2e-8 * max(r["norm"] for r in run["rounds"])


# ---- 1. the pinned sequence ----
def test_pinned_sequence_equals_brute_force():
    g, start, run, tol = pinned()
    gaps = [r["best"] - r["second"] for r in run["rounds"]]
    last = abs(run["rounds"][-1]["best"] - (run["rounds"][-1]["tau"] + 1e-8))
    assert min(gaps) >= 100 * tol and last >= 100 * tol, (gaps, last, tol)      # the precondition: a seed that loses it fails here
    ge = eig_of(*g)
    sol, sel, info = ge.exchange(start)
    print("swaps", info["swaps"], "lambda2", info["lambda2"], "solved", info["solved"], "applies", info["applies"], "removals", info["removal_solves"])
    assert len(run["swaps"]) == 6 and info["swaps"] == run["swaps"] and info["converged"] is True
    assert np.allclose(info["lambda2"], run["lambda2"], rtol=0, atol=tol)
    assert indices(sol) == run["selection"] and [(e.i, e.j) for e in sel] == [(int(g[4][e]), int(g[5][e])) for e in run["selection"]]
    assert run["rounds"][-1]["swap"] is None                           # brute force finds no improving swap from the result
    rounds = len(info["swaps"]) + 1
    assert len(info["solved"]) == len(info["applies"]) == len(info["removal_solves"]) == rounds
    assert np.all(info["removal_solves"] == 8) and np.all(info["solved"] <= 8 * (len(g[6]) - 8)) and np.all(info["solved"] >= 1)
    assert np.all(info["applies"] >= info["solved"]) and info["t_ms"][0] > 0 and info["t_ms"][1] > 0


# ---- 2. the pending block, the folds and the batches do not change the swaps ----
def test_swaps_cross_folds_unchanged():
    g, start, run, tol = pinned()
    ge = eig_of(*g, fold=3)
    assert ge.info()["fold"] == 3
    sol, sel, info = ge.exchange(start)
    assert info["swaps"] == run["swaps"] and info["converged"] is True
    assert np.allclose(info["lambda2"], run["lambda2"], rtol=0, atol=tol)


def test_small_batches_unchanged():
    """K = 20 from the naive start with batch = 16: the removal columns take two batches, the survivors of a row several."""
    g = chain_er(40, 0.1, 1)
    start = E.naive_start(g, 20)
    a, b = eig_of(*g), eig_of(*g, batch=16)
    (sa, _, ia), (sb, _, ib) = a.exchange(start), b.exchange(start)
    print("K=20 swaps", ia["swaps"], "solved (default)", ia["solved"], "solved (batch 16)", ib["solved"])
    assert len(ia["swaps"]) >= 1 and ia["swaps"] == ib["swaps"] and ia["converged"] == ib["converged"] and np.array_equal(sa, sb)
    assert np.all(np.abs(ia["lambda2"] - ib["lambda2"]) <= 2 * tol_of(g, np.arange(len(g[6]))))      # (the norm with every candidate in: above every round's)
    # a row's unsolved candidates cannot reach `top`, so the rows visited are the same and a finer batch solves no more in any of them
    assert np.all(ib["solved"] <= ia["solved"]) and np.any(ib["solved"] < ia["solved"])


# ---- 3. replay validity where the gaps are not pinned ----
@pytest.mark.parametrize("name,k,cap", [("general80", 10, 4), ("chain300", 30, 2), ("petersen", 1, None), ("petersen", 5, None)])
def test_every_swap_is_a_maximiser_on_replay(name, k, cap):
    g = {"general80": lambda: random_general(80, 60, 4), "chain300": lambda: chain_er(300, 0.03, 0), "petersen": petersen}[name]()
    m = len(g[6])
    assert k < m and (name != "petersen" or k in (1, m - 1))
    if name == "chain300":
        assert (m + 255) // 256 > 1                                    # more than one workgroup per row of the pair pass
    start = E.naive_start(g, k)
    ge = eig_of(*g)
    sol, sel, info = ge.exchange(start, max_swaps=cap)
    lam = info["lambda2"]
    print(name, k, "swaps", info["swaps"], "lambda2", lam, "converged", info["converged"], "solved", info["solved"])
    assert len(lam) == len(info["swaps"]) + 1 and np.all(np.diff(lam) > 0)
    if name != "petersen":
        assert len(info["swaps"]) == cap and not info["converged"]
    rows = list(start)

    def round_of(rows):
        if name == "chain300":                                          # (38 820 dense eigenvalue problems per round otherwise)
            r = E.pruned_round(g, sorted(rows), method="secular")
            return r["tau"], r["top"]
        r = E.brute_round(g, sorted(rows))
        return r["tau"], r["best"]
    assert abs(lam[0] - R.fiedler(E.lap_of(g, rows))[0]) <= tol_of(g, rows)
    for t, (e, f) in enumerate(info["swaps"]):
        assert e in rows and f not in rows
        tau, best = round_of(rows)
        rows[rows.index(e)] = f
        tolL = tol_of(g, rows)
        exact = R.fiedler(E.lap_of(g, rows))[0]
        print(name, t, "shortfall", float(best - exact), "lambda2 err / tol", float(abs(lam[t + 1] - exact) / tolL))
        assert abs(lam[t + 1] - exact) <= tolL
        assert exact >= best - 1e-8 - 2 * tolL and exact > tau
    assert indices(sol) == sorted(rows)
    if info["converged"]:
        tau, best = round_of(rows)
        assert best <= tau + 1e-8 + 2 * tol_of(g, rows)


# ---- 4. intel ----
@functools.lru_cache(maxsize=None)
def intel_graph():
    return arrays(load_golden("g2o_intel"))


def intel():
    g = intel_graph()
    return g, mac_of(g), eig_of(*g)


@pytest.mark.parametrize("start", ["rounded", "greedy"])
def test_intel_lambda2_matches_mac_objective(start):
    g, mac, ge = intel()
    m = len(g[6])
    k = m // 10
    x0 = np.zeros(m); x0[:k] = 1.0
    s0 = mac.solve(k, x0)[0] if start == "rounded" else ge.subset(k)[0]
    sol, sel, info = ge.exchange(s0, max_swaps=2)
    print("intel", start, "K", k, "swaps", info["swaps"], "lambda2", info["lambda2"], "solved", info["solved"], "applies", info["applies"], "t_ms", info["t_ms"])
    assert len(info["swaps"]) + 1 == len(info["lambda2"]) and sol.sum() == k and len(sel) == k
    x = np.array(s0, dtype=np.float64)
    assert abs(mac.evaluate_objective(x) - info["lambda2"][0]) <= tol_of(g, indices(x))
    for t, (e, f) in enumerate(info["swaps"]):
        assert x[e] == 1.0 and x[f] == 0.0
        x[e], x[f] = 0.0, 1.0
        assert abs(mac.evaluate_objective(x) - info["lambda2"][t + 1]) <= tol_of(g, indices(x))
    assert np.array_equal(x, sol) and np.all(np.diff(info["lambda2"]) > 0)


@pytest.mark.parametrize("name,cap", [("chain40", True), ("intel", 3)])
def test_mac_solve_with_exchange_polishes_the_rounded_selection(name, cap):
    """exchange=True runs to a swap-optimal selection (the 40-node graph); on intel that takes 79 swaps of about 0.3 s, so the suite
    caps it at 3 (an integer is max_swaps)."""
    g = chain_er(40, 0.1, 1) if name == "chain40" else intel_graph()
    mac = mac_of(g)
    m = len(g[6])
    k = 8 if name == "chain40" else m // 10
    x0 = np.zeros(m); x0[:k] = 1.0
    plain = mac.solve(k, x0)
    again = mac.solve(k, x0, exchange=False)
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1]) and plain[2] == again[2]
    polished = mac.solve(k, x0, exchange=cap)
    assert np.array_equal(polished[1], plain[1]) and polished[2] == plain[2] and len(polished) == 3
    assert polished[0].shape == plain[0].shape and polished[0].sum() == k and set(np.unique(polished[0])) <= {0.0, 1.0}
    fr, fp = mac.evaluate_objective(plain[0]), mac.evaluate_objective(polished[0])
    info = mac.exchange_info
    print(f"{name} solve K={k}: lambda_2(rounded)={fr:.9g} lambda_2(polished)={fp:.9g} upper={plain[2]:.9g} swaps={len(info['swaps'])}")
    assert fp >= fr
    if cap is True:
        assert info["converged"] and E.brute_round(g, indices(polished[0]))["swap"] is None
    else:
        assert len(info["swaps"]) == cap and not info["converged"] and fp > fr
    r2 = mac.exchange(plain[0], max_swaps=1)                            # the GreedyEig is kept
    assert r2[2]["swaps"] == info["swaps"][:1]


# ---- 5. state and arguments ----
def test_runs_repeat_bit_for_bit_and_leave_the_handle_as_new():
    g, start, run, tol = pinned()
    ge, fresh = eig_of(*g), eig_of(*g)
    a = ge.exchange(start)                                              # the first call on a fresh handle
    b = ge.exchange(start)
    c = fresh.exchange(np.isin(np.arange(len(g[6])), start).astype(float))      # the 0/1 form of the same selection
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and a[1] == x[1] and a[2]["swaps"] == x[2]["swaps"] and a[2]["converged"] == x[2]["converged"]
        assert np.array_equal(a[2]["lambda2"], x[2]["lambda2"])         # bit for bit
        for key in ("solved", "applies", "removal_solves"):
            assert np.array_equal(a[2][key], x[2][key])
    # the state describes the final selection
    final = indices(a[0])
    inf = ge.info()
    assert inf["lambda2"] == a[2]["lambda2"][-1] and np.array_equal(inf["solved"], a[2]["solved"])
    L = E.lap_of(g, final)
    lam, u = ge.candidate_lambda2(), ge.candidate_bounds()
    ref = R.values_brute(L, g[4], g[5], g[6])
    uns = np.setdiff1d(np.arange(len(g[6])), final)
    assert np.all(np.isnan(lam[final])) and np.all(np.isnan(u[final]))
    assert np.all(np.abs(lam[uns] - ref[uns]) <= 1e-8 * R.norm_inf_with(L, g[4], g[5], g[6])[uns])
    # (a vector that meets the stop rule is within 1e-8 ||L||_inf / (lambda_3 - lambda_2) ~ 1e-6 of the Fiedler vector; u is linear in it)
    assert np.all(np.abs(u[uns] - R.bounds(L, g[4], g[5], g[6])[uns]) <= 1e-5) and np.all(u[uns] >= lam[uns] - tol)
    # select resets as it always has
    new = eig_of(*g)
    (s1, e1), (s0, e0) = ge.subset(8), new.subset(8)
    assert np.array_equal(s1, s0) and e1 == e0 and np.array_equal(ge.last_lambda2, new.last_lambda2)


def test_max_swaps_zero_loads_and_reports():
    g, start, run, tol = pinned()
    ge = eig_of(*g)
    sol, sel, info = ge.exchange(start, max_swaps=0)
    assert info["swaps"] == [] and info["converged"] is False and len(info["lambda2"]) == 1 and len(info["solved"]) == 0
    assert abs(info["lambda2"][0] - run["lambda2"][0]) <= tol and indices(sol) == sorted(start)
    assert ge.info()["lambda2"] == info["lambda2"][0]
    one = ge.exchange(start, max_swaps=1)[2]
    assert one["swaps"] == run["swaps"][:1] and one["converged"] is False and len(one["solved"]) == 1


def test_bad_arguments_are_named():
    g = chain_er(40, 0.1, 1)
    m = len(g[6])
    ge = eig_of(*g)
    dev = ge._dev
    good = np.arange(5)
    for sel, swaps, gain, msg in (([], 1, 0.0, "k must be"), (np.arange(m), 1, 0.0, "k must be"), ([0, m], 1, 0.0, "outside"),
                                  ([-1, 3], 1, 0.0, "outside"), ([3, 7, 3], 1, 0.0, "more than once"), (good, -1, 0.0, "max_swaps"),
                                  (good, 1, -1e-3, "min_gain"), (good, 1, np.nan, "min_gain"), (good, 1, np.inf, "min_gain")):
        with pytest.raises(AssertionError, match="BAD_ARG.*" + msg):
            dev.exchange(sel, swaps, gain)
    st = dev._lib.machip_eig_exchange(dev._h, 5, None, 1, 0.0, None, None, None, None, None, None, None, None)
    assert st == _lib.BAD_ARG and "sel_in is NULL" in _lib.last_error()
    big = chain_er(300, 0.03, 0)                                        # ldv = 320, ldm = 1324: 8 x 100 x 1644 = 1 315 200 bytes
    with _lib.default_options(eig_xch_max_mb=1):
        with pytest.raises(AssertionError, match=r"BAD_ARG.*8 x 100 x \(320 \+ 1324\) = 1315200 bytes.*eig_xch_max_mb"):
            eig_of(*big)._dev.exchange(np.arange(100), 1)
    # every output may be NULL; the handle is still good
    buf = np.arange(5, dtype=np.int32)
    assert dev._lib.machip_eig_exchange(dev._h, 5, _lib.p_i32(buf), 1, 0.0, None, None, None, None, None, None, None, None) == _lib.OK
    assert len(ge.exchange(good, max_swaps=1)[2]["swaps"]) == 1
    with pytest.raises(ValueError, match="selection"):
        ge.exchange(np.array([0.5, 2.0]))
