"""The exchange on the log tree count on the GPU (mac_amd/csrc/esp_exchange.h) against its NumPy restatement
(tests/esp_exchange_restatement.py), through ``GreedyESP.exchange``, ``ESPRelaxation`` and the handle ``_lib.Esp``.

Sequences are compared on the inputs tests/test_esp_exchange_host.py keeps at least 1e-6 apart at every round (and, for the
tie graph, tied exactly), so no round is left out.  Tolerances: a swap's ratio against log det M' - log det M within the sum of
esp_relax_restatement.F_tolerance at both selections (each 10 x the disagreement of dense LU and SuperLU); the growth within
F_tolerance at the final selection; resistances within 1e-10 of the largest entry (GRAD_RTOL of tests/test_esp_relax_gpu.py).
Every compared figure is printed before it is asserted (run with -s to see them)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
import esp_exchange_restatement as E
import esp_relax_restatement as X
from mac_amd import _lib
from mac_amd.solvers import ESPRelaxation, GreedyESP, NaiveGreedy
from mac_amd.utils.graphs import Edge
from test_esp_relax_gpu import GRAD_RTOL

pytestmark = pytest.mark.gpu

MIN_GAIN = 1e-9


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def greedy_of(g, **kw):
    n, fi, fj, fw, ci, cj, cw = g
    return GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


def intel():
    g = load_golden("g2o_intel")
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def naive_start(g, k):
    """NaiveGreedy's selection, which is the restatement's naive start (the k heaviest candidates)."""
    sel = np.flatnonzero(NaiveGreedy(edges(g[4], g[5], g[6])).subset(k))
    assert np.array_equal(sel, E.naive_start(g, k))
    return sel


def greedy_start(ge, g, k):
    """The device greedy's selection, which is the restated greedy's: the start the host test measured the separations from."""
    sel = np.flatnonzero(ge.subset(k)[0])
    assert np.array_equal(sel, E.greedy_start(g, k))
    return sel


def check_sequence(tag, info, result, ref):
    print(f"{tag}: swaps dev={info['swaps']} ref={len(ref['out'])} converged dev={info['converged']} ref={ref['converged']}")
    print(f"{tag}: out dev={list(info['out'])} ref={ref['out']}")
    print(f"{tag}: in  dev={list(info['in'])} ref={ref['in']}")
    assert list(info["out"]) == ref["out"] and list(info["in"]) == ref["in"]
    assert info["swaps"] == len(ref["out"]) and int(info["converged"]) == ref["converged"]
    assert np.array_equal(np.flatnonzero(result), ref["selection"])


def check_ratios(tag, g, start, info, per_swap=True):
    """Every swap's ratio against the CPU's log-determinants (per_swap), and the growth against F(final) - F(start)."""
    m = len(g[6])
    sel = np.sort(np.asarray(start))
    for t, (e, f, r) in enumerate(zip(info["out"], info["in"], info["ratios"])):
        if per_swap:
            ref, tol = E.log_ratio_check(g, sel, e, f)
            print(f"{tag} swap {t}: log ratio dev={np.log(r):.15g} cpu={ref:.15g} |err|={abs(np.log(r) - ref):.3e} tol={tol:.3e}")
            assert abs(np.log(r) - ref) <= tol
        sel = np.sort(np.append(sel[sel != e], f))
    x0, x1 = E.indicator(m, start), E.indicator(m, sel)
    ld0 = X.logdet_dense(X.M_of(g, np.zeros(m)))
    F0, F1 = X.objective(g, x0, ld0), X.objective(g, x1, ld0)
    tol, d, _ = X.F_tolerance(g, x1)
    print(f"{tag}: growth={info['growth']:.15g} F(start)={F0:.15g} F(final)={F1:.15g} |err|={abs(info['growth'] + F0 - F1):.3e} tol={tol:.3e} d={d:.3e}")
    assert abs(info["growth"] + F0 - F1) <= tol
    assert info["growth"] == float(np.sum(np.log(info["ratios"])))
    return sel


def check_swap_optimal(tag, g, sel):
    first, _ = E.best_swap(g, sel)
    _, tol = E.log_ratio_check(g, sel, first[1], first[2])
    print(f"{tag}: best Delta - 1 of the final selection = {first[0] - 1.0:.3e} (pair {first[1]}, {first[2]}), min_gain={MIN_GAIN:.0e} tol={tol:.3e}")
    assert first[0] - 1.0 <= MIN_GAIN + tol


# ---- 1. Petersen ----
def test_petersen_takes_the_one_swap_of_the_restatement():
    g = X.petersen()
    start = naive_start(g, 2)
    ref = E.from_scratch(g, start, 20)
    result, sel_edges, info = greedy_of(g).exchange(start)
    check_sequence("petersen", info, result, ref)
    assert info["swaps"] == 1 and info["converged"] is True
    assert [(e.i, e.j) for e in sel_edges] == [(int(g[4][q]), int(g[5][q])) for q in ref["selection"]]
    check_ratios("petersen", g, start, info)
    assert info["seconds"] > 0.0


# ---- 2. general500 from the greedy's selection ----
@pytest.mark.parametrize("k", [164, 273])
def test_general500_from_the_greedy_start_follows_the_restatement(k):
    g = X.random_general()
    ge = greedy_of(g)
    assert ge.info()["form"] == "dense" and ge.info()["ld"] == 512
    start = greedy_start(ge, g, k)
    ref = E.incremental(g, start, 10 * k)
    result, _, info = ge.exchange(E.indicator(len(g[6]), start))      # (a 0/1 array here, indices elsewhere)
    check_sequence(f"general500 K={k}", info, result, ref)
    final = check_ratios(f"general500 K={k}", g, start, info)
    check_swap_optimal(f"general500 K={k}", g, final)
    wr, wr_ref = ge.weighted_resistances(), X.gradient(g, result)
    print(f"general500 K={k}: resistances after the exchange, max err={np.max(np.abs(wr - wr_ref)):.3e} max={np.max(wr_ref):.6g}")
    assert np.max(np.abs(wr - wr_ref)) <= GRAD_RTOL * np.max(wr_ref)


# ---- 3. many updates across many folds ----
def test_general500_from_the_naive_start_across_ten_folds():
    g = X.random_general()
    ge = greedy_of(g, fold=8)
    start = naive_start(g, 164)
    ref = E.from_scratch(g, start, 40)
    result, _, info = ge.exchange(start, max_swaps=40)
    check_sequence("general500 naive fold=8", info, result, ref)
    assert info["converged"] is False and info["swaps"] == 40
    check_ratios("general500 naive fold=8", g, start, info)


# ---- 4. intel, both dense forms ----
def test_intel_chain_and_dense_forms_take_the_same_swaps():
    g = intel()
    m = len(g[6])
    k = m // 3
    chain, dense = greedy_of(g), greedy_of(g, dense_inverse=True)
    assert chain.info()["form"] == "chain" and dense.info()["form"] == "dense"
    start = np.flatnonzero(chain.subset(k)[0])
    ra, _, ia = chain.exchange(start)
    rb, _, ib = dense.exchange(start)
    print(f"intel K={k}: chain swaps={ia['swaps']} out={list(ia['out'])} in={list(ia['in'])} growth={ia['growth']:.12g}")
    print(f"intel K={k}: dense swaps={ib['swaps']} out={list(ib['out'])} in={list(ib['in'])} growth={ib['growth']:.12g}")
    assert ia["swaps"] >= 1                                        # (43 in the restatement: test_esp_exchange_host.py)
    assert list(ia["out"]) == list(ib["out"]) and list(ia["in"]) == list(ib["in"]) and np.array_equal(ra, rb)
    assert ia["converged"] is True and ib["converged"] is True
    final = check_ratios("intel chain", g, start, ia)
    check_ratios("intel dense", g, start, ib, per_swap=False)      # (the same swaps: their CPU ratios are the ones just compared)
    print(f"intel: largest |ratio chain / ratio dense - 1| = {np.max(np.abs(ia['ratios'] / ib['ratios'] - 1.0)):.3e}")
    check_swap_optimal("intel", g, final)


# ---- 5. exact ties ----
def test_ties_go_to_the_lowest_pair_and_no_edge_is_exchanged_for_its_twin():
    g = E.twins()
    start = naive_start(g, 10)
    ref = E.from_scratch(g, start, 100)
    ge = greedy_of(g)
    result, _, info = ge.exchange(start)
    check_sequence("twins", info, result, ref)
    assert all(e // 2 != f // 2 for e, f in zip(info["out"], info["in"]))
    assert all(f % 2 == 0 for f in info["in"])                     # of two tied twins the lower index enters
    s = ge.weighted_resistances()
    assert np.array_equal(s[0::2], s[1::2])                        # twins score the same bits, whatever was selected


# ---- 6. the edges of the index space ----
@pytest.mark.parametrize("n", [65, 66])
def test_awkward_shapes_follow_the_restatement(n):
    g = E.awkward(n)
    m = len(g[6])
    ge = greedy_of(g)
    assert ge.info()["ld"] == (64 if n == 65 else 128)
    for k in (1, 37, m - 1):
        start = naive_start(g, k)
        ref = E.from_scratch(g, start, 10 * k)
        result, _, info = ge.exchange(start)
        check_sequence(f"awkward n={n} K={k}", info, result, ref)
        assert 5 not in info["in"]                                 # the self-loop
        check_ratios(f"awkward n={n} K={k}", g, start, info)
    # max_swaps = 0: the selection is loaded and returned
    start = naive_start(g, 37)
    result, sel_edges, info = ge.exchange(start, max_swaps=0)
    assert np.array_equal(np.flatnonzero(result), start) and info["swaps"] == 0 and info["converged"] is False and len(info["ratios"]) == 0
    assert info["growth"] == 0.0 and len(sel_edges) == 37
    wr, wr_ref = ge.weighted_resistances(), X.gradient(g, E.indicator(m, start))
    print(f"awkward n={n}: resistances of the loaded selection, max err={np.max(np.abs(wr - wr_ref)):.3e} max={np.max(wr_ref):.6g}")
    assert np.max(np.abs(wr - wr_ref)) <= GRAD_RTOL * np.max(wr_ref)


# ---- 7. both row paths ----
def test_lds_and_global_rows_give_the_same_bits():
    g = X.random_general()
    for k in (164, 273):
        ge = greedy_of(g)
        start = greedy_start(ge, g, k)
        _, _, a = ge.exchange(start)
        with _lib.default_options(esp_xch_lds_kb=0):
            _, _, b = ge.exchange(start)
            _, _, c = greedy_of(g).exchange(start)
        print(f"rows K={k}: LDS out={list(a['out'])} ratios={[float(r).hex() for r in a['ratios']]}")
        print(f"rows K={k}: global out={list(b['out'])} ratios={[float(r).hex() for r in b['ratios']]}")
        for o in (b, c):
            assert a["swaps"] >= 1 and np.array_equal(a["out"], o["out"]) and np.array_equal(a["in"], o["in"])
            assert np.array_equal(a["ratios"], o["ratios"])


# ---- 8. repeatability and the handle afterwards ----
def test_runs_repeat_and_the_handle_stays_a_fresh_one_for_the_other_calls():
    g = X.random_general()
    k = 164
    m = len(g[6])
    start = naive_start(g, k)
    ge = greedy_of(g)
    r1, _, a = ge.exchange(start, max_swaps=12)
    r2, _, b = ge.exchange(start, max_swaps=12)
    print(f"repeat: ratios first={[float(r).hex() for r in a['ratios'][:3]]} second={[float(r).hex() for r in b['ratios'][:3]]}")
    assert a["swaps"] == 12 and np.array_equal(r1, r2)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["in"], b["in"]) and np.array_equal(a["ratios"], b["ratios"])
    fresh = greedy_of(g)
    o1, g1, _ = ge._dev.select([k])
    o0, g0, _ = fresh._dev.select([k])
    assert np.array_equal(o0, o1) and np.array_equal(g0, g1)
    assert ge.info() == fresh.info()
    n, fi, fj, fw, ci, cj, cw = g
    used, clean = ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n), ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n)
    used.exchange(start, max_swaps=12)
    x = np.random.default_rng(5).random(m)
    (F1, gr1), (F0, gr0) = used.problem(x), clean.problem(x)
    print(f"problem after an exchange: F={F1!r} fresh={F0!r}")
    assert F1 == F0 and np.array_equal(gr1, gr0)


# ---- 9. polishing the relaxation's rounded selection ----
def test_solve_with_exchange_polishes_the_rounded_selection():
    g = X.random_general()
    n, fi, fj, fw, ci, cj, cw = g
    k = 164
    x0 = NaiveGreedy(edges(ci, cj, cw)).subset(k)
    a, b = ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n), ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n)
    plain = a.solve(k, x0)
    again = b.solve(k, x0, exchange=False)
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1]) and plain[2] == again[2] and a.trace == b.trace
    polished = b.solve(k, x0, exchange=True)
    assert np.array_equal(polished[1], plain[1]) and polished[2] == plain[2]
    assert polished[0].shape == plain[0].shape and polished[0].sum() == k and set(np.unique(polished[0])) <= {0.0, 1.0}
    Fr, Fp = a.evaluate_objective(plain[0]), a.evaluate_objective(polished[0])
    print(f"solve K={k}: F(rounded)={Fr:.12g} F(polished)={Fp:.12g} upper={plain[2]:.12g}")
    assert Fp >= Fr and Fp <= plain[2]
    check_swap_optimal("solve", g, np.flatnonzero(polished[0]))


# ---- 10. errors ----
def test_bad_arguments_are_named():
    g = X.random_general()
    m = len(g[6])
    ge = greedy_of(g)
    dev = ge._dev
    good = np.arange(5)
    for sel, swaps, gain, msg in (([], 1, 1e-9, "k must be"), (np.arange(m), 1, 1e-9, "k must be"), ([0, m], 1, 1e-9, "outside"),
                                  ([-1, 3], 1, 1e-9, "outside"), ([3, 7, 3], 1, 1e-9, "more than once"), (good, -1, 1e-9, "max_swaps"),
                                  (good, 1, -1e-3, "min_gain"), (good, 1, np.nan, "min_gain"), (good, 1, np.inf, "min_gain")):
        with pytest.raises(AssertionError, match="BAD_ARG.*" + msg):
            dev.exchange(sel, swaps, gain)
    lib, buf, d, n, conv = dev._lib, np.zeros(8, dtype=np.int32), np.zeros(8), C.c_int64(0), C.c_int32(0)
    p, q = _lib.p_i32(buf), _lib.p_f64(d)
    for args in ((None, p, p, p, q, C.byref(n), C.byref(conv)), (p, None, p, p, q, C.byref(n), C.byref(conv)),
                 (p, p, None, p, q, C.byref(n), C.byref(conv)), (p, p, p, None, q, C.byref(n), C.byref(conv)),
                 (p, p, p, p, None, C.byref(n), C.byref(conv)), (p, p, p, p, q, None, C.byref(conv)), (p, p, p, p, q, C.byref(n), None)):
        st = lib.machip_esp_exchange(dev._h, 1, args[0], 2, 1e-9, args[1], args[2], args[3], args[4], args[5], args[6], None)
        assert st == _lib.BAD_ARG and "NULL" in _lib.last_error(), _lib.last_error()
    with _lib.default_options(esp_xch_max_mb=1):
        with pytest.raises(AssertionError, match=r"BAD_ARG.*300 x 512 x 8 = 1228800 bytes"):
            dev.exchange(np.arange(300), 1)
    assert ge.exchange(good, max_swaps=1)[2]["swaps"] == 1          # the handle is still good
    with pytest.raises(AssertionError, match="BAD_ARG.*beta"):
        greedy_of(X.disconnected())._dev.exchange(good, 1)
    chain = X.chain_er(60, 0.05, 1)
    for mf in (True, "tree"):
        free = greedy_of(chain, matrix_free=mf)
        with pytest.raises(ValueError, match="matrix_free"):
            free.exchange([0, 1])
        with pytest.raises(AssertionError, match="BAD_ARG.*MATRIX_FREE"):
            free._dev.exchange([0, 1], 1)
    with pytest.raises(ValueError, match="selection"):
        ge.exchange(np.array([0.5, 2.0]))
    d = X.disconnected()
    relax = ESPRelaxation(edges(d[1], d[2], d[3]), edges(d[4], d[5], d[6]), d[0])
    with pytest.raises(ValueError, match="beta"):                  # refused before the Frank-Wolfe run
        relax.solve(5, np.zeros(len(d[6])), exchange=True)
    assert relax.trace == []
