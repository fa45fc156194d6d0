"""The exchange in edge space on the GPU (mac_amd/csrc/esp_exchange_edge.h) against its NumPy restatement
(tests/esp_exchange_edge_restatement.py), through ``ESPRelaxation.exchange_edge``, ``solve(exchange="edge")`` and the handle
``_lib.Esp``.

Sequences are compared on the inputs tests/test_esp_exchange_edge_host.py keeps at least 1e-6 apart at every round (and, for the
tie graph, tied exactly).  Tolerances are those of tests/test_esp_exchange_gpu.py, whose checks are used as they are: a swap's
ratio against log det M' - log det M within the sum of esp_relax_restatement.F_tolerance at both selections; the growth within
F_tolerance at the final selection; brute-force swap-optimality of the final selection.  Beyond the dense limits there is no
n x n reference: the growth is compared with the difference of sparse-LU log-determinants within 10 max(d, 1e-13 |logdet|), d the
disagreement of that route and the edge restatement (the rule of test_beyond_the_node_forms_limit_matches_sparse_solves).
Every compared figure is printed before it is asserted (run with -s to see them)."""
import ctypes as C

import numpy as np
import pytest

import esp_edge_tree_restatement as T
import esp_exchange_edge_restatement as EE
import esp_exchange_restatement as E
import esp_relax_restatement as X
import esp_restatement as R
from mac_amd import _lib
from mac_amd.solvers import ESPRelaxation, GreedyESP
from mac_amd.utils.graphs import Edge
from test_esp_exchange_gpu import check_ratios, check_sequence, check_swap_optimal

pytestmark = pytest.mark.gpu

SEPARATION_FLOOR = 1e-6


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def relax_of(g, tree):
    n, fi, fj, fw, ci, cj, cw = g
    return ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n, edge_space="tree" if tree else True)


def greedy_of(g, **kw):
    n, fi, fj, fw, ci, cj, cw = g
    return GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


def restated(g, tree, start, cap=None):
    """The edge restatement's run from `start`; the comparison is only made where its rounds are decided by more than rounding."""
    ref = EE.run(g, tree, start, 10 * len(start) if cap is None else cap)
    print(f"restatement: swaps={len(ref['out'])} converged={ref['converged']} smallest separation={min(ref['separations']):.3e}")
    assert min(ref["separations"]) >= SEPARATION_FLOOR
    return ref


def follow(tag, g, tree, start, ld, relax=None):
    """exchange_edge from `start` against the restatement: the sequence, every swap's ratio, the growth, swap-optimality."""
    relax = relax or relax_of(g, tree)
    ref = restated(g, tree, start)
    result, sel_edges, info = relax.exchange_edge(start)
    assert relax.info()["relax_ld"] == ld
    check_sequence(tag, info, result, ref)
    assert [(e.i, e.j) for e in sel_edges] == [(int(g[4][q]), int(g[5][q])) for q in ref["selection"]]
    final = check_ratios(tag, g, start, info)
    check_swap_optimal(tag, g, final)
    return relax, info


# ---- 1. chain form ----
@pytest.mark.parametrize("k", [28, 42])
@pytest.mark.parametrize("start", ["naive", "greedy"])
def test_chain_form_follows_the_restatement(k, start):
    g = X.chain_er(60, 0.05, 1)
    assert len(g[6]) == 85
    if start == "greedy":
        sel = np.flatnonzero(greedy_of(g, matrix_free=True).subset(k)[0])
        assert np.array_equal(sel, E.greedy_start(g, k))
    else:
        sel = E.naive_start(g, k)
    relax, _ = follow(f"chain60 {start} K={k}", g, False, sel, 128)
    assert relax.info()["relax_form"] == "edge"


# ---- 2. tree form with seeds ----
@pytest.mark.parametrize("case,ks,M,ld", [("tree40", ("m//3", 1, "m-1"), 76, 128), ("awkward12", (1, 4, "m-1"), 16, 64),
                                          ("rt70", ("m//3",), 128, 128), ("rt130deep", ("m//3",), 199, 256)])
def test_tree_form_with_seeds_follows_the_restatement(case, ks, M, ld):
    g = {"tree40": T.tree40, "awkward12": T.awkward12, "rt70": lambda: T.random_tree(70, 5, 123, 7),
         "rt130deep": lambda: T.random_tree(130, 9, 190, 9, deep=40)}[case]()
    m = len(g[6])
    relax = relax_of(g, True)
    assert m + relax.info()["seeds"] == M and relax.info()["relax_form"] == "edge_tree"
    for k in ks:
        k = {"m//3": m // 3, "m-1": m - 1}.get(k, k)
        _, info = follow(f"{case} K={k}", g, True, E.naive_start(g, k), ld, relax)
        loops = np.flatnonzero(np.asarray(g[4]) == np.asarray(g[5]))
        assert not set(loops.tolist()) & set(int(f) for f in info["in"])          # a self-loop is never swapped in


# ---- 3. intel with 50 closures fixed, against the restatement and against the dense exchange ----
def test_intel_fixed50_from_the_greedy_start_takes_the_swaps_of_the_dense_exchange():
    g = T.intel_fixed50()
    k = 245
    dense = greedy_of(g)
    start = np.flatnonzero(dense.subset(k)[0])
    _, info = follow(f"intel50 K={k}", g, True, start, 832)
    assert info["swaps"] > 64 // 2 and info["converged"] is True     # (41 in the restatement from the restated greedy's start: more than one fold of swaps)
    _, _, idn = dense.exchange(start)
    assert dense.info()["ld"] == 1728
    print(f"intel50 K={k}: dense swaps={idn['swaps']} out={list(idn['out'])} in={list(idn['in'])} growth={idn['growth']:.12g}")
    assert list(idn["out"]) == list(info["out"]) and list(idn["in"]) == list(info["in"]) and idn["converged"] is True
    print(f"intel50: largest |ratio edge / ratio dense - 1| = {np.max(np.abs(info['ratios'] / idn['ratios'] - 1.0)):.3e}")


# ---- 4. exact ties ----
def test_ties_go_to_the_lowest_pair():
    g = E.twins()
    start = E.naive_start(g, 20)
    ref = EE.run(g, True, start, 200)
    relax = relax_of(g, True)
    result, _, info = relax.exchange_edge(start)
    check_sequence("twins", info, result, ref)
    assert all(e // 2 != f // 2 for e, f in zip(info["out"], info["in"]))
    assert all(f % 2 == 0 for f in info["in"])                     # of two tied twins the lower index enters
    check_ratios("twins", g, start, info)


# ---- 5. beyond every dense limit ----
@pytest.mark.parametrize("case", ["chain100k", "tree40k", "tree40kdeep"])
def test_beyond_every_dense_limit_follows_the_restatement_and_sparse_logdets(case):
    """Measured on the MI355X: |growth - sparse LU| = 2.2e-9 (chain100k, tol 1.6e-8), 4.1e-13 (tree40k) and 2.8e-12 (tree40kdeep,
    tol 6.6e-9 both).  The chain is the hard one: G's entries reach 9.2e4 there while 1 - s_e of the selected edges goes down to
    4.1e-4 (k_esp_xe_entered)."""
    tree = case != "chain100k"
    g = EE.long_chain(100_000, 300, 41) if not tree else EE.large_tree(case == "tree40kdeep")
    m, k = len(g[6]), 100
    start = E.naive_start(g, k)
    ref = restated(g, tree, start)
    relax = relax_of(g, tree)
    result, _, info = relax.exchange_edge(start)
    assert relax.info()["relax_ld"] == 320
    check_sequence(case, info, result, ref)
    if case == "chain100k":
        assert info["swaps"] == 23
    ld1 = R.logdet_sparse(X.M_of(g, result, sparse=True))
    sparse = ld1 - R.logdet_sparse(X.M_of(g, E.indicator(m, start), sparse=True))
    edge = float(np.sum(np.log(ref["ratios"])))
    d = abs(sparse - edge)
    tol = 10.0 * max(d, 1e-13 * abs(ld1))
    print(f"{case}: growth dev={info['growth']:.15g} sparse LU={sparse:.15g} edge restatement={edge:.15g} "
          f"|dev - sparse|={abs(info['growth'] - sparse):.3e} |dev - edge|={abs(info['growth'] - edge):.3e} tol={tol:.3e} d={d:.3e} logdet={ld1:.15g}")
    assert abs(info["growth"] - sparse) <= tol and abs(info["growth"] - edge) <= tol


# ---- 6. repeatability and the handle afterwards ----
@pytest.mark.parametrize("tree", [False, True])
def test_runs_repeat_and_the_handle_stays_a_fresh_one_for_the_other_calls(tree):
    g = T.random_tree(70, 5, 123, 7) if tree else X.chain_er(60, 0.05, 1)
    m = len(g[6])
    k = m // 3
    start = E.naive_start(g, k)
    used, fresh = relax_of(g, tree), relax_of(g, tree)
    r1, _, a = used.exchange_edge(start)                              # the first call on the handle
    r2, _, b = used.exchange_edge(start)
    print(f"repeat: ratios first={[float(r).hex() for r in a['ratios'][:3]]} second={[float(r).hex() for r in b['ratios'][:3]]}")
    assert a["swaps"] >= 1 and np.array_equal(r1, r2)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["in"], b["in"]) and np.array_equal(a["ratios"], b["ratios"])
    x = np.random.default_rng(5).random(m)
    (F1, gr1), (F0, gr0) = used.problem(x), fresh.problem(x)
    print(f"problem after an exchange: F={F1!r} fresh={F0!r}")
    assert F1 == F0 and np.array_equal(gr1, gr0)
    r3, _, c = used.exchange_edge(start)                              # and after relaxation calls
    assert np.array_equal(r1, r3) and np.array_equal(a["ratios"], c["ratios"])
    o1, g1, _ = used._dev.select([k])
    o0, g0, _ = fresh._dev.select([k])
    assert np.array_equal(o0, o1) and np.array_equal(g0, g1)
    assert np.array_equal(used._dev.weighted_resistances(), fresh._dev.weighted_resistances())
    r4, _, d = used.exchange_edge(start)                              # and after a greedy run
    assert np.array_equal(r1, r4) and np.array_equal(a["ratios"], d["ratios"])
    o2, g2, _ = used._dev.select([k])
    assert np.array_equal(o0, o2) and np.array_equal(g0, g2)
    result, sel_edges, info = used.exchange_edge(start, max_swaps=0)
    assert np.array_equal(np.flatnonzero(result), start) and info["swaps"] == 0 and info["converged"] is False and len(info["ratios"]) == 0
    assert info["growth"] == 0.0 and len(sel_edges) == k


# ---- 7. polishing the relaxation's rounded selection ----
def test_solve_with_exchange_edge_polishes_the_rounded_selection():
    g = T.intel_fixed50()
    m, k = len(g[6]), 245
    x0 = E.indicator(m, E.naive_start(g, k))
    a, b = relax_of(g, True), relax_of(g, True)
    plain = a.solve(k, x0)
    polished = b.solve(k, x0, exchange="edge")
    assert np.array_equal(polished[1], plain[1]) and polished[2] == plain[2] and a.trace == b.trace
    assert polished[0].shape == plain[0].shape and polished[0].sum() == k and set(np.unique(polished[0])) <= {0.0, 1.0}
    Fr, Fp = a.evaluate_objective(plain[0]), a.evaluate_objective(polished[0])
    tol = X.F_tolerance(g, polished[0])[0]
    print(f"solve K={k}: F(rounded)={Fr:.12g} F(polished)={Fp:.12g} upper={plain[2]:.12g} tol={tol:.3e}")
    assert Fp >= Fr and Fp <= plain[2] + tol
    check_swap_optimal("solve", g, np.flatnonzero(polished[0]))


# ---- 8. errors ----
def test_bad_arguments_are_named():
    g = T.intel_fixed50()
    m = len(g[6])
    relax = relax_of(g, True)
    dev = relax._dev
    good = np.arange(5)
    for sel, swaps, gain, msg in (([], 1, 1e-9, "k must be"), (np.arange(m), 1, 1e-9, "k must be"), ([0, m], 1, 1e-9, "outside"),
                                  ([-1, 3], 1, 1e-9, "outside"), ([3, 7, 3], 1, 1e-9, "more than once"), (good, -1, 1e-9, "max_swaps"),
                                  (good, 1, -1e-3, "min_gain"), (good, 1, np.nan, "min_gain")):
        with pytest.raises(AssertionError, match="BAD_ARG.*" + msg):
            dev.exchange_edge(sel, swaps, gain)
    lib, buf, d, n, conv = dev._lib, np.zeros(8, dtype=np.int32), np.zeros(8), C.c_int64(0), C.c_int32(0)
    p, q = _lib.p_i32(buf), _lib.p_f64(d)
    for args in ((None, p, p, p, q, C.byref(n), C.byref(conv)), (p, None, p, p, q, C.byref(n), C.byref(conv)),
                 (p, p, None, p, q, C.byref(n), C.byref(conv)), (p, p, p, None, q, C.byref(n), C.byref(conv)),
                 (p, p, p, p, None, C.byref(n), C.byref(conv)), (p, p, p, p, q, None, C.byref(conv)), (p, p, p, p, q, C.byref(n), None)):
        st = lib.machip_esp_exchange_edge(dev._h, 1, args[0], 2, 1e-9, args[1], args[2], args[3], args[4], args[5], args[6], None)
        assert st == _lib.BAD_ARG and "NULL" in _lib.last_error(), _lib.last_error()
    with _lib.default_options(esp_xch_max_mb=1):
        with pytest.raises(AssertionError, match=r"BAD_ARG.*245 x 832 x 8 = 1630720 bytes.*esp_xch_max_mb"):
            dev.exchange_edge(np.arange(245), 1)
    assert relax.exchange_edge(good, max_swaps=1)[2]["swaps"] == 1          # the handle is still good
    with pytest.raises(AssertionError, match="BAD_ARG.*MATRIX_FREE"):      # the dense entry point keeps refusing this handle
        dev.exchange(good, 1)
    chain = X.chain_er(60, 0.05, 1)
    n_, fi, fj, fw, ci, cj, cw = chain
    node = ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n_)
    with pytest.raises(ValueError, match="edge_space"):
        node.exchange_edge([0, 1])
    for other in (node._dev, greedy_of(chain, matrix_free=True)._dev, greedy_of(chain, matrix_free="tree")._dev):
        with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_EDGE_RELAX"):
            other.exchange_edge([0, 1], 1)
    with pytest.raises(ValueError, match="selection"):
        relax.exchange_edge(np.array([0.5, 2.0]))
