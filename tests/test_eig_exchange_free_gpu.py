"""GreedyEig.exchange_free on the GPU (mac_amd/csrc/eig_exchange_free.h, the matrix-free members of eig_routes.h) against the NumPy
restatements of its rules (tests/eig_exchange_restatement.py: the rounds; tests/eig_exchange_free_restatement.py: the history).

Tolerances.  Those of tests/test_eig_exchange_gpu.py for everything a round decides: a reported value is within tolL = 1e-8 ||L||_inf
of an eigenvalue of its L, a swap may fall short of the round's maximum by 1e-8 + 2 tolL, and a sequence is pinned only where the
brute-force gaps are at least 100 times that (tests/test_eig_exchange_free_host.py checks the same on the CPU).
The history: Sigma0 - Z diag(c) Z^T against numpy.linalg.inv(L_S[1:, 1:]), largest entry of the difference over largest entry of the
inverse, at 1 000 times the error the NumPy restatement of the same sequence of loads, swaps and compactions shows against the same
inverse.  The restatement's error is computed with the test; measured on the CPU it is 4.5e-13 (chain300 K = 40), 5.9e-13 (K = 100;
5.5e-13 over the spanning tree), 2.9e-13 (K = 1), 2.4e-15 (general80 K = 10: 39 seeds, the fixed links outside the tree that are
distinct), 6.5e-15 / 1.3e-15 / 1.4e-15 ((c) after its eleven swaps with room for 32 / 2 / 1 swaps between compactions): bounds of
1.3e-12 to 5.9e-10, where a wrong coefficient or a column out of place is an error of order 1."""
import functools

import numpy as np
import pytest

import eig_exchange_free_restatement as X
import eig_exchange_restatement as E
import eig_restatement as R
from mac_amd import _lib
from mac_amd.solvers import MAC
from test_eig_gpu import chain_er, edges, petersen, random_general
import test_eig_gpu

pytestmark = pytest.mark.gpu

_made = []


def eig_of(g, matrix_free="tree", **kw):
    ge = test_eig_gpu.eig_of(*g, matrix_free=matrix_free, **kw)
    _made.append(ge)
    return ge


@pytest.fixture(autouse=True)
def no_handle_outlives_its_test():
    """Every handle a test of this module makes is destroyed when the test ends."""
    yield
    for obj in _made:
        for name in ("_greedy_eig", "_greedy_eig_free"):
            inner = getattr(obj, name, None)
            if inner is not None:
                inner._dev.close()
        obj._dev.close()
    _made.clear()


def indices(sol):
    return [int(e) for e in np.flatnonzero(sol)]


def tol_of(g, sel):
    return 1e-8 * R.norm_inf(E.lap_of(g, sel))


@functools.lru_cache(maxsize=None)
def pinned(case):
    """(graph, start, the brute-force run, tol) of (a) chain_er(40, 0.1, 1) from the greedy start, (b) chain_er(40, 0.1, 2) with five
    closures from the naive start, (c) chain_er(40, 0.1, 1) with five closures from the greedy start; K = 8."""
    if case == "a":
        g = chain_er(40, 0.1, 1)
        start = E.greedy_start(g, 8)
    elif case == "b":
        g = X.with_closures(chain_er(40, 0.1, 2), 5)
        start = E.naive_start(g, 8)
    else:
        g = X.with_closures(chain_er(40, 0.1, 1), 5)
        start = E.greedy_start(g, 8)
    run = E.brute(g, start, 100)
    tol = 1e-8 + 2e-8 * max(r["norm"] for r in run["rounds"])
    gaps = [r["best"] - r["second"] for r in run["rounds"]]
    last = abs(run["rounds"][-1]["best"] - (run["rounds"][-1]["tau"] + 1e-8))
    assert min(gaps) >= 100 * tol and last >= 100 * tol, (case, gaps, last, tol)      # the precondition: a seed that loses it fails here
    return g, start, run, tol


def sigma0_and_seeds(g, matrix_free):
    """What the route's history corrects: the chain's inverse and no seeds, or the spanning tree's and the links outside it."""
    n, fi, fj, fw = g[:4]
    if matrix_free is True:
        return X.sigma0_of(n, fi, fj, fw), (np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0))
    plan = _lib.host_esp_tree(n, fi, fj, fw)
    return X.sigma0_of(n, *X.tree_edges(plan["parent"], plan["R"])), plan["seeds"]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def check_history(ge, g, matrix_free, start, swaps=(), C=32, converged=True):
    """The handle's history is the inverse of L_S, as closely as the restatement's own (times 1 000), and has its number of columns."""
    n = g[0]
    S0, seeds = sigma0_and_seeds(g, matrix_free)
    rows = sorted(start)
    for e, f in swaps:
        rows[rows.index(e)] = f
    inv = np.linalg.inv(E.lap_of(g, rows)[1:, 1:])
    Zr, cr = X.history_after(g, S0, seeds, start, swaps, C, converged)
    own = rel(X.implied_inverse(S0, Zr, cr), inv)
    Z, c = ge._dev.history()
    inf = ge.info()
    assert Z.shape == (inf["ld"], inf["pending"]) and c.shape == (inf["pending"],) and Z.shape[1] == Zr.shape[1]
    assert np.all(Z[n - 1:] == 0.0)                                     # rows n' .. ld are written as 0
    err = rel(X.implied_inverse(S0, Z[:n - 1], c), inv)
    print(f"history: {Z.shape[1]} columns, error {err:.2e}, the restatement's {own:.2e}, columns against the restatement's {rel(Z[:n - 1], Zr):.2e}")
    assert own < 1e-11 and err <= 1000 * own
    return err


# ---- 1. the pinned sequences ----
@pytest.mark.parametrize("case,matrix_free", [("a", True), ("a", "tree"), ("b", "tree"), ("c", "tree")])
def test_pinned_sequence_equals_brute_force_and_the_dense_exchange(case, matrix_free):
    g, start, run, tol = pinned(case)
    ge = eig_of(g, matrix_free)
    assert ge.info()["seeds"] == (0 if case == "a" else 5)
    sol, sel, info = ge.exchange_free(start)
    print(case, matrix_free, "swaps", info["swaps"], "lambda2", info["lambda2"], "solved", info["solved"], "applies", info["applies"])
    assert len(run["swaps"]) == {"a": 6, "b": 4, "c": 11}[case] and info["swaps"] == run["swaps"] and info["converged"] is True
    assert np.allclose(info["lambda2"], run["lambda2"], rtol=0, atol=tol)
    assert indices(sol) == run["selection"] and [(e.i, e.j) for e in sel] == [(int(g[4][e]), int(g[5][e])) for e in run["selection"]]
    assert run["rounds"][-1]["swap"] is None                           # brute force finds no improving swap from the result
    rounds = len(info["swaps"]) + 1
    assert len(info["solved"]) == len(info["applies"]) == len(info["removal_solves"]) == rounds and info["compactions"] == 0
    assert np.all(info["removal_solves"] == 8) and np.all(info["solved"] <= 8 * (len(g[6]) - 8)) and np.all(info["solved"] >= 1)
    assert np.all(info["applies"] >= info["solved"]) and info["t_ms"][0] > 0 and info["t_ms"][1] > 0
    assert ge.info()["pending"] == ge.info()["seeds"] + 8 + 2 * len(run["swaps"])
    dense = eig_of(g, False)
    d = dense.exchange(start)[2]
    assert d["swaps"] == info["swaps"] and d["converged"] is True and "compactions" not in d
    assert np.allclose(d["lambda2"], info["lambda2"], rtol=0, atol=tol)


# ---- 2. compaction ----
@pytest.mark.parametrize("C", [2, 1])
def test_compactions_follow_the_rule_and_change_no_swap(C):
    g, start, run, tol = pinned("c")
    ge = eig_of(g)
    plain = ge.exchange_free(start)[2]
    assert plain["compactions"] == 0 and plain["swaps"] == run["swaps"]
    assert ge.info()["pending"] == X.compaction_rule(8, 5, 32, 11)[1] == 5 + 8 + 22
    with _lib.default_options(eig_xch_free_swaps=C):
        sol, _, info = ge.exchange_free(start)
    want, pending = X.compaction_rule(8, 5, C, 11)
    print("C", C, "compactions", info["compactions"], "pending", ge.info()["pending"], "rule", (want, pending))
    assert want >= 5 and info["compactions"] == want and ge.info()["pending"] == pending
    assert info["swaps"] == run["swaps"] and info["converged"] is True and indices(sol) == run["selection"]
    assert np.allclose(info["lambda2"], run["lambda2"], rtol=0, atol=tol)
    check_history(ge, g, "tree", start, run["swaps"], C=C)
    capped = ge.exchange_free(start, max_swaps=3)[2]                  # C = min(max_swaps, the option): the default 32 is cut to 3
    assert capped["swaps"] == run["swaps"][:3] and capped["compactions"] == 0 and ge.info()["pending"] == 5 + 8 + 6


# ---- 3. the history is the inverse ----
@pytest.mark.parametrize("name,K,matrix_free", [("chain300", 40, True), ("chain300", 100, True), ("chain300", 1, True), ("chain300", 100, "tree"),
                                                ("general80", 10, "tree")])
def test_the_loaded_history_is_the_inverse(name, K, matrix_free):
    """max_swaps = 0 loads and stops: K = 40 is one short block, K = 100 a full block of 64 and a short one, K = 1 a block of one;
    general80 has its seeds in front of its block."""
    g = chain_er(300, 0.03, 0) if name == "chain300" else random_general(80, 60, 4)
    start = E.naive_start(g, K)
    ge = eig_of(g, matrix_free)
    seeds = ge.info()["seeds"]      # (general80: 40 fixed links beside the random tree's 79, 39 of them distinct links outside the spanning tree)
    assert seeds == (len(_lib.host_esp_tree(*g[:4])["seeds"][2]) if matrix_free == "tree" else 0) and seeds == (39 if name == "general80" else 0)
    sol, _, info = ge.exchange_free(start, max_swaps=0)
    assert info["swaps"] == [] and info["compactions"] == 0 and indices(sol) == start and ge.info()["pending"] == seeds + K
    assert abs(info["lambda2"][0] - R.fiedler(E.lap_of(g, start))[0]) <= tol_of(g, start)
    check_history(ge, g, matrix_free, start, converged=False)


def test_the_history_after_a_full_run_is_the_inverse():
    g, start, run, tol = pinned("c")
    ge = eig_of(g)
    assert ge.exchange_free(start)[2]["swaps"] == run["swaps"]
    check_history(ge, g, "tree", start, run["swaps"])
    with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_EIG_MATRIX_FREE"):
        eig_of(g, False)._dev.history()


# ---- 4. replay validity where the gaps are not pinned ----
@pytest.mark.parametrize("name,k,cap", [("general80", 10, 4), ("petersen", 1, None), ("petersen", 5, None)])
def test_every_swap_is_a_maximiser_on_replay(name, k, cap):
    g = random_general(80, 60, 4) if name == "general80" else petersen()
    m = len(g[6])
    assert k < m and (name != "petersen" or k in (1, m - 1))
    start = E.naive_start(g, k)
    ge = eig_of(g)
    sol, sel, info = ge.exchange_free(start, max_swaps=cap)
    lam = info["lambda2"]
    print(name, k, "swaps", info["swaps"], "lambda2", lam, "converged", info["converged"], "solved", info["solved"])
    assert len(lam) == len(info["swaps"]) + 1 and np.all(np.diff(lam) > 0)
    if name != "petersen":
        assert len(info["swaps"]) == cap and not info["converged"]
    rows = list(start)
    assert abs(lam[0] - R.fiedler(E.lap_of(g, rows))[0]) <= tol_of(g, rows)
    for t, (e, f) in enumerate(info["swaps"]):
        assert e in rows and f not in rows
        r = E.brute_round(g, sorted(rows))
        tau, best = r["tau"], r["best"]
        rows[rows.index(e)] = f
        tolL = tol_of(g, rows)
        exact = R.fiedler(E.lap_of(g, rows))[0]
        print(name, t, "shortfall", float(best - exact), "lambda2 err / tol", float(abs(lam[t + 1] - exact) / tolL))
        assert abs(lam[t + 1] - exact) <= tolL
        assert exact >= best - 1e-8 - 2 * tolL and exact > tau
    assert indices(sol) == sorted(rows)
    if info["converged"]:
        r = E.brute_round(g, sorted(rows))
        assert r["best"] <= r["tau"] + 1e-8 + 2 * tol_of(g, rows)


# ---- 5. batches ----
@pytest.mark.parametrize("matrix_free", [True, "tree"])
def test_small_batches_unchanged(matrix_free):
    """K = 20 from the naive start with batch = 16: the removal columns take two batches, the survivors of a row several; the
    blocked load works on 64 columns whatever the batch."""
    g = chain_er(40, 0.1, 1)
    start = E.naive_start(g, 20)
    a, b = eig_of(g, matrix_free), eig_of(g, matrix_free, batch=16)
    (sa, _, ia), (sb, _, ib) = a.exchange_free(start), b.exchange_free(start)
    print("K=20 swaps", ia["swaps"], "solved (default)", ia["solved"], "solved (batch 16)", ib["solved"])
    assert len(ia["swaps"]) >= 1 and ia["swaps"] == ib["swaps"] and ia["converged"] == ib["converged"] and np.array_equal(sa, sb)
    assert np.all(np.abs(ia["lambda2"] - ib["lambda2"]) <= 2 * tol_of(g, np.arange(len(g[6]))))
    assert np.all(ib["solved"] <= ia["solved"])


# ---- 6. state and arguments ----
@pytest.mark.parametrize("matrix_free", [True, "tree"])
def test_runs_repeat_bit_for_bit_and_leave_the_handle_as_new(matrix_free):
    g, start, run, tol = pinned("a")
    ge, fresh = eig_of(g, matrix_free), eig_of(g, matrix_free)
    a = ge.exchange_free(start)
    b = ge.exchange_free(start)
    c = fresh.exchange_free(np.isin(np.arange(len(g[6])), start).astype(float))      # the 0/1 form of the same selection
    ha, hc = ge._dev.history(), fresh._dev.history()
    assert np.array_equal(ha[0], hc[0]) and np.array_equal(ha[1], hc[1])             # the history too
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and a[1] == x[1] and a[2]["swaps"] == x[2]["swaps"] and a[2]["converged"] == x[2]["converged"]
        assert np.array_equal(a[2]["lambda2"], x[2]["lambda2"])         # bit for bit
        for key in ("solved", "applies", "removal_solves"):
            assert np.array_equal(a[2][key], x[2][key])
    final = indices(a[0])
    inf = ge.info()
    assert inf["lambda2"] == a[2]["lambda2"][-1] and np.array_equal(inf["solved"], a[2]["solved"])
    L = E.lap_of(g, final)
    lam, u = ge.candidate_lambda2(), ge.candidate_bounds()
    ref = R.values_brute(L, g[4], g[5], g[6])
    uns = np.setdiff1d(np.arange(len(g[6])), final)
    assert np.all(np.isnan(lam[final])) and np.all(np.isnan(u[final]))
    assert np.all(np.abs(lam[uns] - ref[uns]) <= 1e-8 * R.norm_inf_with(L, g[4], g[5], g[6])[uns])
    assert np.all(np.abs(u[uns] - R.bounds(L, g[4], g[5], g[6])[uns]) <= 1e-5) and np.all(u[uns] >= lam[uns] - tol)
    new = eig_of(g, matrix_free)
    (s1, e1), (s0, e0) = ge.subset(8), new.subset(8)
    assert np.array_equal(s1, s0) and e1 == e0 and np.array_equal(ge.last_lambda2, new.last_lambda2)


def test_max_swaps_zero_loads_and_reports():
    g, start, run, tol = pinned("a")
    ge = eig_of(g, True)
    sol, sel, info = ge.exchange_free(start, max_swaps=0)
    assert info["swaps"] == [] and info["converged"] is False and len(info["lambda2"]) == 1 and len(info["solved"]) == 0
    assert abs(info["lambda2"][0] - run["lambda2"][0]) <= tol and indices(sol) == sorted(start) and info["compactions"] == 0
    assert ge.info()["lambda2"] == info["lambda2"][0]
    one = ge.exchange_free(start, max_swaps=1)[2]
    assert one["swaps"] == run["swaps"][:1] and one["converged"] is False and len(one["solved"]) == 1


def test_bad_arguments_are_named_and_the_routes_keep_their_entries():
    g = chain_er(40, 0.1, 1)
    m = len(g[6])
    ge = eig_of(g, True)
    dev = ge._dev
    good = np.arange(5)
    for sel, swaps, gain, msg in (([], 1, 0.0, "k must be"), (np.arange(m), 1, 0.0, "k must be"), ([0, m], 1, 0.0, "outside"),
                                  ([-1, 3], 1, 0.0, "outside"), ([3, 7, 3], 1, 0.0, "more than once"), (good, -1, 0.0, "max_swaps"),
                                  (good, 1, -1e-3, "min_gain"), (good, 1, np.nan, "min_gain"), (good, 1, np.inf, "min_gain")):
        with pytest.raises(AssertionError, match="BAD_ARG.*" + msg):
            dev.exchange_free(sel, swaps, gain)
    st = dev._lib.machip_eig_exchange_free(dev._h, 5, None, 1, 0.0, None, None, None, None, None, None, None, None, None)
    assert st == _lib.BAD_ARG and "sel_in is NULL" in _lib.last_error()
    with _lib.default_options(eig_xch_max_mb=1):
        with pytest.raises(AssertionError, match=r"BAD_ARG.*8 x 100 x \(320 \+ 1324\) = 1315200 bytes.*eig_xch_max_mb"):
            eig_of(chain_er(300, 0.03, 0), True)._dev.exchange_free(np.arange(100), 1)
    buf = np.arange(5, dtype=np.int32)                                  # every output may be NULL; the handle is still good
    assert dev._lib.machip_eig_exchange_free(dev._h, 5, _lib.p_i32(buf), 1, 0.0, None, None, None, None, None, None, None, None, None) == _lib.OK
    assert len(ge.exchange_free(good, max_swaps=1)[2]["swaps"]) == 1
    with pytest.raises(ValueError, match="selection"):
        ge.exchange_free(np.array([0.5, 2.0]))
    # a dense handle is refused by both layers, and names the entry that works there
    dense = eig_of(g, False)
    with pytest.raises(ValueError, match="use exchange$"):
        dense.exchange_free(good)
    with pytest.raises(AssertionError, match="BAD_ARG.*machip_eig_exchange$"):
        dense._dev.exchange_free(good, 1)
    assert len(dense.exchange(good, max_swaps=1)[2]["swaps"]) == 1
    # exchange on a matrix-free handle is still refused
    for h in (ge, eig_of(g, "tree")):
        with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_EIG_MATRIX_FREE"):
            h.exchange(good)


# ---- 7. past the dense limits ----
def big(kind):
    rng = np.random.default_rng(7)
    m = 300
    if kind == "chain":
        n = 33000
        fi = np.arange(n - 1); fj = fi + 1
    else:
        n = 17000
        k = np.arange(1, n)
        xi = rng.integers(0, n, 20)
        fi, fj = np.concatenate([k, xi]), np.concatenate([rng.integers(0, k), (xi + rng.integers(1, n, 20)) % n])
    fw = rng.uniform(50.0, 200.0, len(fi))
    ci = rng.integers(0, n, m)
    cj = (ci + rng.integers(1, n, m)) % n
    return n, fi, fj, fw, ci, cj, rng.uniform(50.0, 200.0, m)


@pytest.mark.parametrize("kind", ["chain", "tree"])
def test_past_the_dense_limit_a_swap_reports_lambda2(kind):
    """n = 33 000 on the chain route, n = 17 000 (a random recursive tree plus 20 links) on the tree route: the dense routes refuse
    both.  The stop rule certifies values to 1e-8 ||L||_inf and, on a long chain, little more than that (Regime):
    the swap's identity is not asserted, the reported values are, against a sparse shift-invert solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    g = big(kind)
    n, fi, fj, fw, ci, cj, cw = g
    K = 3
    with pytest.raises(AssertionError, match="BAD_ARG.*" + ("32768" if kind == "chain" else "16384")):
        eig_of(g, False)
    ge = eig_of(g, True if kind == "chain" else "tree")
    assert ge.info()["seeds"] == (0 if kind == "chain" else 20)
    sol, sel, info = ge.exchange_free(np.arange(K), max_swaps=1)
    assert len(info["swaps"]) <= 1 and len(info["lambda2"]) == len(info["swaps"]) + 1 and len(sel) == K and sol.sum() == K

    def lap(sel):
        a = np.concatenate([fi, ci[sel]]); b = np.concatenate([fj, cj[sel]]); w = np.concatenate([fw, cw[sel]])
        A = sp.coo_matrix((w, (a, b)), shape=(n, n))
        A = A + A.T
        return (sp.diags(np.asarray(A.sum(axis=1)).ravel()) - A).tocsc()
    rows = list(range(K))
    sels = [list(rows)]
    for e, f in info["swaps"]:
        assert e in rows and f not in rows
        rows[rows.index(e)] = f
        sels.append(list(rows))
    assert indices(sol) == sorted(rows)
    got = info["lambda2"]
    for k, s in enumerate(sels):
        Lk = lap(np.array(s))
        norm = float(abs(Lk).sum(axis=1).max())
        ref = np.sort(spla.eigsh(Lk, k=2, sigma=-0.5 * got[k], which="LM", return_eigenvectors=False))[1]
        print(f"{kind} n = {n}, after {k} swaps: lambda_2 {got[k]:.6e}, shift-invert {ref:.6e}, |error| / (1e-8 ||L||_inf) "
              f"{abs(got[k] - ref) / (1e-8 * norm):.3e}, t_ms {info['t_ms']}")
        assert abs(got[k] - ref) <= 1e-8 * norm
        assert k == 0 or got[k] >= got[k - 1] - 1e-8 * norm


# ---- 8. MAC ----
def test_mac_exchange_free_and_solve_with_exchange_free():
    g, start, run, tol = pinned("a")
    n, fi, fj, fw, ci, cj, cw = g
    mac = MAC(edges(fi, fj, fw), edges(ci, cj, cw), n)
    _made.append(mac)
    sol, sel, info = mac.exchange_free(start)
    assert info["swaps"] == run["swaps"] and info["converged"] and E.brute_round(g, indices(sol))["swap"] is None
    assert mac._greedy_eig_free.info()["form"] == "tree_free" and mac._greedy_eig is None
    m, k = len(cw), 8
    x0 = np.zeros(m); x0[:k] = 1.0
    plain = mac.solve(k, x0)
    polished = mac.solve(k, x0, exchange="free")
    assert np.array_equal(polished[1], plain[1]) and polished[2] == plain[2] and len(polished) == 3      # unrounded and upper unchanged
    assert polished[0].sum() == k and set(np.unique(polished[0])) <= {0.0, 1.0}
    fr, fp = mac.evaluate_objective(plain[0]), mac.evaluate_objective(polished[0])
    print(f"solve K={k}: lambda_2(rounded)={fr:.9g} lambda_2(polished)={fp:.9g} upper={plain[2]:.9g} swaps={len(mac.exchange_info['swaps'])}")
    assert fp >= fr and mac.exchange_info["converged"] and "compactions" in mac.exchange_info
    assert E.brute_round(g, indices(polished[0]))["swap"] is None
    with pytest.raises(ValueError, match="invalid literal"):           # any other string goes through int(), as before
        mac.solve(k, x0, exchange="fre")
    capped = mac.solve(k, x0, exchange="2")
    assert len(mac.exchange_info["swaps"]) == 2 and "compactions" not in mac.exchange_info and capped[2] == plain[2]
