"""GreedyKirchhoff on the MI355X against its NumPy restatement (tests/kirchhoff_restatement.py) and brute-force pseudo-inverses.

Tolerance on gains and traces: max(16 x drift, 1e-10) relative, drift being the restatement's own distance between the gains its
recurrences kept and an exact re-scoring on that case (the cancellation in the q recurrence is real; the factor 16 covers the
different reduction order).  Observed on the MI355X: recorded gains within 5.7e-11 (chain-ER; drift 2.0e-10 to
3.1e-10), 3.4e-15 (general500; drift 1.2e-13) and 2.9e-9 (intel; drift 1.3e-7) of the restatement's."""
import functools

import numpy as np
import pytest

from conftest import load_golden
import kirchhoff_restatement as KR
from mac_amd import _lib
from mac_amd.solvers import GreedyESP, GreedyKirchhoff
from test_esp_gpu import arrays, chain_er, edges, petersen, random_general

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "petersen":
        return petersen()
    if name == "er65":
        return chain_er(65, 0.05, 2)
    if name == "er66":
        return chain_er(66, 0.05, 2)
    if name == "er130":
        return chain_er(130, 0.03, 5)
    if name == "general500":
        return random_general()
    return arrays(load_golden("g2o_intel"))


@functools.lru_cache(maxsize=None)
def restated(name, K, fold=64):
    """(order, gains, margins, drift, tolerance) of the restatement, computed once per setting."""
    order, gains, margins, drift = KR.greedy(*graph(name), K, fold=fold)
    for a in (order, gains, margins):
        a.setflags(write=False)
    return order, gains, margins, drift, max(16.0 * drift, 1e-10)


@functools.lru_cache(maxsize=None)
def exact_index(name, sel=()):
    n, fi, fj, fw, ci, cj, cw = graph(name)
    return KR.exact_trace(n, list(zip(fi, fj, fw)) + [(ci[e], cj[e], cw[e]) for e in sel])


def kir_of(name, **kw):
    n, fi, fj, fw, ci, cj, cw = graph(name)
    return GreedyKirchhoff(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


def rel_close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


# ---- 1. gains after create ----
@pytest.mark.parametrize("name,np_ld", [("petersen", (9, 64)), ("er65", (64, 64)), ("er66", (65, 128)), ("general500", (499, 512))])
def test_gains_after_create_match_restatement(name, np_ld):
    n, fi, fj, fw, ci, cj, cw = graph(name)
    gk = kir_of(name)
    inf = gk.info()
    assert (n - 1, inf["ld"]) == np_ld and inf["form"] == ("chain" if name.startswith("er") else "dense") and inf["beta"] == 0.0
    Sig, _ = KR.R.initial_sigma(n, fi, fj, fw)
    ref = KR.exact_scores(Sig, n, ci, cj, cw)[3]
    got = gk.gains()
    assert not np.isnan(got).any()
    loops = ci == cj
    assert np.all(got[loops] == 0.0)                                   # a self-loop: z = 0, gain exactly 0
    print(name, "max rel diff of the gains after create", np.max(np.abs(got - ref)[~loops] / np.abs(ref[~loops])))
    assert rel_close(got[~loops], ref[~loops], 1e-10)
    if name == "general500":                                           # a candidate and its reverse: the same bits
        rev = GreedyKirchhoff(edges(fi, fj, fw), edges(cj, ci, cw), n)
        assert np.array_equal(rev.gains(), got)


# ---- 2. the same picks as the restatement; gains, the trace identity ----
@pytest.mark.parametrize("name,fold,K", [("er130", 4, 60), ("er130", 64, 60), ("er130", 64, 64), ("er130", 64, 70),
                                         ("general500", 64, 50), ("intel", 64, 78)])
def test_same_picks_gains_and_trace_identity(name, fold, K):
    n, fi, fj, fw, ci, cj, cw = graph(name)
    order, gains, margins, drift, tol = restated(name, K, fold)
    assert margins.min() >= 1e-6
    gk = kir_of(name, fold=fold)
    res, sel = gk.subset(K)
    got = gk._dev.kirchhoff_select([K])[0]
    assert np.array_equal(got, order)
    ref = np.zeros(len(cw)); ref[order] = 1.0
    assert np.array_equal(res, ref)
    assert [(e.i, e.j, e.weight) for e in sel] == [(int(ci[e]), int(cj[e]), float(cw[e])) for e in order]
    print(name, fold, K, "drift", drift, "max rel diff of last_gains", np.max(np.abs(gk.last_gains - gains) / gains))
    assert rel_close(gk.last_gains, gains, tol)
    assert gk.info()["pending"] == K % fold
    after = gk.gains()                                                 # folds what is pending, re-scores everything exactly
    exact = KR.gains_after(n, fi, fj, fw, ci, cj, cw, order)
    big = np.abs(exact) > 0
    print(name, fold, K, "max rel diff of gains() after the run", np.max(np.abs(after - exact)[big] / np.abs(exact[big])))
    assert rel_close(after[big], exact[big], tol) and np.all(after[~big] == 0.0)
    base = gk.kirchhoff_index(None)
    with_sel = gk.kirchhoff_index(res)
    truth0, truth = exact_index(name), exact_index(name, tuple(int(e) for e in order))
    print(name, fold, K, "trace identity, relative to the fixed graph's:", (base - gk.last_gains.sum() - with_sel) / truth0,
          (with_sel - truth) / truth0, (base - truth0) / truth0)
    assert abs(base - truth0) <= tol * truth0
    assert abs(base - gk.last_gains.sum() - with_sel) <= tol * truth0
    assert abs(base - gk.last_gains.sum() - truth) <= tol * truth0
    assert abs(with_sel - truth) <= tol * truth0


# ---- 3. scoring other selections; order independence ----
def test_kirchhoff_index_scores_any_selection_in_any_order():
    name, K = "er130", 60
    n, fi, fj, fw, ci, cj, cw = graph(name)
    m = len(cw)
    tol = restated(name, K)[4]
    truth0 = exact_index(name)
    gk = kir_of(name, fold=16)
    esp_sel = np.flatnonzero(GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n).subset(K)[0])
    rnd = np.sort(np.random.default_rng(11).choice(m, K, replace=False))
    for sel in (esp_sel, rnd):
        truth = exact_index(name, tuple(int(e) for e in sel))
        a = gk.kirchhoff_index(sel)
        mask = np.zeros(m); mask[sel] = 1.0
        b = gk.kirchhoff_index(mask)
        c = gk.kirchhoff_index(np.random.default_rng(12).permutation(sel))
        assert a == b
        assert abs(a - truth) <= tol * truth0 and abs(c - truth) <= tol * truth0 and abs(a - c) <= tol * truth0
        assert a < gk.kirchhoff_index(None)
    assert abs(gk.kirchhoff_index([]) - truth0) <= tol * truth0
    with pytest.raises(AssertionError, match="twice"):
        gk.kirchhoff_index([3, 5, 3])
    with pytest.raises(AssertionError, match="out of range"):
        gk.kirchhoff_index([3, m])


# ---- 4. a duplicate candidate ----
def test_duplicate_candidate_lower_index_first_then_its_copy_drops():
    n, fi, fj, fw, ci, cj, cw = graph("er130")
    first = int(restated("er130", 60)[0][0])
    ci2, cj2, cw2 = np.append(ci, ci[first]), np.append(cj, cj[first]), np.append(cw, cw[first])
    m = len(cw2)
    order, gains, margins, _ = KR.greedy(n, fi, fj, fw, ci2, cj2, cw2, 2)
    assert order[0] == first and margins[0] == 0.0                      # an exact tie, decided by the index
    gk = GreedyKirchhoff(edges(fi, fj, fw), edges(ci2, cj2, cw2), n)
    g0 = gk.gains()
    assert g0[first] == g0[m - 1]
    got, gg, _ = gk._dev.kirchhoff_select([2])
    assert got[0] == first and got[1] == order[1] != m - 1
    g1 = gk._dev.kirchhoff_select([1])[1]
    assert g1[0] == g0[first]
    after = gk.gains()
    assert after[m - 1] < g0[m - 1] and after[m - 1] == after[first]


# ---- 5. forms, repeatability, budgets ----
def test_dense_inverse_form_gives_the_same_picks_as_the_chain_form():
    order, gains, _, _, tol = restated("er130", 60)
    a, b = kir_of("er130"), kir_of("er130", dense_inverse=True)
    assert a.info()["form"] == "chain" and b.info()["form"] == "dense"
    ra, rb = a.subset(60)[0], b.subset(60)[0]
    assert np.array_equal(ra, rb)
    assert rel_close(b.last_gains, gains, tol) and rel_close(a.last_gains, gains, tol)


def test_runs_repeat_bit_for_bit_on_one_handle_and_on_two():
    a, b = kir_of("general500", fold=16), kir_of("general500", fold=16)
    o1, g1, _ = a._dev.kirchhoff_select([50])
    o2, g2, _ = a._dev.kirchhoff_select([50])
    o3, g3, _ = b._dev.kirchhoff_select([50])
    assert np.array_equal(o1, o2) and np.array_equal(o1, o3)
    assert g1.tobytes() == g2.tobytes() == g3.tobytes()
    assert a.gains().tobytes() == b.gains().tobytes()
    assert a.kirchhoff_index(o1) == b.kirchhoff_index(o1)


def test_budget_prefixes_equal_single_runs():
    gk = kir_of("er130")
    results, sel_edges, times = gk.subsets([5, 20, 60])
    gains = gk.last_gains.copy()
    assert len(results) == 3 and len(sel_edges) == 60 and len(times) == 3 and all(np.diff(times) >= 0)
    for k, r in zip([5, 20, 60], results):
        res, sel = gk.subset(k)
        assert np.array_equal(res, r) and sel == sel_edges[:k]
        assert np.array_equal(gk.last_gains, gains[:k])
    for bad in (0, len(gk.all_candidate_edges) + 1):
        with pytest.raises(AssertionError):
            gk.subset(bad)
    with pytest.raises(AssertionError):
        gk.subsets([5, 3])


# ---- 6. refusals ----
def test_refusals_disconnected_fixed_graph_and_matrix_free_handle():
    n, fi, fj, fw, ci, cj, cw = chain_er(400, 0.01, 6)
    keep = fi != 199                                                   # two chains 0..199 and 200..399: beta = 1e-4
    with pytest.raises(_lib.MachipError, match="disconnected"):
        GreedyKirchhoff(edges(fi[keep], fj[keep], fw[keep]), edges(ci, cj, cw), n)
    dev = _lib.Esp(n, fi[keep], fj[keep], fw[keep], ci, cj, cw)
    for call in (lambda: dev.kirchhoff_select([3]), dev.kirchhoff_gains, lambda: dev.kirchhoff_eval([1, 2])):
        with pytest.raises(_lib.Disconnected, match="infinite"):
            call()
    free = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free=True)
    for call in (lambda: free.kirchhoff_select([3]), free.kirchhoff_gains, lambda: free.kirchhoff_eval([1, 2])):
        with pytest.raises(AssertionError, match="needs the dense inverse"):
            call()
    tree = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free="tree")
    with pytest.raises(AssertionError, match="needs the dense inverse"):
        tree.kirchhoff_select([3])
    ok = _lib.Esp(n, fi, fj, fw, ci, cj, cw)
    with pytest.raises(AssertionError, match="increasing"):
        ok.kirchhoff_select([5, 3])
    with pytest.raises(AssertionError, match="not enough"):
        ok.kirchhoff_select([len(cw) + 1])


# ---- 7. GreedyESP on the same handle type: unchanged before and after a Kirchhoff run ----
def test_greedy_esp_is_unchanged_by_a_kirchhoff_run_on_its_handle():
    n, fi, fj, fw, ci, cj, cw = graph("er130")
    ref_order, ref_gains, margins = KR.R.greedy(n, fi, fj, fw, ci, cj, cw, 60, fold=16)
    assert margins.min() > 1e-9
    esp = GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, fold=16)
    o0, g0, _ = esp._dev.select([60])
    r0 = esp.weighted_resistances()
    assert np.array_equal(o0, ref_order) and rel_close(g0, ref_gains, 1e-9)
    ko, _, _ = esp._dev.kirchhoff_select([37])                         # leaves pending columns and its own state behind
    esp._dev.kirchhoff_gains()
    esp._dev.kirchhoff_eval(ko[:9])
    o1, g1, _ = esp._dev.select([60])
    assert np.array_equal(o0, o1) and g0.tobytes() == g1.tobytes()
    assert esp.weighted_resistances().tobytes() == r0.tobytes()
    assert not np.array_equal(ko[:37], o0[:37])                        # (the two criteria do pick differently here)
