"""GreedyESP's matrix-free route on the GPU (mac_amd/csrc/esp_free.h): beyond the dense limit against the NumPy restatement of the
history recurrence (tests/esp_free_restatement.py), against the dense routes where both run, the log-det identity, sparse solves.

Tolerances.  The gains of the large case: the test runs the restatement in float64 and in np.longdouble; their largest relative
difference d is the error of a float64 evaluation of the recurrence, and the device -- which sums a row's products over column
slices, another order -- gets 100 d, floor 1e-12.  Against the dense chain route (where both run) the sums differ by their order
only: 1e-11 relative on the gains (the route does not keep one chain per row once the history is sliced; with one slice,
option esp_free_split = 1, the per-entry arithmetic is the dense chain form's with fold > K and the test asks for equal bits)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from conftest import load_golden
import esp_free_restatement as F
import esp_restatement as R
from mac_amd import _lib
from mac_amd.solvers import GreedyESP
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu

LARGE_SEED, LARGE_K = 2, 300


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def esp_of(n, fi, fj, fw, ci, cj, cw, **kw):
    return GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


def close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300) + 1e-15 * np.max(np.abs(b)))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


@functools.lru_cache(maxsize=None)
def large():
    """The case beyond the limit, its restatement in two precisions and their disagreement on the gains."""
    g = F.large_case(LARGE_SEED)
    o64, g64, m64 = F.greedy(*g, LARGE_K)
    old, gld, _ = F.greedy(*g, LARGE_K, dtype=np.longdouble)
    assert m64.min() > 1e-6 and np.array_equal(o64, old)
    d = rel(g64, gld)
    print(f"large case: smallest margin {m64.min():.3g}, float64 vs longdouble gains {d:.3g}")
    return g, o64, g64, d


@functools.lru_cache(maxsize=None)
def large_run():
    """One device run of the large case (kept for the tests that only read it)."""
    g, _, _, _ = large()
    esp = esp_of(*g, matrix_free=True)
    order, gains, _ = esp._dev.select([LARGE_K])
    return esp, order.copy(), gains.copy(), esp.weighted_resistances().copy()


def grown(g, sel):
    n, fi, fj, fw, ci, cj, cw = g
    return R.reduced_laplacian(n, np.concatenate([fi, ci[sel]]), np.concatenate([fj, cj[sel]]), np.concatenate([fw, cw[sel]]),
                               sparse=True)


# ---- 1. beyond the limit ----
def test_beyond_the_dense_limit_matches_the_restatement():
    g, o64, g64, d = large()
    n, fi, fj, fw, ci, cj, cw = g
    esp = esp_of(*g, matrix_free=True)
    inf = esp.info()
    assert inf["form"] == "chain_free" and inf["beta"] == 0.0 and inf["ld"] >= n - 1 and inf["fold"] == 0
    res, sel = esp.subset(LARGE_K)
    ref = np.zeros(len(cw)); ref[o64] = 1.0
    assert np.array_equal(res, ref)
    assert [(e.i, e.j, e.weight) for e in sel] == [(int(ci[e]), int(cj[e]), float(cw[e])) for e in o64]
    tol = max(100.0 * d, 1e-12)
    err = rel(esp.last_gains, g64)
    print(f"gains: device vs restatement {err:.3g}, tolerance {tol:.3g} (100 x {d:.3g}, floor 1e-12)")
    assert len(esp.last_gains) == LARGE_K and err <= tol          # every pick is compared
    order, gains, _ = esp._dev.select([LARGE_K])
    assert np.array_equal(order, o64) and np.array_equal(gains, esp.last_gains)
    assert esp.info()["pending"] == LARGE_K


# ---- 2. agreement with the dense routes where both run ----
@pytest.mark.parametrize("case", ["intel", "sphere2500"])
def test_agrees_with_the_dense_chain_route(case):
    g = arrays(load_golden("g2o_" + case))
    K = len(g[6]) if case == "intel" else 600
    a = esp_of(*g)
    b = esp_of(*g, matrix_free=True)
    assert a.info()["form"] == "chain" and b.info()["form"] == "chain_free"
    if case == "intel":
        assert close(b.weighted_resistances(), a.weighted_resistances(), 1e-10)        # before any pick
    oa, ga, _ = a._dev.select([K])
    ob, gb, _ = b._dev.select([K])
    assert np.array_equal(oa, ob)
    print(f"{case}: gains, matrix-free vs dense chain route {rel(gb, ga):.3g}")
    assert np.all(np.abs(gb - ga) <= 1e-11 * np.abs(ga))       # (sliced sums: not one FMA chain per row, so not array_equal)
    if case == "intel":
        a.subset(200); b.subset(200)
        assert close(b.weighted_resistances(), a.weighted_resistances(), 1e-10)


# ---- 3. the log-det identity at n = 40 000 ----
def test_logdet_identity_beyond_the_limit():
    g, o64, g64, _ = large()
    n, fi, fj, fw, ci, cj, cw = g
    _, order, gains, _ = large_run()
    assert np.array_equal(order, o64)
    ld0, ldK = R.logdet_sparse(grown(g, o64[:0])), R.logdet_sparse(grown(g, o64))
    # second route: the tridiagonal M_0 by its pivot recurrence, plus the restatement's own sum of log1p
    diag = fw + np.concatenate([fw[1:], [0.0]])
    p, tri = 0.0, 0.0
    for i in range(n - 1):
        p = diag[i] - (fw[i] ** 2 / p if i else 0.0)
        tri += np.log(p)
    second = tri + float(np.sum(np.log1p(g64)))
    growth = ldK - ld0
    d = abs(ldK - second)
    tol = 10.0 * max(d, 1e-9 * abs(growth))
    dev = float(np.sum(np.log1p(gains)))
    print(f"logdet growth: sparse {growth!r}, device {dev!r}, |diff| {abs(dev - growth):.3g}; the two CPU routes disagree by {d:.3g}"
          f" (M_0: {abs(ld0 - tri):.3g}); tolerance {tol:.3g}")
    assert abs(dev - growth) <= tol


# ---- 4. weighted resistances after the 300 picks, against sparse solves (the loose cross-check) ----
def test_weighted_resistances_after_the_run_match_sparse_solves():
    g, o64, _, _ = large()
    n, fi, fj, fw, ci, cj, cw = g
    _, order, _, r = large_run()
    assert np.array_equal(order, o64)
    idx = np.random.default_rng(0).choice(len(cw), 200, replace=False)
    A = np.zeros((n, len(idx)))
    A[ci[idx], np.arange(len(idx))] += 1.0
    A[cj[idx], np.arange(len(idx))] -= 1.0
    A = A[1:]
    X = splu(grown(g, o64)).solve(A)
    ref = cw[idx] * np.einsum("ij,ij->j", A, X)
    print(f"resistances after {LARGE_K} picks vs sparse solves: {np.max(np.abs(r[idx] - ref) / np.maximum(np.abs(ref), 1e-300)):.3g}")
    assert close(r[idx], ref, 1e-5)
    assert np.all(r[o64] < 1.0)                        # a selected edge is in the graph now: its w r is a leverage score


# ---- 5. repeatability and options ----
def test_repeatability_prefixes_growth_and_split_option():
    g, o64, g64, _ = large()
    esp, order, gains, r = large_run()
    o2, g2, _ = esp._dev.select([LARGE_K])                       # the same handle again
    assert np.array_equal(o2, order) and np.array_equal(g2, gains) and np.array_equal(esp.weighted_resistances(), r)
    fresh = esp_of(*g, matrix_free=True)
    results, sel, times = fresh.subsets_lazy([50, 150, 300])     # one run, three budgets
    assert len(times) == 3 and all(np.diff(times) >= 0)
    for k, res in zip([50, 150, 300], results):
        ref = np.zeros(len(g[6])); ref[order[:k]] = 1.0
        assert np.array_equal(res, ref)
    assert np.array_equal(fresh.last_gains, gains) and np.array_equal(fresh.weighted_resistances(), r)
    small = esp_of(*g, matrix_free=True)                         # a larger K than the first call's: the history grows
    o1, g1, _ = small._dev.select([100])
    assert np.array_equal(o1, order[:100]) and np.array_equal(g1, gains[:100]) and small.info()["pending"] == 100
    o3, g3, _ = small._dev.select([LARGE_K])
    assert np.array_equal(o3, order) and np.array_equal(g3, gains) and np.array_equal(small.weighted_resistances(), r)
    for split in (1, 3):                                         # slices of the history: another summation order, the same picks
        with _lib.default_options(esp_free_split=split):
            e = esp_of(*g, matrix_free=True)
        os_, gs, _ = e._dev.select([LARGE_K])
        print(f"esp_free_split={split}: gains vs automatic {rel(gs, gains):.3g}")
        assert np.array_equal(os_, order) and np.all(np.abs(gs - gains) <= 1e-12 * np.abs(gains))


def test_one_slice_is_bit_identical_to_the_dense_chain_route_without_folds():
    """esp_free_split = 1 keeps one FMA chain per row, columns ascending: the arithmetic of k_esp_z with every update pending."""
    g = arrays(load_golden("g2o_intel"))
    a = esp_of(*g, fold=256)
    with _lib.default_options(esp_free_split=1):
        b = esp_of(*g, matrix_free=True)
    oa, ga, _ = a._dev.select([200])
    ob, gb, _ = b._dev.select([200])
    assert np.array_equal(oa, ob) and np.array_equal(ga, gb)


# ---- 6. edge cases ----
def test_edge_cases_duplicates_node0_selfloop_parallel_matrix_free():
    rng = np.random.default_rng(9)
    n = 12
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    cand = [(2, 7, 1.3), (7, 2, 1.3), (2, 7, 1.3),         # duplicates (one reversed): exact ties, lowest index first
            (0, 9, 0.8), (11, 0, 1.1),                       # touching node 0
            (5, 5, 2.0),                                     # self-loop: score 0
            (3, 4, 0.7),                                     # parallel to a fixed link
            (1, 10, 0.9), (4, 8, 1.7), (6, 11, 0.6)]
    ci = np.array([c[0] for c in cand]); cj = np.array([c[1] for c in cand]); cw = np.array([c[2] for c in cand])
    m = len(cand)
    order, gains, _ = R.greedy(n, fi, fj, fw, ci, cj, cw, m)
    esp = esp_of(n, fi, fj, fw, ci, cj, cw, matrix_free=True)
    assert esp.info()["form"] == "chain_free"
    r0 = esp.weighted_resistances()
    assert close(r0, R.scores(R.initial_sigma(n, fi, fj, fw)[0], ci, cj, cw), 1e-10) and r0[5] == 0.0
    res, sel = esp.subset(1)
    assert res.sum() == 1 and res[order[0]] == 1.0 and sel == [esp.all_candidate_edges[order[0]]]
    res, sel = esp.subset(m)
    assert res.sum() == m and len(sel) == m
    dev_order, dev_gains, _ = esp._dev.select([m])       # (duplicates are equal Edge tuples: indices from the handle)
    assert np.array_equal(dev_order, order)
    assert [tuple(e) for e in sel] == [cand[e] for e in order]
    pos = dev_order.tolist()
    assert pos.index(0) < pos.index(1) < pos.index(2)    # exact ties go to the lowest index
    assert dev_order[-1] == 5 and dev_gains[-1] == 0.0   # the self-loop scores 0 throughout
    assert close(dev_gains, gains, 1e-9)


# ---- 7. error paths ----
def random_general(n=500, seed=4):
    """Connected, not a chain: a random spanning tree plus extra fixed edges; random candidates (some touching node 0)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, 800), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, 820)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, 820)


def test_error_paths():
    with pytest.raises(AssertionError, match="BAD_ARG.*needs a chain"):
        esp_of(*random_general(), matrix_free=True)
    g = arrays(load_golden("g2o_intel"))
    with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_DENSE_INVERSE"):
        esp_of(*g, matrix_free=True, dense_inverse=True)
    esp = esp_of(*g, matrix_free=True)
    m = len(g[6])
    x = np.full(m, 0.5)
    for call in (lambda: esp._dev.relax_eval(x), lambda: esp._dev.relax_run(10, x), lambda: esp._dev.relax_inner(x, x)):
        with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_MATRIX_FREE"):
            call()
    n, fi, fj, fw, ci, cj, cw = g
    lib = _lib.load()
    h = C.c_void_p()
    st = lib.machip_eig_create(0, n, len(fw), _lib.p_i32(_lib.i32(fi)), _lib.p_i32(_lib.i32(fj)), _lib.p_f64(_lib.f64(fw)), m,
                               _lib.p_i32(_lib.i32(ci)), _lib.p_i32(_lib.i32(cj)), _lib.p_f64(_lib.f64(cw)), 0, 0,
                               _lib.ESP_MATRIX_FREE, C.byref(h))
    assert st == _lib.BAD_ARG and "MACHIP_ESP_MATRIX_FREE" in _lib.last_error() and not h.value
    assert np.array_equal(esp.subset(5)[0], esp_of(*g).subset(5)[0])       # the handle still works after the refusals


def test_a_history_that_cannot_fit_is_refused_before_anything_is_allocated():
    n, m = 40000, 1200000                      # 8 ld K = 384 GB: more than the device has in all
    rng = np.random.default_rng(0)
    fi = np.arange(n - 1)
    dev = _lib.Esp(n, fi, fi + 1, np.ones(n - 1), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m),
                   matrix_free=True)
    ld = dev.info()["ld"]
    with pytest.raises(AssertionError) as ei:
        dev.select([m])
    msg = str(ei.value)
    assert "BAD_ARG" in msg and "does not fit" in msg and f"n = {n}" in msg and f"K = {m}" in msg and str(8 * ld * m) in msg
    assert dev.info()["pending"] == 0           # no run happened, no history was made
    order, gain, _ = dev.select([3])            # and a budget that fits runs
    assert len(set(order.tolist())) == 3 and np.all(np.diff(gain) <= 0)
