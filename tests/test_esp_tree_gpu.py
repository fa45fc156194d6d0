"""GreedyESP's matrix-free route for any connected fixed graph on the GPU (mac_amd/csrc/esp_tree.h, matrix_free="tree"): against the
dense general route where both run, beyond the dense limit against the NumPy restatement (tests/esp_tree_restatement.py: sparse
solves against the spanning tree, no lowest-common-ancestor logic), the log-det identity, the chain route's bits on a chain,
yesterday's selection as today's fixed edges, edge cases, determinism, refusals.

Tolerances.  Large cases: the restatement runs in float64 and in np.longdouble; their largest relative difference d on the gains is
the error of a float64 evaluation, the device gets max(100 d, 1e-12) (as tests/test_esp_free_gpu.py).  Against the dense general
route: 1e-9 relative on the gains and 1e-10 on the weighted resistances, the figures the existing tests use between the dense
general route and the chain-free one."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import load_golden
import esp_free_restatement as F
import esp_restatement as R
import esp_tree_restatement as T
from mac_amd import _lib
from mac_amd.solvers import GreedyESP
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu

LARGE_K = 300
LARGE = {"shallow": (T.shallow_case, 1), "deep": (T.deep_case, 1)}      # shape -> (generator, seed); margins asserted below


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def esp_of(n, fi, fj, fw, ci, cj, cw, **kw):
    return GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


def dev_of(n, fi, fj, fw, ci, cj, cw, **kw):
    return _lib.Esp(n, fi, fj, fw, ci, cj, cw, **kw)


def close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300) + 1e-15 * np.max(np.abs(b)))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


def random_general(n=500, seed=4):
    """The shape of tests/test_esp_free_gpu.py's random_general: a random spanning tree plus n / 2 extra fixed edges."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, 800), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, 820)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, 820)


@functools.lru_cache(maxsize=None)
def large(shape):
    """A case beyond the dense limit, its restatement in two precisions and their disagreement on the gains."""
    gen, seed = LARGE[shape]
    g = gen(seed)
    P = T.plan(*g[:4])
    o64, g64, m64 = T.greedy(*g, LARGE_K, P=P)
    old, gld, _ = T.greedy(*g, LARGE_K, dtype=np.longdouble, P=P)
    assert len(P["seeds"][2]) == 200
    assert m64.min() > 1e-6 and np.array_equal(o64, old)          # the sequence is pinned
    d = rel(g64, gld)
    depth = np.zeros(g[0], dtype=np.int64)
    for v in P["order"][1:]:
        depth[v] = depth[P["parent"][v]] + 1
    print(f"{shape}: tree depth {depth.max()}, smallest margin {m64.min():.3g}, float64 vs longdouble gains {d:.3g}")
    return g, o64, g64, d


@functools.lru_cache(maxsize=None)
def large_run(shape):
    g = large(shape)[0]
    esp = esp_of(*g, matrix_free="tree")
    order, gains, _ = esp._dev.select([LARGE_K])
    return esp, order.copy(), gains.copy(), esp.weighted_resistances().copy()


# ---- 1. a small general graph against the dense general route ----
def test_small_general_graph_agrees_with_the_dense_general_route():
    g = random_general()
    m = len(g[6])
    a = esp_of(*g)
    b = esp_of(*g, matrix_free="tree")
    H = _lib.host_esp_tree(*g[:4])
    inf = b.info()
    assert a.info()["form"] == "dense" and inf["form"] == "tree_free" and inf["beta"] == 0.0 and inf["fold"] == 0
    assert inf["seeds"] == len(H["seeds"][2]) > 100 and a.info()["seeds"] == 0
    assert close(b.weighted_resistances(), a.weighted_resistances(), 1e-10)          # before any pick
    oa, ga, _ = a._dev.select([m])
    ob, gb, _ = b._dev.select([m])
    assert np.array_equal(oa, ob)                                                   # every pick of K = m
    ok = ga > 0
    print(f"general n = 500: gains, tree route vs dense general route {rel(gb[ok], ga[ok]):.3g}")
    assert close(gb, ga, 1e-9)
    assert b.info()["pending"] == m
    a.subset(200); b.subset(200)
    assert close(b.weighted_resistances(), a.weighted_resistances(), 1e-10)          # after 200 picks


# ---- 2. beyond the dense limit ----
@pytest.mark.parametrize("shape", ["shallow", "deep"])
def test_beyond_the_dense_limit_matches_the_restatement(shape):
    g, o64, g64, d = large(shape)
    n, fi, fj, fw, ci, cj, cw = g
    esp, order, gains, _ = large_run(shape)
    inf = esp.info()
    assert inf["form"] == "tree_free" and inf["seeds"] == 200 and inf["ld"] >= n - 1 and inf["pending"] == LARGE_K
    assert np.array_equal(order, o64)                             # every pick
    tol = max(100.0 * d, 1e-12)
    err = rel(gains, g64)
    print(f"{shape}: gains, device vs restatement {err:.3g}, tolerance {tol:.3g} (100 x {d:.3g}, floor 1e-12)")
    assert len(gains) == LARGE_K and err <= tol
    res, sel = esp.subset(LARGE_K)
    ref = np.zeros(len(cw)); ref[o64] = 1.0
    assert np.array_equal(res, ref) and np.array_equal(esp.last_gains, gains)
    assert [(e.i, e.j, e.weight) for e in sel] == [(int(ci[e]), int(cj[e]), float(cw[e])) for e in o64]


# ---- 3. the log-det identity ----
@pytest.mark.parametrize("shape", ["shallow", "deep"])
def test_logdet_identity_beyond_the_limit(shape):
    g, o64, g64, _ = large(shape)
    n, fi, fj, fw, ci, cj, cw = g
    _, order, gains, _ = large_run(shape)
    assert np.array_equal(order, o64)
    L0 = R.reduced_laplacian(n, fi, fj, fw, sparse=True)          # all fixed edges, the seeds among them
    LK = R.reduced_laplacian(n, np.concatenate([fi, ci[o64]]), np.concatenate([fj, cj[o64]]), np.concatenate([fw, cw[o64]]), sparse=True)
    growth = R.logdet_sparse(LK) - R.logdet_sparse(L0)
    second = float(np.sum(np.log1p(g64)))                         # the other CPU route: the restatement's own sum
    d = abs(growth - second)
    tol = 10.0 * max(d, 1e-9 * abs(growth))
    dev = float(np.sum(np.log1p(gains)))
    print(f"{shape}: logdet growth sparse {growth!r}, device {dev!r}, |diff| {abs(dev - growth):.3g}; the two CPU routes disagree by {d:.3g};"
          f" tolerance {tol:.3g}")
    assert abs(dev - growth) <= tol


# ---- 4. a chain input: the chain route's bits ----
def test_chain_input_gives_the_chain_routes_bits():
    """The values entering the FMA chains are the same doubles by construction (R[lca] = R[min] on a chain, no seeds), the slices
    are the same function of (ld, j): equal order and equal gains, bit for bit."""
    g = arrays(load_golden("g2o_intel"))
    a = esp_of(*g, matrix_free=True)
    b = esp_of(*g, matrix_free="tree")
    assert b.info()["form"] == "tree_free" and b.info()["seeds"] == 0
    assert np.array_equal(a.weighted_resistances(), b.weighted_resistances())
    oa, ga, _ = a._dev.select([200])
    ob, gb, _ = b._dev.select([200])
    assert np.array_equal(oa, ob) and np.array_equal(ga, gb)
    assert np.array_equal(a.weighted_resistances(), b.weighted_resistances())


# ---- 5. yesterday's selection as today's fixed edges ----
def test_yesterdays_selection_as_todays_fixed_edges():
    """Picks 1..100 of a chain-route run become fixed edges; 100 picks of the tree route then reproduce picks 101..200 of the single
    K = 200 run.  The split stays at 100: the CPU restatement's margins over picks 101..200 are asserted to be above 1e-9."""
    SPLIT, K = 100, 200
    g = arrays(load_golden("g2o_intel"))
    n, fi, fj, fw, ci, cj, cw = g
    _, _, margins = F.greedy(n, fi, fj, fw, ci, cj, cw, K)
    print(f"intel: smallest margin over picks {SPLIT + 1}..{K} on the CPU: {margins[SPLIT:].min():.3g}")
    assert margins[SPLIT:].min() > 1e-9
    order, gains, _ = dev_of(*g, matrix_free=True).select([K])
    first = order[:SPLIT]
    rest = np.setdiff1d(np.arange(len(cw)), first)                # the remaining candidates, in their order
    today = dev_of(n, np.concatenate([fi, ci[first]]), np.concatenate([fj, cj[first]]), np.concatenate([fw, cw[first]]),
                   ci[rest], cj[rest], cw[rest], matrix_free="tree")
    inf = today.info()
    assert inf["form"] == "tree_free" and 0 < inf["seeds"] <= SPLIT
    o2, g2, _ = today.select([K - SPLIT])
    assert np.array_equal(rest[o2], order[SPLIT:])
    print(f"intel: {inf['seeds']} seeds; gains of picks {SPLIT + 1}..{K}, seeded tree route vs the single run {rel(g2, gains[SPLIT:]):.3g}")
    assert np.all(np.abs(g2 - gains[SPLIT:]) <= 1e-11 * np.abs(gains[SPLIT:]))


# ---- 6. edge cases ----
def test_edge_cases_on_a_12_node_graph():
    n = 12
    #     a spanning tree that is not index-consecutive, given with a duplicate (reversed) and a self-loop, plus two cycle-closing links
    fixed = [(0, 3, 1.2), (3, 1, 0.7), (3, 7, 1.9), (1, 3, 0.4),       # 1-3 twice, once reversed: one link of weight 1.1
             (7, 2, 0.9), (7, 7, 5.0),                                  # a fixed self-loop: dropped
             (0, 5, 1.4), (5, 4, 0.8), (4, 6, 1.1), (6, 8, 0.6), (8, 9, 1.3), (2, 10, 1.0), (10, 11, 0.5),
             (9, 11, 1.6), (1, 4, 0.75), (11, 9, 0.2)]                  # seeds: 9-11 (given twice, once reversed) and 1-4
    fi = np.array([f[0] for f in fixed]); fj = np.array([f[1] for f in fixed]); fw = np.array([f[2] for f in fixed])
    cand = [(2, 6, 1.3), (6, 2, 1.3), (2, 6, 1.3),         # exact duplicates (one reversed): ties, lowest index first
            (0, 9, 0.8), (11, 0, 1.1),                       # candidates at node 0
            (5, 5, 2.0),                                     # self-loop: score 0
            (3, 7, 0.7),                                     # parallel to a tree link
            (4, 1, 0.9),                                     # parallel to a seed
            (1, 10, 0.9), (4, 8, 1.7), (6, 11, 0.6)]
    ci = np.array([c[0] for c in cand]); cj = np.array([c[1] for c in cand]); cw = np.array([c[2] for c in cand])
    m = len(cand)
    H = _lib.host_esp_tree(n, fi, fj, fw)
    assert sorted(zip(*[x.tolist() for x in H["seeds"][:2]])) == [(1, 4), (9, 11)] and sorted(H["seeds"][2].tolist()) == [0.75, 1.6 + 0.2]
    order, gains, _ = R.greedy(n, fi, fj, fw, ci, cj, cw, m)
    esp = esp_of(n, fi, fj, fw, ci, cj, cw, matrix_free="tree")
    assert esp.info()["form"] == "tree_free" and esp.info()["seeds"] == 2
    r0 = esp.weighted_resistances()
    assert close(r0, R.scores(R.initial_sigma(n, fi, fj, fw)[0], ci, cj, cw), 1e-10) and r0[5] == 0.0
    res, sel = esp.subset(1)
    assert res.sum() == 1 and res[order[0]] == 1.0 and sel == [esp.all_candidate_edges[order[0]]]
    res, sel = esp.subset(m)
    assert res.sum() == m and len(sel) == m
    dev_order, dev_gains, _ = esp._dev.select([m])
    assert np.array_equal(dev_order, order)
    pos = dev_order.tolist()
    assert pos.index(0) < pos.index(1) < pos.index(2)    # exact ties go to the lowest index
    assert dev_order[-1] == 5 and dev_gains[-1] == 0.0   # the self-loop scores 0 throughout
    assert close(dev_gains, gains, 1e-9)
    assert close(esp.weighted_resistances(), R.scores(np.linalg.inv(R.reduced_laplacian(
        n, np.concatenate([fi, ci]), np.concatenate([fj, cj]), np.concatenate([fw, cw]))), ci, cj, cw), 1e-10)


# ---- 7. determinism ----
def test_two_runs_budget_prefixes_and_a_grown_history_are_bit_identical():
    g = large("shallow")[0]
    esp, order, gains, r = large_run("shallow")
    o2, g2, _ = esp._dev.select([LARGE_K])                       # the same handle again: restarts from the cached scores
    assert np.array_equal(o2, order) and np.array_equal(g2, gains) and np.array_equal(esp.weighted_resistances(), r)
    fresh = esp_of(*g, matrix_free="tree")
    r0 = fresh.weighted_resistances()                            # seeds the handle before any select
    results, sel, times = fresh.subsets_lazy([50, 150, 300])     # one run, three budgets
    assert len(times) == 3 and all(np.diff(times) >= 0)
    for k, res in zip([50, 150, 300], results):
        ref = np.zeros(len(g[6])); ref[order[:k]] = 1.0
        assert np.array_equal(res, ref)
    assert np.array_equal(fresh.last_gains, gains) and np.array_equal(fresh.weighted_resistances(), r)
    small = esp_of(*g, matrix_free="tree")                       # a larger K than the first call's: the history grows, the seeds stay
    o1, g1, _ = small._dev.select([100])
    assert np.array_equal(o1, order[:100]) and np.array_equal(g1, gains[:100]) and small.info()["pending"] == 100
    o3, g3, _ = small._dev.select([LARGE_K])
    assert np.array_equal(o3, order) and np.array_equal(g3, gains) and np.array_equal(small.weighted_resistances(), r)
    again = esp_of(*g, matrix_free="tree")
    assert np.array_equal(again.weighted_resistances(), r0)      # before any pick: the tree term and the seeds alone


# ---- 8. refusals ----
def test_refusals():
    n, fi, fj, fw, ci, cj, cw = random_general()
    keep = np.ones(len(fw), dtype=bool)
    keep[np.flatnonzero((fi == 7) | (fj == 7))] = False          # node 7 loses every fixed edge
    with pytest.raises(AssertionError, match="BAD_ARG.*connected fixed graph"):
        dev_of(n, fi[keep], fj[keep], fw[keep], ci, cj, cw, matrix_free="tree")
    with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_DENSE_INVERSE"):
        dev_of(n, fi, fj, fw, ci, cj, cw, matrix_free="tree", dense_inverse=True)
    lib = _lib.load()
    p_i32, p_f64, i32, f64 = _lib.p_i32, _lib.p_f64, _lib.i32, _lib.f64
    args = (n, len(fw), p_i32(i32(fi)), p_i32(i32(fj)), p_f64(f64(fw)), len(cw), p_i32(i32(ci)), p_i32(i32(cj)), p_f64(f64(cw)))

    def create(fold, flags):
        h = C.c_void_p()
        st = lib.machip_esp_create(0, *args, fold, flags, C.byref(h))
        msg = _lib.last_error()
        if st == _lib.OK:
            lib.machip_esp_destroy(h)
        return st, msg

    TREE = _lib.ESP_MATRIX_FREE | _lib.ESP_SPANNING_TREE
    st, msg = create(0, _lib.ESP_SPANNING_TREE)
    assert st == _lib.BAD_ARG and "only together with MACHIP_ESP_MATRIX_FREE" in msg
    st, msg = create(0, TREE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_DENSE_INVERSE" in msg
    st, msg = create(64, TREE)
    assert st == _lib.BAD_ARG and "fold" in msg
    st, msg = create(0, 4)                                        # the pins that do not move
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    with pytest.raises(AssertionError, match="BAD_ARG.*needs a chain"):
        esp_of(n, fi, fj, fw, ci, cj, cw, matrix_free=True)
    assert create(0, TREE)[0] == _lib.OK
    esp = esp_of(n, fi, fj, fw, ci, cj, cw, matrix_free="tree")
    x = np.full(len(cw), 0.5)
    for call in (lambda: esp._dev.relax_eval(x), lambda: esp._dev.relax_run(10, x), lambda: esp._dev.relax_inner(x, x)):
        with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_MATRIX_FREE"):
            call()
    for flags in (TREE, _lib.ESP_SPANNING_TREE):
        h = C.c_void_p()
        st = lib.machip_eig_create(0, *args, 0, 0, flags, C.byref(h))
        assert st == _lib.BAD_ARG and "not available" in _lib.last_error() and not h.value
    assert np.array_equal(esp.subset(5)[0], esp_of(n, fi, fj, fw, ci, cj, cw).subset(5)[0])       # the handle still works


def test_a_history_that_cannot_fit_is_refused_before_anything_is_allocated():
    n, m, r = 40000, 1200000, 50                # 8 ld (r + K) = 384 GB: more than the device has in all
    rng = np.random.default_rng(0)
    ti = np.arange(1, n)
    tj = np.array([rng.integers(0, i) for i in range(1, n)])
    fi = np.concatenate([ti, np.arange(r)]); fj = np.concatenate([tj, n - 1 - np.arange(r)])
    dev = _lib.Esp(n, fi, fj, np.ones(len(fi)), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m),
                   matrix_free="tree")
    inf = dev.info()
    ld, seeds = inf["ld"], inf["seeds"]
    assert 0 < seeds <= r
    with pytest.raises(AssertionError) as ei:
        dev.select([m])
    msg = str(ei.value)
    assert "BAD_ARG" in msg and "does not fit" in msg and f"n = {n}" in msg and f"K = {m}" in msg and f"{seeds} seeds" in msg
    assert str(8 * ld * (seeds + m)) in msg
    assert dev.info()["pending"] == 0           # no run happened
    order, gain, _ = dev.select([3])            # and a budget that fits runs
    assert len(set(order.tolist())) == 3 and np.all(np.diff(gain) <= 0)
    with pytest.raises(AssertionError, match="does not fit"):
        dev.select([m])                         # refused again with a seeded history in place ...
    o2, g2, _ = dev.select([3])                 # ... which is still there
    assert np.array_equal(o2, order) and np.array_equal(g2, gain)
