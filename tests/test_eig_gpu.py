"""GreedyEig on the GPU (mac_amd/csrc/eig.h) against an independent NumPy restatement of the rule (tests/eig_restatement.py).

Tolerances.  The device's stop rule is ||L_e v - lambda v||_1 / ||L_e||_inf < 1e-8 with ||v||_2 = 1; ||r||_2 <= ||r||_1, so a
reported value is within TOL(e) = 1e-8 ||L_e||_inf of an eigenvalue of L_e.  The reference's scan has a tie tolerance of 1e-8, so a
device pick may fall short of the CPU maximum by 1e-8 + 2 TOL (the solver's error on both sides).  The order is pinned only on an
input where the restatement's smallest best-vs-second gap is at least 100 times that."""
import networkx as nx
import numpy as np
import pytest

from conftest import load_golden
import eig_restatement as R
from mac_amd import _lib
from mac_amd.solvers import MAC, GreedyEig
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def eig_of(n, fi, fj, fw, ci, cj, cw, **kw):
    return GreedyEig(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


def chain_er(n, p, seed):
    """Chain-fixed random graph: links (i, i+1) and ER candidates off the chain, weights uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < p
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def petersen():
    G = nx.petersen_graph()
    T = nx.minimum_spanning_tree(G)
    rng = np.random.default_rng(2)
    f = [(a, b, float(rng.uniform(0.5, 2.0))) for a, b in T.edges]
    c = [(a, b, float(rng.uniform(0.5, 2.0))) for a, b in nx.difference(G, T).edges]
    return (10, np.array([e[0] for e in f]), np.array([e[1] for e in f]), np.array([e[2] for e in f]),
            np.array([e[0] for e in c]), np.array([e[1] for e in c]), np.array([e[2] for e in c]))


def random_general(n=200, mc=300, seed=4):
    """Connected, not a chain: a random spanning tree plus extra fixed edges; random candidates (some touching node 0)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, mc), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, mc + 20)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, mc + 20)


def case(name):
    if name == "petersen":
        return petersen()
    if name == "general200":
        return random_general()
    if name == "chain300":
        return chain_er(300, 0.03, 0)
    return arrays(load_golden("g2o_intel"))


CASES = ["petersen", "general200", "chain300", "intel"]


# ---- 1. values and bounds of every candidate after create ----
@pytest.mark.parametrize("name", CASES)
def test_candidate_values_and_bounds_after_create_match_restatement(name):
    g = case(name)
    n, fi, fj, fw, ci, cj, cw = g
    L = R.laplacian(n, fi, fj, fw)
    ref = R.values_brute(L, ci, cj, cw) if name == "petersen" else R.values_secular(L, ci, cj, cw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(*g)
    inf = ge.info()
    assert inf["form"] == ("chain" if name in ("chain300", "intel") else "dense") and inf["beta"] == 0.0
    assert abs(inf["lambda2"] - R.fiedler(L)[0]) <= 1e-8 * R.norm_inf(L)
    lam = ge.candidate_lambda2()
    print(name, "max |lambda2 - ref| / tol:", float(np.max(np.abs(lam - ref) / tol)))
    assert np.all(np.abs(lam - ref) <= tol)
    u, uref = ge.candidate_bounds(), R.bounds(L, ci, cj, cw)
    print(name, "max rel bound error:", float(np.max(np.abs(u - uref) / np.abs(uref))))
    assert np.all(np.abs(u - uref) <= 1e-10 * np.abs(uref))
    assert np.all(u >= lam - tol)


# ---- 2. replay validity: every pick is (within the tolerances) a maximiser, and the reported lambda_2 is right ----
@pytest.mark.parametrize("name", CASES)
def test_every_pick_is_a_maximiser_on_replay(name):
    g = case(name)
    m = len(g[6])
    K = {"petersen": m, "general200": 30, "chain300": 30, "intel": 10}[name]
    ge = eig_of(*g)
    sol, sel = ge.subset(K)
    order = [int(np.nonzero((g[4] == e.i) & (g[5] == e.j) & (g[6] == e.weight))[0][0]) for e in sel]
    assert len(set(order)) == K and np.array_equal(np.nonzero(sol)[0], np.sort(order))
    r = R.greedy(*g, K, method="brute" if name == "petersen" else "secular", order=order)
    for k in range(K):
        tolL = 1e-8 * r["norms"][k].max()
        best = np.nanmax(r["values"][k])
        print(name, k, "shortfall", float(best - r["lam2"][k]), "lambda2 err / tol", float(abs(ge.last_lambda2[k] - r["lam2"][k]) / tolL))
        assert r["lam2"][k] >= best - 1e-8 - 2 * tolL
        assert abs(ge.last_lambda2[k] - r["lam2"][k]) <= tolL


# ---- 3. order pinned where the gaps allow it ----
def test_order_equals_restatement_where_the_gaps_are_wide():
    g = chain_er(40, 0.1, 1)
    K = 5
    r = R.greedy(*g, K, method="brute")
    tol = 1e-8 + 2e-8 * max(x.max() for x in r["norms"])
    assert r["gaps"].min() >= 100 * tol, (r["gaps"], tol)          # the precondition: a seed that loses it fails here
    ge = eig_of(*g)
    sol, sel = ge.subset(K)
    assert [(e.i, e.j) for e in sel] == [(int(g[4][e]), int(g[5][e])) for e in r["order"]]
    assert np.allclose(ge.last_lambda2, r["lam2"], rtol=0, atol=tol)


# ---- 4. pruning is sound and is used ----
def test_pruning_skips_candidates_and_only_ones_that_cannot_win():
    g = chain_er(300, 0.03, 0)
    m = len(g[6])
    K = 12
    ge = eig_of(*g, batch=64)
    sol, sel = ge.subset(K)
    inf = ge.info()
    solved = inf["solved"]
    unselected = m - np.arange(K)
    assert len(solved) == K and np.all(solved <= unselected) and np.all(inf["applications"] >= solved)
    print("solved per pick", solved.tolist(), "of", unselected.tolist(), "applications", inf["applications"].tolist())
    assert np.any(solved < unselected)
    order = [int(np.nonzero((g[4] == e.i) & (g[5] == e.j))[0][0]) for e in sel]
    r = R.greedy(*g, K, order=order)
    for k in range(K):
        # the device solves the candidates in decreasing order of the bound: the unsolved ones are the m_k - solved[k] smallest bounds
        u = r["bounds"][k]
        idx = np.argsort(-np.where(np.isnan(u), -np.inf, u), kind="stable")[:unselected[k]]
        unsolved = idx[solved[k]:]
        if len(unsolved):
            assert np.max(r["values"][k][unsolved]) < r["lam2"][k]


# ---- 5. pending block / fold and batch size do not change the result ----
@pytest.mark.parametrize("kw", [dict(fold=3), dict(fold=64), dict(batch=16)])
def test_fold_and_batch_do_not_change_the_picks(kw):
    g = chain_er(300, 0.03, 0)
    K = 10
    a = eig_of(*g)
    b = eig_of(*g, **kw)
    sa, ea = a.subset(K)
    sb, eb = b.subset(K)
    L = R.laplacian(g[0], np.concatenate([g[1], g[4]]), np.concatenate([g[2], g[5]]), np.concatenate([g[3], g[6]]))
    tol = 1e-8 * R.norm_inf(L)
    assert b.info()[next(iter(kw))] == next(iter(kw.values()))
    assert [(e.i, e.j) for e in ea] == [(e.i, e.j) for e in eb]
    assert np.all(np.abs(a.last_lambda2 - b.last_lambda2) <= 2 * tol)


# ---- 6. chain form vs the dense inverse ----
def test_chain_form_and_dense_inverse_agree_on_a_long_chain():
    g = chain_er(1024, 0.001, 5)
    a = eig_of(*g)
    b = eig_of(*g, dense_inverse=True)
    assert a.info()["form"] == "chain" and b.info()["form"] == "dense"
    a.subset(5); b.subset(5)
    L = R.laplacian(g[0], np.concatenate([g[1], g[4]]), np.concatenate([g[2], g[5]]), np.concatenate([g[3], g[6]]))
    tol = 1e-8 * R.norm_inf(L)
    print("chain vs dense lambda2", a.last_lambda2, b.last_lambda2)
    assert np.all(np.abs(a.last_lambda2 - b.last_lambda2) <= 2 * tol)


# ---- 7. end to end, as the reference's example uses the class ----
def test_end_to_end_on_intel_matches_mac_objective():
    g = arrays(load_golden("g2o_intel"))
    n, fi, fj, fw, ci, cj, cw = g
    K = 10
    ge = eig_of(*g)
    sol, sel = ge.subset(K)
    assert sol.shape == (len(cw),) and set(np.unique(sol)) == {0.0, 1.0} and sol.sum() == K
    cand = edges(ci, cj, cw)
    assert sorted((e.i, e.j, e.weight) for e in sel) == sorted((cand[i].i, cand[i].j, cand[i].weight) for i in np.nonzero(sol)[0])
    obj = MAC(edges(fi, fj, fw), cand, n).evaluate_objective(sol)
    L = R.laplacian(n, np.concatenate([fi, ci[sol == 1]]), np.concatenate([fj, cj[sol == 1]]), np.concatenate([fw, cw[sol == 1]]))
    assert abs(obj - ge.last_lambda2[-1]) <= 1e-8 * R.norm_inf(L)
    assert np.all(np.diff(ge.last_lambda2) >= -1e-8 * R.norm_inf(L))
    sol2, sel2 = ge.subset(K)                       # a second run on the same handle, and a fresh handle
    sol3, sel3 = eig_of(*g).subset(K)
    assert sel == sel2 == sel3 and np.array_equal(sol, sol2) and np.array_equal(sol, sol3)


def test_edge_cases_k_zero_k_too_large_disconnected():
    g = petersen()
    ge = eig_of(*g)
    sol, sel = ge.subset(0)
    assert sel == [] and np.array_equal(sol, np.zeros(len(g[6])))
    with pytest.raises(AssertionError):
        ge.subset(len(g[6]) + 1)
    n, fi, fj, fw, ci, cj, cw = chain_er(40, 0.1, 1)
    keep = fi != 19                                  # two chains: every node has a fixed edge, the graph is not connected
    with pytest.raises(_lib.Disconnected):
        eig_of(n, fi[keep], fj[keep], fw[keep], ci, cj, cw)


def edge_case_graph(tree):
    """12 nodes, a fixed tree (the chain, or one that branches at node 0 and below) and candidates that are duplicates (one
    reversed), a self-loop, parallel to a fixed link, at node 0, with weights from 1e-3 to 1e3."""
    rng = np.random.default_rng(9)
    n = 12
    fi = np.arange(1, n)
    fj = fi - 1 if tree == "chain" else np.array([0, 0, 1, 1, 2, 3, 3, 5, 6, 6, 8])
    fw = rng.uniform(0.5, 2.0, n - 1)
    cand = [(2, 7, 1.3), (7, 2, 1.3), (2, 7, 1.3),           # exact duplicates, one reversed
            (5, 5, 2.0),                                      # self-loop: lambda_2(L_cur), and its bound is that
            (int(fi[4]), int(fj[4]), 0.7),                    # parallel to a fixed link
            (0, 9, 0.8), (11, 0, 1.1), (0, 4, 1e3),           # at node 0
            (1, 10, 1e-3), (4, 8, 1e3), (6, 11, 0.03), (3, 9, 30.0)]
    return n, fi, fj, fw, np.array([c[0] for c in cand]), np.array([c[1] for c in cand]), np.array([c[2] for c in cand])


@pytest.mark.parametrize("tree", ["chain", "branching"])
def test_edge_cases_duplicates_node0_selfloop_parallel(tree):
    g = edge_case_graph(tree)
    n, fi, fj, fw, ci, cj, cw = g
    m, loop = len(cw), 3
    L = R.laplacian(n, fi, fj, fw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(*g)
    assert ge.info()["form"] == ("chain" if tree == "chain" else "dense")
    lam, u = ge.candidate_lambda2(), ge.candidate_bounds()
    ref, uref = R.values_brute(L, ci, cj, cw), R.bounds(L, ci, cj, cw)
    print(tree, "max |lambda2 - ref| / tol:", float(np.max(np.abs(lam - ref) / tol)), "max rel bound error:", float(np.max(np.abs(u - uref) / np.abs(uref))))
    assert np.all(np.abs(lam - ref) <= tol)
    assert np.all(np.abs(u - uref) <= 1e-10 * np.abs(uref)) and np.all(u >= lam - tol)
    assert u[loop] == ge.info()["lambda2"] and abs(lam[loop] - R.fiedler(L)[0]) <= tol[loop]
    # a replay of all m picks (duplicates are equal Edge tuples: indices from the handle)
    sol, sel = ge.subset(m)
    order, lam2, _ = ge._dev.select(m)
    assert sol.sum() == m and sorted(order.tolist()) == list(range(m)) and np.array_equal(lam2, ge.last_lambda2)
    assert [(e.i, e.j, e.weight) for e in sel] == [(int(ci[e]), int(cj[e]), float(cw[e])) for e in order]
    r = R.greedy(*g, m, method="brute", order=order)
    for k in range(m):
        tolL = 1e-8 * r["norms"][k].max()
        vals = r["values"][k]
        assert r["lam2"][k] >= np.nanmax(vals) - 1e-8 - 2 * tolL
        assert abs(lam2[k] - r["lam2"][k]) <= tolL
        if order[k] == loop:      # only when no other candidate raises lambda_2 by more than the tie tolerance (and the solver's error)
            others = np.delete(vals, loop)
            print(tree, "self-loop picked at", k, "of", m)
            assert np.all(np.isnan(others)) or np.nanmax(others) - r["lam_before"][k] <= 1e-8 + 2 * tolL


@pytest.mark.parametrize("n", [2, 3])
def test_two_and_three_node_graphs(n):
    """n' = 1 and 2: one 64-tile of Sigma that is nearly all padding; for n = 2 the start vector is the Fiedler vector already (a
    zero residual at the start)."""
    fi, fj, fw = np.arange(1, n), np.arange(n - 1), np.array([1.5, 0.75])[:n - 1]
    cand = [(0, n - 1, 2.0), (n - 1, 0, 0.5), (1, 1, 3.0)] + ([(1, 2, 1e-3)] if n == 3 else [])
    g = (n, fi, fj, fw, np.array([c[0] for c in cand]), np.array([c[1] for c in cand]), np.array([c[2] for c in cand]))
    ci, cj, cw = g[4:]
    m = len(cw)
    L = R.laplacian(n, fi, fj, fw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(*g)
    inf = ge.info()
    assert inf["ld"] == 64 and abs(inf["lambda2"] - R.fiedler(L)[0]) <= 1e-8 * R.norm_inf(L)
    lam, u = ge.candidate_lambda2(), ge.candidate_bounds()
    assert np.all(np.abs(lam - R.values_brute(L, ci, cj, cw)) <= tol)
    uref = R.bounds(L, ci, cj, cw)
    assert np.all(np.abs(u - uref) <= 1e-10 * np.abs(uref)) and np.all(u >= lam - tol)
    order, lam2, _ = ge._dev.select(m)
    assert sorted(order.tolist()) == list(range(m))
    r = R.greedy(*g, m, method="brute", order=order)
    for k in range(m):
        tolL = 1e-8 * r["norms"][k].max()
        assert r["lam2"][k] >= np.nanmax(r["values"][k]) - 1e-8 - 2 * tolL and abs(lam2[k] - r["lam2"][k]) <= tolL


def test_reference_example_lines_run(tmp_path):
    """The solver section of the reference's Petersen example, through the compat package, in a fresh interpreter."""
    import os, subprocess, sys
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import networkx as nx, numpy as np\n"
            "from mac.solvers import MAC, NaiveGreedy\nfrom mac.solvers.greedy_eig import GreedyEig\n"
            "from mac.utils.conversions import nx_to_mac\nfrom mac.utils.graphs import select_edges\n"
            "G = nx.petersen_graph(); n = len(G.nodes())\n"
            "spanning_tree = nx.minimum_spanning_tree(G); loop_graph = nx.difference(G, spanning_tree)\n"
            "fixed = nx_to_mac(spanning_tree); cand = nx_to_mac(loop_graph)\n"
            "k = int(0.4 * len(cand))\n"
            "ge = GreedyEig(fixed, cand, n)\nresult, edges = ge.subset(k)\n"
            "mac = MAC(fixed, cand, n)\n"
            "assert len(edges) == k and result.sum() == k\n"
            "assert abs(mac.evaluate_objective(result) - ge.last_lambda2[-1]) < 1e-6\nprint('ok', ge.last_lambda2)"
            % (ROOT, os.path.join(ROOT, "compat")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
