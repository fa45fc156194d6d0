"""GreedyESP on the GPU (mac_amd/csrc/esp.h) against an independent NumPy restatement of the rule (tests/esp_restatement.py),
the log-det identity  sum_k log(1 + gain_k) = logdet(L_K,red + beta I) - logdet(L_0,red + beta I)  and sparse solves."""
import networkx as nx
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from conftest import load_golden
import esp_restatement as R
from mac_amd import _lib
from mac_amd.solvers import MAC, GreedyESP
from mac_amd.utils.graphs import Edge, weight_graph_lap_from_edge_list

pytestmark = pytest.mark.gpu


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def esp_of(n, fi, fj, fw, ci, cj, cw, **kw):
    return GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, **kw)


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


def random_general(n=500, seed=4):
    """Connected, not a chain: a random spanning tree plus extra fixed edges; random candidates (some touching node 0)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, 800), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, 820)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, 820)


def dense_scores(n, fi, fj, fw, ci, cj, cw):
    Sig, _ = R.initial_sigma(n, fi, fj, fw)
    return R.scores(Sig, ci, cj, cw)


def close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300) + 1e-15 * np.max(np.abs(b)))


# ---- 1. resistances after create ----
@pytest.mark.parametrize("case", ["petersen", "general500", "disconnected", "intel"])
def test_resistances_after_create_match_dense_inverse(case):
    if case == "petersen":
        g = petersen()
    elif case == "general500":
        g = random_general()
    elif case == "disconnected":       # two chains 0..199 and 200..399: no node without a fixed edge -> beta = 1e-4
        n, fi, fj, fw, ci, cj, cw = chain_er(400, 0.01, 6)
        keep = fi != 199
        g = (n, fi[keep], fj[keep], fw[keep], ci, cj, cw)
    else:
        g = arrays(load_golden("g2o_intel"))
    esp = esp_of(*g)
    inf = esp.info()
    assert inf["form"] == ("chain" if case == "intel" else "dense")
    assert inf["beta"] == (1e-4 if case == "disconnected" else 0.0)
    assert close(esp.weighted_resistances(), dense_scores(*g), 1e-10)


def test_chain_forms_agree_with_each_other_and_the_dense_inverse():
    """n = 4 096 chain: the closed form is exact; the dense Gauss-Jordan inverse of this ill-conditioned (~n^2) matrix carries
    ~1e-10 relative error in the resistances, about twice LAPACK's (measured: 1.1e-10 vs 4e-11)."""
    g = chain_er(4096, 0.0004, 8)
    n, fi, fj, fw, ci, cj, cw = g
    link = np.concatenate([[0.0], np.cumsum(1.0 / fw)])
    exact = cw * np.abs(link[ci] - link[cj])
    ref = dense_scores(*g)
    a = esp_of(*g)
    b = esp_of(*g, dense_inverse=True)
    assert a.info()["form"] == "chain" and b.info()["form"] == "dense"
    ra, rb = a.weighted_resistances(), b.weighted_resistances()
    assert close(ra, exact, 1e-11) and close(ra, ref, 1e-10)
    assert close(rb, exact, 1e-9) and close(ra, rb, 1e-9)
    k = 200
    _, _, margins = R.greedy(*g, k)
    assert margins.min() > 1e-8
    assert np.array_equal(a.subset(k)[0], b.subset(k)[0])


# ---- 2. selection parity with the restatement ----
def test_intel_full_sweep_matches_restatement():
    g = arrays(load_golden("g2o_intel"))
    m = len(g[6])
    ks = [int(p * m) for p in np.linspace(0.1, 1.0, 10)]
    order, gains, margins = R.greedy(*g, m)
    assert margins.min() > 1e-9
    esp = esp_of(*g, lazy=True)
    results, sel_edges, times = esp.subsets_lazy(ks)
    assert len(results) == 10 and len(times) == 10 and all(np.diff(times) >= 0)
    for k, r in zip(ks, results):
        ref = np.zeros(m); ref[order[:k]] = 1.0
        assert np.array_equal(r, ref)
    assert [(e.i, e.j, e.weight) for e in sel_edges] == [(int(g[4][e]), int(g[5][e]), float(g[6][e])) for e in order]
    assert close(esp.last_gains, gains, 1e-9)
    res, sel, t = esp.subset(ks[2])              # lazy: the reference's 3-tuple
    assert np.array_equal(res, results[2]) and len(sel) == ks[2] and t >= 0


@pytest.mark.parametrize("case", ["sphere2500", "er300", "er2000"])
def test_selection_parity_with_restatement(case):
    if case == "sphere2500":
        g, K = arrays(load_golden("g2o_sphere2500")), 600
    elif case == "er300":
        g = chain_er(300, 0.03, 0); K = len(g[6])
    else:
        g, K = chain_er(2000, 0.001, 0), 1000
    order, gains, margins = R.greedy(*g, K)
    assert margins.min() > 1e-9              # the seeds are chosen so that the sequence is pinned
    esp = esp_of(*g)
    res, sel = esp.subset(K)
    assert np.array_equal(np.nonzero(res)[0], np.sort(order))
    assert [(e.i, e.j) for e in sel] == [(int(g[4][e]), int(g[5][e])) for e in order]
    assert close(esp.last_gains, gains, 1e-9)


# ---- 3. log-det identity on the tie-heavy and the beta cases ----
@pytest.mark.parametrize("name,pct", [("city10000", 0.1), ("ais2klinik", 0.2)])
def test_logdet_identity(name, pct):
    g = arrays(load_golden("g2o_" + name))
    n, fi, fj, fw, ci, cj, cw = g
    K = int(pct * len(cw))
    esp = esp_of(*g)
    beta = esp.info()["beta"]
    assert beta == (1e-4 if name == "ais2klinik" else 0.0)
    res, _ = esp.subset(K)
    sel = np.nonzero(res)[0]
    assert len(sel) == K
    eye = beta * np.ones(n - 1)
    L0 = R.reduced_laplacian(n, fi, fj, fw, sparse=True) + sp.diags(eye)
    LK = R.reduced_laplacian(n, np.concatenate([fi, ci[sel]]), np.concatenate([fj, cj[sel]]),
                             np.concatenate([fw, cw[sel]]), sparse=True) + sp.diags(eye)
    growth = R.logdet_sparse(LK) - R.logdet_sparse(L0)
    assert abs(np.sum(np.log1p(esp.last_gains)) - growth) <= 1e-9 * abs(growth)


# ---- 4. weighted resistances after a run ----
def test_weighted_resistances_after_200_intel_picks_match_sparse_solves():
    g = arrays(load_golden("g2o_intel"))
    n, fi, fj, fw, ci, cj, cw = g
    esp = esp_of(*g)
    res, _ = esp.subset(200)
    sel = np.nonzero(res)[0]
    r = esp.weighted_resistances()
    LK = R.reduced_laplacian(n, np.concatenate([fi, ci[sel]]), np.concatenate([fj, cj[sel]]), np.concatenate([fw, cw[sel]]),
                             sparse=True)
    A = np.zeros((n, len(cw)))
    A[ci, np.arange(len(cw))] += 1.0
    A[cj, np.arange(len(cw))] -= 1.0
    A = A[1:]
    X = splu(LK).solve(A)
    ref = cw * np.einsum("ij,ij->j", A, X)
    assert close(r, ref, 1e-9)


# ---- 5. fold invariance and determinism ----
def test_fold_invariance_and_bitwise_repeatability():
    g = arrays(load_golden("g2o_intel"))
    m = len(g[6])
    runs = {}
    for fold in (1, 7, 64):
        esp = esp_of(*g, fold=fold)
        res, sel = esp.subset(m)
        runs[fold] = ([(e.i, e.j, e.weight) for e in sel], esp.last_gains.copy())
        if fold == 64:
            r1 = esp.weighted_resistances()
            assert [(e.i, e.j, e.weight) for e in esp.subset(m)[1]] == runs[64][0]
            assert np.array_equal(esp.last_gains, runs[64][1])
            assert np.array_equal(esp.weighted_resistances(), r1)
    for fold in (1, 7):
        assert runs[fold][0] == runs[64][0]
        assert close(runs[fold][1], runs[64][1], 1e-12)


# ---- 6. edge cases ----
def test_edge_cases_duplicates_node0_selfloop_parallel():
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
    esp = esp_of(n, fi, fj, fw, ci, cj, cw)
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


def test_reference_assertions_and_error_paths():
    g = chain_er(50, 0.1, 1)
    esp = esp_of(*g)
    m = len(g[6])
    for bad in (0, m + 1):
        with pytest.raises(AssertionError):
            esp.subset(bad)
    with pytest.raises(AssertionError):
        esp.subsets_lazy([5, 3])
    with pytest.raises(AssertionError):
        esp.subsets_lazy([0, 3])
    n, fi, fj, fw, ci, cj, cw = g
    keep = (fi != 48)                               # node 49 loses its only fixed edge
    with pytest.raises(_lib.Disconnected):
        esp_of(n, fi[keep], fj[keep], fw[keep], ci, cj, cw)
    with pytest.raises(AssertionError, match="32768"):
        big = 40000
        esp_of(big, np.arange(big - 1), np.arange(1, big), np.ones(big - 1), [0], [7], [1.0])


# ---- 7. end to end, like examples/g2o_experiment.py --run-greedy ----
def test_intel_greedy_results_through_mac_evaluate_objective():
    g = arrays(load_golden("g2o_intel"))
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    ks = [int(p * m) for p in np.linspace(0.1, 1.0, 10)]
    order, _, _ = R.greedy(*g, m)
    fixed, cand = edges(fi, fj, fw), edges(ci, cj, cw)
    esp = GreedyESP(fixed, cand, n, lazy=True)
    results, _, _ = esp.subsets_lazy(ks)
    mac = MAC(fixed, cand, n)
    for k, r in zip(ks, results):
        lam = mac.evaluate_objective(r)
        Lf = weight_graph_lap_from_edge_list(fixed + [cand[e] for e in order[:k]], n).toarray()      # the restatement's pick
        ref = scipy.linalg.eigh(Lf, eigvals_only=True, subset_by_index=[1, 1])[0]
        assert abs(lam - ref) <= 1e-8 * max(1.0, abs(ref))
