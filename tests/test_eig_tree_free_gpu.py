"""GreedyEig's spanning-tree matrix-free route on the GPU (mac_amd/csrc/eig_free_tree.h; GreedyEig(..., matrix_free="tree")).

The preconditioner only proposes directions, so the sweeps over the tree, the seeds in the history, the projection and the
back-substitution are pinned the way tests/test_eig_free_gpu.py pins the chain route's kernels: by ``info()["applications"]`` against
the NumPy restatement with the exact preconditioner, |applications - A_ref| <= D / 4, D from deliberately damaged variants of
tests/eig_tree_free_restatement.py (never from the device; tests/test_eig_tree_free_host.py asserts D >= 0.05 A_ref, that
rounding-size noise stays under D / 20, and that the recorded A_ref and D of tests/golden/eig_tree_free_reference.json are what the
restatement computes).  Values are checked against the dense general form and tests/eig_restatement.py with the tolerances
tests/test_eig_gpu.py states: a reported lambda_2 is within 1e-8 ||L_e||_inf of an eigenvalue, a bound within 1e-10 relative.

Measured on the MI355X: the largest |applications - A_ref| over every case of this module is 3 applications (the smallest allowance
46.75), 0.043 of the allowance at the most; lambda_2 of the tree route and the dense general form differ by 5.5e-10 of
1e-8 ||L||_inf at the most; at n = 20 000 lambda_2 is within 1.3e-10 of 1e-8 ||L||_inf of the shift-invert solve.  The bounds of the
two routes differ by 2.9e-14 relative at the most, after create and after the run.  Against the restatement's bounds (numpy.linalg.eigh's
vector) they are within 7e-13 after create on all three inputs and, after the run, within 8e-14 / 1.5e-13 on deep150 / deep129 but
6.43e-8 on general150 -- on BOTH routes: after those 10 picks lambda_2 / lambda_3 = 0.983 and the polish of the winner's pair (stop
once three iterations in a row have not halved the best residual) ends at a relative residual of 1.4e-9; the NumPy restatement with the
exact preconditioner ends there too (64 iterations, 5.5e-8).  That comparison is therefore held to what the stop rule promises."""
import numpy as np
import pytest

import eig_free_restatement as F
import eig_lobpcg_restatement as Q
import eig_restatement as R
import eig_tree_free_restatement as T
import test_eig_gpu
from mac_amd import _lib

pytestmark = pytest.mark.gpu

_made = []
FORCED = dict(eig_free_rows=T.ROWS, eig_free_split=T.SPLIT)
LD = {"general150": 192, "deep150": 192, "deep129": 128}
SEEDS = {"general150": 74, "deep150": 5, "deep129": 5}


def eig_of(g, options=None, **kw):
    kw.setdefault("matrix_free", "tree")
    with _lib.default_options(**(options or {})):
        ge = test_eig_gpu.eig_of(*g, **kw)
    _made.append(ge)
    return ge


@pytest.fixture(autouse=True)
def no_handle_outlives_its_test():
    yield
    for ge in _made:
        ge._dev.close()
    _made.clear()


def picks_of(g, sel):
    return [int(np.nonzero((g[4] == e.i) & (g[5] == e.j) & (g[6] == e.weight))[0][0]) for e in sel]


def check_counts(tag, apps, ref):
    dev = np.asarray(apps, dtype=np.float64) - ref["A"]
    print(f"{tag}: largest |deviation| {int(np.max(np.abs(dev)))}, smallest allowance {float(np.min(ref['D'] / 4))}, "
          f"largest |deviation| / allowance {float(np.max(np.abs(dev) / (ref['D'] / 4))):.3f}")
    assert np.all(np.abs(dev) <= ref["D"] / 4)


# ---- 1. applications per pick are the exact preconditioner's ----
@pytest.mark.parametrize("options", [None, FORCED], ids=["automatic", "rows32_split3"])
@pytest.mark.parametrize("name,K,batch", T.CASES)
def test_applications_per_pick_are_those_of_the_exact_preconditioner(name, K, batch, options):
    ref = T.recorded(name, K, batch)
    g = T.graph(name)
    r = SEEDS[name]
    ge = eig_of(g, options, batch=batch)
    inf = ge.info()
    assert inf["form"] == "tree_free" and inf["fold"] == 0 and inf["batch"] == batch and inf["ld"] == LD[name]
    assert inf["seeds"] == r and inf["pending"] == r
    sol, sel = ge.subset(K)
    inf = ge.info()
    assert picks_of(g, sel) == ref["order"].tolist()
    assert np.array_equal(inf["solved"], ref["solved"])
    assert inf["form"] == "tree_free" and inf["fold"] == 0 and inf["seeds"] == r and inf["pending"] == r + K and inf["ld"] == LD[name]
    check_counts(f"{name} K {K} batch {batch} {options}", inf["applications"], ref)


# ---- 2. agreement with the dense general form ----
@pytest.mark.parametrize("name", T.NAMES)
def test_values_and_picks_agree_with_the_dense_general_form(name):
    g = T.graph(name)
    n, fi, fj, fw, ci, cj, cw = g
    K = Q.K_PICKS
    free, dense = eig_of(g), eig_of(g, matrix_free=False)
    assert free.info()["form"] == "tree_free" and dense.info()["form"] == "dense"
    L = R.laplacian(n, fi, fj, fw)

    def check_candidates(tag, L, selected):
        """lambda_2 of every candidate against the secular restatement; the bounds against the dense general form's to 1e-10
        relative (the two handles are in the same state), and against the restatement's to what the stop rule promises."""
        tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
        ref, uref = R.values_secular(L, ci, cj, cw), R.bounds(L, ci, cj, cw)
        lam, u, ud = free.candidate_lambda2(), free.candidate_bounds(), dense.candidate_bounds()
        keep = np.ones(len(cw), dtype=bool)
        keep[selected] = False
        assert np.all(np.isnan(lam[~keep])) and np.all(np.isnan(u[~keep])) and np.all(np.isnan(ud[~keep]))
        rel_dense = float(np.max((np.abs(u - ud) / np.abs(ud))[keep]))
        rel_ref = float(np.max((np.abs(u - uref) / np.abs(uref))[keep]))
        print(name, tag, "max |lambda2 - ref| / tol", float(np.max(np.abs(lam - ref)[keep] / tol[keep])),
              "max rel bound difference from the dense general form", rel_dense, "from the restatement", rel_ref)
        assert np.all(np.abs(lam - ref)[keep] <= tol[keep]) and np.all((u >= lam - tol)[keep])
        assert np.all((np.abs(u - ud) <= 1e-10 * np.abs(ud))[keep])
        # The restatement's bounds come from numpy.linalg.eigh's vector, the device's from a pair that obeys the stop rule
        # ||r||_1 < 1e-8 ||L||_inf (and is polished beyond it as far as the polish gets: tests/test_eig_gpu.py checks 1e-10 on fresh
        # handles, where it gets far).  With ||r||_2 <= ||r||_1 and gap = lambda_3 - lambda_2 the vector is within
        # sin(theta) <= ||r||_2 / gap of the true one, a difference d = v_i - v_j within delta = 2 sin(theta), so
        # |u - uref| <= |lambda - lambda_ref| + w (2 |d| delta + delta^2).
        ev = np.linalg.eigvalsh(L)
        normL = R.norm_inf(L)
        delta = 2.0 * 1e-8 * normL / (ev[2] - ev[1])
        d = np.sqrt(np.maximum(uref - ev[1], 0.0) / cw)
        assert np.all((np.abs(u - uref) <= 1e-8 * normL + cw * (2.0 * d * delta + delta * delta))[keep])
        return rel_ref
    assert abs(free.info()["lambda2"] - R.fiedler(L)[0]) <= 1e-8 * R.norm_inf(L)
    assert check_candidates("after create", L, []) <= 1e-10          # (a fresh handle: the polish reaches rounding, as in test_eig_gpu.py)
    (_, sf), (_, sd) = free.subset(K), dense.subset(K)
    order = picks_of(g, sf)
    assert order == picks_of(g, sd)
    Lk = R.laplacian(n, np.concatenate([fi, ci[order]]), np.concatenate([fj, cj[order]]), np.concatenate([fw, cw[order]]))
    print(name, "max |lambda2 tree - dense| / (1e-8 ||L||)", float(np.max(np.abs(free.last_lambda2 - dense.last_lambda2)) / (1e-8 * R.norm_inf(Lk))))
    assert np.all(np.abs(free.last_lambda2 - dense.last_lambda2) <= 1e-8 * R.norm_inf(Lk))
    check_candidates("after the run", Lk, order)


# ---- 3. a chain as the fixed graph: r = 0, preorder is the identity ----
@pytest.mark.parametrize("name", ["chain150", "chain129"])
def test_a_chain_runs_as_the_chain_route_does(name):
    g = F.graph(name)
    n, fi, fj, fw, ci, cj, cw = g
    K = Q.K_PICKS
    tree, chain = eig_of(g), eig_of(g, matrix_free=True)
    inf = tree.info()
    assert inf["form"] == "tree_free" and inf["seeds"] == 0 and inf["pending"] == 0 and chain.info()["form"] == "chain_free"
    (_, st), (_, sc) = tree.subset(K), chain.subset(K)
    order = picks_of(g, st)
    assert order == picks_of(g, sc)
    assert np.array_equal(tree.info()["solved"], chain.info()["solved"]) and tree.info()["pending"] == K
    Lk = R.laplacian(n, np.concatenate([fi, ci[order]]), np.concatenate([fj, cj[order]]), np.concatenate([fw, cw[order]]))
    print(name, "max |lambda2 tree - chain| / (1e-8 ||L||)", float(np.max(np.abs(tree.last_lambda2 - chain.last_lambda2)) / (1e-8 * R.norm_inf(Lk))),
          "applications", tree.info()["applications"].tolist(), chain.info()["applications"].tolist())
    assert np.all(np.abs(tree.last_lambda2 - chain.last_lambda2) <= 1e-8 * R.norm_inf(Lk))


# ---- 4. repeatability ----
def test_runs_repeat_bit_for_bit_and_the_history_grows_around_its_seeds():
    g = T.graph("deep150")
    r = SEEDS["deep150"]
    ge, fresh = eig_of(g, batch=64), eig_of(g, batch=64)

    def run(h, K):
        order, lam, _ = h._dev.select(K)
        inf = h.info()
        assert inf["pending"] == r + K and inf["seeds"] == r
        return order.copy(), lam.copy(), inf["solved"], inf["applications"]
    small = run(ge, 4)                      # a smaller budget first: the history is made for r + 4 columns, then grown, the seeds copied
    runs = [run(ge, Q.K_PICKS), run(ge, Q.K_PICKS), run(fresh, Q.K_PICKS)]
    again = run(ge, 4)
    for a, b in [(runs[0], runs[1]), (runs[0], runs[2]), (small, again)]:
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for q in range(4):
        assert np.array_equal(small[q], runs[0][q][:4])


# ---- 5. edge cases ----
def _check_small(g):
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    L = R.laplacian(n, fi, fj, fw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(g)
    inf = ge.info()
    assert inf["form"] == "tree_free" and inf["ld"] == 64 and abs(inf["lambda2"] - R.fiedler(L)[0]) <= 1e-8 * R.norm_inf(L)
    lam, u = ge.candidate_lambda2(), ge.candidate_bounds()
    assert np.all(np.abs(lam - R.values_brute(L, ci, cj, cw)) <= tol)
    uref = R.bounds(L, ci, cj, cw)
    assert np.all(np.abs(u - uref) <= 1e-10 * np.abs(uref)) and np.all(u >= lam - tol)
    order, lam2, _ = ge._dev.select(m)
    assert sorted(order.tolist()) == list(range(m)) and ge.info()["pending"] == inf["seeds"] + m
    r = R.greedy(*g, m, method="brute", order=order)
    for k in range(m):
        tolL = 1e-8 * r["norms"][k].max()
        assert r["lam2"][k] >= np.nanmax(r["values"][k]) - 1e-8 - 2 * tolL and abs(lam2[k] - r["lam2"][k]) <= tolL
    return inf


@pytest.mark.parametrize("shape", ["n2", "n3_path_node0_leaf", "n3_star_node0_hub", "n3_triangle", "star6_node0_hub", "star6_node0_leaf"])
def test_small_graphs_paths_and_stars(shape):
    fixed = {"n2": (2, [1], [0]), "n3_path_node0_leaf": (3, [0, 1], [1, 2]), "n3_star_node0_hub": (3, [1, 0], [0, 2]),
             "n3_triangle": (3, [0, 1, 2], [1, 2, 0]), "star6_node0_hub": (6, [0] * 5, [1, 2, 3, 4, 5]),
             "star6_node0_leaf": (6, [3] * 5, [0, 1, 2, 4, 5])}[shape]
    n, fi, fj = fixed
    fw = np.array([1.5, 0.75, 1.25, 0.5, 2.0])[:len(fi)]
    cand = [(0, n - 1, 2.0), (n - 1, 0, 0.5), (1, 1, 3.0)] + ([(1, 2, 1e-3)] if n >= 3 else []) + ([(4, 5, 0.7), (2, 0, 1.1)] if n == 6 else [])
    g = (n, np.array(fi), np.array(fj), fw, np.array([c[0] for c in cand]), np.array([c[1] for c in cand]), np.array([c[2] for c in cand]))
    inf = _check_small(g)
    assert inf["seeds"] == (1 if shape == "n3_triangle" else 0) == inf["pending"]


def test_edge_cases_duplicates_node0_selfloop_parallel():
    g = test_eig_gpu.edge_case_graph("branching")
    n, fi, fj, fw, ci, cj, cw = g
    m, loop = len(cw), 3
    L = R.laplacian(n, fi, fj, fw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(g)
    assert ge.info()["form"] == "tree_free" and ge.info()["seeds"] == 0
    lam, u = ge.candidate_lambda2(), ge.candidate_bounds()
    ref, uref = R.values_brute(L, ci, cj, cw), R.bounds(L, ci, cj, cw)
    assert np.all(np.abs(lam - ref) <= tol)
    assert np.all(np.abs(u - uref) <= 1e-10 * np.abs(uref)) and np.all(u >= lam - tol)
    assert u[loop] == ge.info()["lambda2"] and abs(lam[loop] - R.fiedler(L)[0]) <= tol[loop]
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
        if order[k] == loop:
            others = np.delete(vals, loop)
            assert np.all(np.isnan(others)) or np.nanmax(others) - r["lam_before"][k] <= 1e-8 + 2 * tolL


def test_parallel_fixed_edges_and_a_fixed_self_loop_are_one_link():
    n, fi, fj, fw, ci, cj, cw = test_eig_gpu.edge_case_graph("branching")
    g = (n, np.concatenate([fi, fj[:3], [4]]), np.concatenate([fj, fi[:3], [4]]), np.concatenate([fw, [0.3, 0.6, 0.9, 5.0]]), ci, cj, cw)
    inf = _check_small(g)
    assert inf["seeds"] == 0


@pytest.mark.parametrize("batch", [1, 48])
def test_small_batches_pick_what_the_full_batch_picks(batch):
    g = T.graph("deep129")
    n, fi, fj, fw, ci, cj, cw = g
    K = 3 if batch == 1 else 5
    full, small = eig_of(g), eig_of(g, batch=batch)
    assert small.info()["batch"] == batch
    (_, sa), (_, sb) = full.subset(K), small.subset(K)
    order = picks_of(g, sa)
    assert order == picks_of(g, sb) == T.recorded("deep129", Q.K_PICKS, 512)["order"][:K].tolist()
    Lk = R.laplacian(n, np.concatenate([fi, ci[order]]), np.concatenate([fj, cj[order]]), np.concatenate([fw, cw[order]]))
    assert np.all(np.abs(full.last_lambda2 - small.last_lambda2) <= 1e-8 * R.norm_inf(Lk))


# ---- 6. past the dense limit ----
def big_tree(n=20000, extra=20, m=300, seed=7):
    rng = np.random.default_rng(seed)
    k = np.arange(1, n)
    par = rng.integers(0, k)
    xi = rng.integers(0, n, extra)
    xj = (xi + rng.integers(1, n, extra)) % n
    fi, fj = np.concatenate([k, xi]), np.concatenate([par, xj])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = rng.integers(0, n, m)
    cj = (ci + rng.integers(1, n, m)) % n
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, m)


def test_a_general_graph_past_the_dense_limit_selects_and_reports_lambda2():
    """n = 20 000, a random recursive tree plus 20 fixed links: the dense route refuses it.  lambda_2 of the fixed graph and after
    every pick against a sparse shift-invert solve, to the stop rule's own 1e-8 ||L||_inf."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    g = big_tree()
    n, fi, fj, fw, ci, cj, cw = g
    K = 3
    with pytest.raises(AssertionError, match="BAD_ARG.*16384"):
        eig_of(g, matrix_free=False)
    ge = eig_of(g)
    inf = ge.info()
    assert inf["form"] == "tree_free" and inf["ld"] == 20032 and inf["seeds"] == 20 == inf["pending"]
    lam0 = inf["lambda2"]
    order, lam, _ = ge._dev.select(K)
    order2, lam_again, _ = ge._dev.select(K)
    assert np.array_equal(order, order2) and np.array_equal(lam, lam_again) and len(set(order.tolist())) == K
    assert ge.info()["pending"] == 20 + K

    def lap(sel):
        a = np.concatenate([fi, ci[sel]]); b = np.concatenate([fj, cj[sel]]); w = np.concatenate([fw, cw[sel]])
        A = sp.coo_matrix((w, (a, b)), shape=(n, n))
        A = A + A.T
        return (sp.diags(np.asarray(A.sum(axis=1)).ravel()) - A).tocsc()
    got = np.concatenate([[lam0], lam])
    for k in range(K + 1):
        Lk = lap(order[:k])
        norm = float(abs(Lk).sum(axis=1).max())
        ref = np.sort(spla.eigsh(Lk, k=2, sigma=-0.5 * got[k], which="LM", return_eigenvectors=False))[1]
        print(f"n = {n}, after {k} picks: lambda_2 {got[k]:.6e}, shift-invert {ref:.6e}, |error| / (1e-8 ||L||_inf) "
              f"{abs(got[k] - ref) / (1e-8 * norm):.3e}, lambda_2 / ||L||_inf {ref / norm:.3e}")
        assert abs(got[k] - ref) <= 1e-8 * norm
        assert k == 0 or got[k] >= got[k - 1] - 1e-8 * norm


# ---- 7. refusals on the device ----
def test_exchange_is_refused_and_the_handle_still_selects():
    g = T.graph("deep150")
    ge = eig_of(g)
    sol, sel = ge.subset(4)
    with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_EIG_MATRIX_FREE"):
        ge.exchange(sol)
    inf = ge.info()
    assert inf["pending"] == SEEDS["deep150"] + 4 and inf["form"] == "tree_free"
    sol2, sel2 = ge.subset(4)
    assert sel2 == sel and np.array_equal(sol, sol2)


def test_a_history_that_cannot_fit_is_refused_before_anything_is_allocated():
    n, m, r = 40000, 1200000, 3                # 8 ld (r + K) = 384 GB: more than the device has in all
    rng = np.random.default_rng(0)
    k = np.arange(1, n)
    fi, fj = np.concatenate([k, [10, 200, 3000]]), np.concatenate([k // 2, [39000, 25000, 7]])      # a binary heap's tree plus r links
    dev = _lib.Eig(n, fi, fj, np.ones(n - 1 + r), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m), batch=64,
                   matrix_free="tree")
    try:
        inf = dev.info()
        ld = inf["ld"]
        assert inf["form"] == "tree_free" and inf["seeds"] == r == inf["pending"]
        with pytest.raises(AssertionError) as ei:
            dev.select(m)
        msg = str(ei.value)
        assert "BAD_ARG" in msg and "does not fit" in msg and f"n = {n}" in msg and f"K = {m}" in msg and f"r = {r}" in msg
        assert str(8 * ld * (r + m)) in msg
        after = dev.info()
        assert after["pending"] == r and after["lambda2"] == inf["lambda2"] and len(after["solved"]) == 0      # no run happened, the seeds stay
        u = dev.candidate_bounds()             # and the handle still answers
        assert np.all(u >= inf["lambda2"])
    finally:
        dev.close()
