"""GreedyEig's matrix-free route on the GPU (mac_amd/csrc/eig_free.h; GreedyEig(..., matrix_free=True)).

The preconditioner only proposes directions, so the scans, the projection and the back-substitution are pinned the way
tests/test_eig_precond_gpu.py pins the dense route's kernels: by ``info()["applications"]`` against the NumPy restatement with the
exact preconditioner, |applications - A_ref| <= D / 4, D from deliberately damaged variants of tests/eig_free_restatement.py (never
from the device; tests/test_eig_free_host.py asserts D >= 0.05 A_ref and that rounding-size noise stays under D / 20).  Values are
checked against the dense chain form and tests/eig_restatement.py with the tolerances tests/test_eig_gpu.py states: a reported
lambda_2 is within 1e-8 ||L_e||_inf of an eigenvalue, a bound within 1e-10 relative.

Measured on the MI355X: the largest |applications - A_ref| over every case of this module is 4 applications (the smallest allowance
58.75), 0.028 of the allowance at the most; lambda_2 of the two routes differs by 1.9e-9 of 1e-8 ||L||_inf at the most."""
import numpy as np
import pytest

import eig_free_restatement as F
import eig_lobpcg_restatement as Q
import eig_restatement as R
import test_eig_gpu
from mac_amd import _lib

pytestmark = pytest.mark.gpu

_made = []
FORCED = dict(eig_free_rows=F.ROWS, eig_free_split=F.SPLIT)
LD = {"chain150": 192, "chain129": 128, "long66": 128}


def eig_of(g, options=None, **kw):
    kw.setdefault("matrix_free", True)
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
@pytest.mark.parametrize("name,K,batch", F.CASES)
def test_applications_per_pick_are_those_of_the_exact_preconditioner(name, K, batch, options):
    ref = F.reference(name, K, batch)
    g = F.graph(name)
    ge = eig_of(g, options, batch=batch)
    inf = ge.info()
    assert inf["form"] == "chain_free" and inf["fold"] == 0 and inf["batch"] == batch and inf["ld"] == LD[name] and inf["pending"] == 0
    sol, sel = ge.subset(K)
    inf = ge.info()
    assert picks_of(g, sel) == ref["run"]["order"].tolist()
    assert np.array_equal(inf["solved"], ref["run"]["solved"])
    assert inf["form"] == "chain_free" and inf["fold"] == 0 and inf["pending"] == K and inf["ld"] == LD[name]
    check_counts(f"{name} K {K} batch {batch} {options}", inf["applications"], ref)


# ---- 2. agreement with the dense chain form ----
@pytest.mark.parametrize("name,K", [("chain150", Q.K_PICKS), ("chain129", Q.K_PICKS), ("long66", F.K_LONG)])
def test_values_and_picks_agree_with_the_dense_chain_form(name, K):
    g = F.graph(name)
    n, fi, fj, fw, ci, cj, cw = g
    free, dense = eig_of(g), eig_of(g, matrix_free=False)
    assert free.info()["form"] == "chain_free" and dense.info()["form"] == "chain"
    L = R.laplacian(n, fi, fj, fw)

    def check_candidates(tag, L, selected):
        tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
        ref, uref = R.values_secular(L, ci, cj, cw), R.bounds(L, ci, cj, cw)
        lam, u = free.candidate_lambda2(), free.candidate_bounds()
        keep = np.ones(len(cw), dtype=bool)
        keep[selected] = False
        assert np.all(np.isnan(lam[~keep])) and np.all(np.isnan(u[~keep]))
        print(name, tag, "max |lambda2 - ref| / tol", float(np.max(np.abs(lam - ref)[keep] / tol[keep])),
              "max rel bound error", float(np.max((np.abs(u - uref) / np.abs(uref))[keep])))
        assert np.all(np.abs(lam - ref)[keep] <= tol[keep])
        assert np.all((np.abs(u - uref) <= 1e-10 * np.abs(uref))[keep]) and np.all((u >= lam - tol)[keep])
    assert abs(free.info()["lambda2"] - R.fiedler(L)[0]) <= 1e-8 * R.norm_inf(L)
    check_candidates("after create", L, [])
    (_, sf), (_, sd) = free.subset(K), dense.subset(K)
    order = picks_of(g, sf)
    assert order == picks_of(g, sd)
    Lk = R.laplacian(n, np.concatenate([fi, ci[order]]), np.concatenate([fj, cj[order]]), np.concatenate([fw, cw[order]]))
    print(name, "max |lambda2 free - dense| / (1e-8 ||L||)", float(np.max(np.abs(free.last_lambda2 - dense.last_lambda2)) / (1e-8 * R.norm_inf(Lk))))
    assert np.all(np.abs(free.last_lambda2 - dense.last_lambda2) <= 1e-8 * R.norm_inf(Lk))
    check_candidates("after the run", Lk, order)


# ---- 3. repeatability ----
def test_runs_repeat_bit_for_bit_and_a_smaller_budget_first_changes_nothing():
    g = F.graph("chain150")
    ge, fresh = eig_of(g, batch=64), eig_of(g, batch=64)

    def run(h, K):
        order, lam, _ = h._dev.select(K)
        inf = h.info()
        assert inf["pending"] == K
        return order.copy(), lam.copy(), inf["solved"], inf["applications"]
    small = run(ge, 4)                      # a smaller budget first: the history is made for 4 columns, then grown
    runs = [run(ge, Q.K_PICKS), run(ge, Q.K_PICKS), run(fresh, Q.K_PICKS)]
    again = run(ge, 4)                      # the history never shrinks: 4 picks in the room of 10
    for a, b in [(runs[0], runs[1]), (runs[0], runs[2]), (small, again)]:
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(small[0], runs[0][0][:4]) and np.array_equal(small[1], runs[0][1][:4])
    assert np.array_equal(small[2], runs[0][2][:4]) and np.array_equal(small[3], runs[0][3][:4])


# ---- 4. edge cases ----
def test_edge_cases_duplicates_node0_selfloop_parallel():
    g = test_eig_gpu.edge_case_graph("chain")
    n, fi, fj, fw, ci, cj, cw = g
    m, loop = len(cw), 3
    L = R.laplacian(n, fi, fj, fw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(g)
    assert ge.info()["form"] == "chain_free"
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


@pytest.mark.parametrize("n", [2, 3])
def test_two_and_three_node_graphs(n):
    fi, fj, fw = np.arange(1, n), np.arange(n - 1), np.array([1.5, 0.75])[:n - 1]
    cand = [(0, n - 1, 2.0), (n - 1, 0, 0.5), (1, 1, 3.0)] + ([(1, 2, 1e-3)] if n == 3 else [])
    g = (n, fi, fj, fw, np.array([c[0] for c in cand]), np.array([c[1] for c in cand]), np.array([c[2] for c in cand]))
    ci, cj, cw = g[4:]
    m = len(cw)
    L = R.laplacian(n, fi, fj, fw)
    tol = 1e-8 * R.norm_inf_with(L, ci, cj, cw)
    ge = eig_of(g)
    inf = ge.info()
    assert inf["form"] == "chain_free" and inf["ld"] == 64 and abs(inf["lambda2"] - R.fiedler(L)[0]) <= 1e-8 * R.norm_inf(L)
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


@pytest.mark.parametrize("batch", [1, 48])
def test_small_batches_pick_what_the_full_batch_picks(batch):
    g = Q.graph("chain40")
    n, fi, fj, fw, ci, cj, cw = g
    K = 5
    full, small = eig_of(g), eig_of(g, batch=batch)
    assert small.info()["batch"] == batch
    (_, sa), (_, sb) = full.subset(K), small.subset(K)
    order = picks_of(g, sa)
    assert order == picks_of(g, sb)
    Lk = R.laplacian(n, np.concatenate([fi, ci[order]]), np.concatenate([fj, cj[order]]), np.concatenate([fw, cw[order]]))
    assert np.all(np.abs(full.last_lambda2 - small.last_lambda2) <= 1e-8 * R.norm_inf(Lk))
    r = R.greedy(*g, K, method="brute", order=order)
    assert np.all(np.abs(small.last_lambda2 - r["lam2"]) <= 1e-8 * np.array([x.max() for x in r["norms"]]))


# ---- 5. past the dense limit ----
def test_a_chain_past_the_dense_limit_selects_and_reports_lambda2():
    """n = 33 000: the dense route refuses it.  lambda_2 / ||L||_inf is 1.2e-9 ... 9.7e-9 here, below the stop rule's 1e-8: the rule
    certifies little more than the sign (Regime), so the picks' identity is not asserted -- the reported values
    are, to the rule's own 1e-8 ||L||_inf, against a sparse shift-invert solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    n, m, K = 33000, 300, 3
    rng = np.random.default_rng(7)
    fi = np.arange(n - 1)
    fw = rng.uniform(50.0, 200.0, n - 1)
    ci = rng.integers(0, n, m)
    cj = (ci + rng.integers(1, n, m)) % n
    cw = rng.uniform(50.0, 200.0, m)
    g = (n, fi, fi + 1, fw, ci, cj, cw)
    with pytest.raises(AssertionError, match="BAD_ARG.*32768"):
        eig_of(g, matrix_free=False)
    ge = eig_of(g)
    inf = ge.info()
    assert inf["form"] == "chain_free" and inf["ld"] == 33024
    lam0 = inf["lambda2"]
    order, lam, _ = ge._dev.select(K)
    order2, lam_again, _ = ge._dev.select(K)
    assert np.array_equal(order, order2) and np.array_equal(lam, lam_again) and len(set(order.tolist())) == K

    def lap(sel):
        a = np.concatenate([fi, ci[sel]]); b = np.concatenate([fi + 1, cj[sel]]); w = np.concatenate([fw, cw[sel]])
        A = sp.coo_matrix((w, (a, b)), shape=(n, n))
        A = A + A.T
        return (sp.diags(np.asarray(A.sum(axis=1)).ravel()) - A).tocsc()
    got = np.concatenate([[lam0], lam])
    for k in range(K + 1):
        Lk = lap(order[:k])
        norm = float(abs(Lk).sum(axis=1).max())
        ref = np.sort(spla.eigsh(Lk, k=2, sigma=-0.5 * got[k], which="LM", return_eigenvectors=False))[1]
        print(f"n = {n}, after {k} picks: lambda_2 {got[k]:.6e}, shift-invert {ref:.6e}, relative error {abs(got[k] - ref) / ref:.3e}, "
              f"|error| / (1e-8 ||L||_inf) {abs(got[k] - ref) / (1e-8 * norm):.3e}, lambda_2 / ||L||_inf {ref / norm:.3e}")
        assert abs(got[k] - ref) <= 1e-8 * norm
        assert k == 0 or got[k] >= got[k - 1] - 1e-8 * norm


# ---- 6. error paths on the device ----
def test_exchange_is_refused_and_the_handle_still_selects():
    g = F.graph("chain150")
    ge = eig_of(g)
    sol, sel = ge.subset(4)
    with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_EIG_MATRIX_FREE"):
        ge.exchange(sol)
    inf = ge.info()
    assert inf["pending"] == 4 and inf["form"] == "chain_free"
    sol2, sel2 = ge.subset(4)
    assert sel2 == sel and np.array_equal(sol, sol2)


def test_a_history_that_cannot_fit_is_refused_before_anything_is_allocated():
    n, m = 40000, 1200000                      # 8 ld K = 384 GB: more than the device has in all
    rng = np.random.default_rng(0)
    fi = np.arange(n - 1)
    dev = _lib.Eig(n, fi, fi + 1, np.ones(n - 1), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m), batch=64,
                   matrix_free=True)
    try:
        inf = dev.info()
        ld = inf["ld"]
        with pytest.raises(AssertionError) as ei:
            dev.select(m)
        msg = str(ei.value)
        assert "BAD_ARG" in msg and "does not fit" in msg and f"n = {n}" in msg and f"K = {m}" in msg and str(8 * ld * m) in msg
        after = dev.info()
        assert after["pending"] == 0 and after["lambda2"] == inf["lambda2"] and len(after["solved"]) == 0      # no run happened, no history was made
        u = dev.candidate_bounds()             # and the handle still answers
        assert np.all(u >= inf["lambda2"])
    finally:
        dev.close()
