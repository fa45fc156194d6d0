"""GreedyEig's preconditioner on the GPU, pinned through the operator applications the library reports.

Sigma only proposes search directions: every lambda_2, pick and swap is decided by the sparse L_cur, so k_eig_z, k_eig_product, the
rank-(pending + 1) correction of k_eig_rr, the folds and the exchange's trial column can be subtly wrong with every value right.
What a wrong preconditioner does cost is iterations, and ``info()["applications"]`` / the exchange's ``applies`` count them: one
per column per iteration in which the column is still active after the residual test.

Reference: tests/eig_lobpcg_restatement.py, the same recurrence in NumPy with the exact preconditioner (a float64 inverse of every
column's own reduced Laplacian): A_ref[k] per pick or round.  Allowance: D[k] / 4, two-sided (too few applications means a stop rule
retired a column early), D[k] the smallest excess of any restated variant with one term broken that can differ at k -- computed
from the restatement here, never from the device.  tests/test_eig_precond_host.py asserts on the same inputs that D >= 0.05 A_ref,
that rounding-size noise stays under D / 20, and that the prune decisions of the batch-64 case and of the exchange round have
margins that pin the set of solved columns.  A quarter sits between the two with a factor of 4 or more on either side.

Measured on the MI355X: the largest |applications - A_ref| over every case of this module is 3 applications (A_ref between 812 and
7643 per pick, the smallest allowance 63.75), 0.026 of the allowance at the most; the exchange round's 5619 are met exactly."""
import numpy as np
import pytest

import eig_lobpcg_restatement as Q
import test_eig_gpu

pytestmark = pytest.mark.gpu

_made = []


def eig_of(name, **kw):
    ge = test_eig_gpu.eig_of(*Q.graph(name), **kw)
    _made.append(ge)
    return ge


@pytest.fixture(autouse=True)
def no_handle_outlives_its_test():
    yield
    for ge in _made:
        ge._dev.close()
    _made.clear()


def picks_of(name, sel):
    g = Q.graph(name)
    return [int(np.nonzero((g[4] == e.i) & (g[5] == e.j) & (g[6] == e.weight))[0][0]) for e in sel]


def check_counts(tag, apps, ref):
    dev = np.asarray(apps, dtype=np.float64) - ref["A"]
    print(f"{tag}: applications {np.asarray(apps).tolist()}, A_ref {ref['A'].astype(int).tolist()}, deviation {dev.astype(int).tolist()}, "
          f"allowance {(ref['D'] / 4).tolist()}, largest |deviation| / allowance {float(np.max(np.abs(dev) / (ref['D'] / 4))):.3f}")
    assert np.all(np.abs(dev) <= ref["D"] / 4)


# ---- 1. the greedy: picks, solved columns and applications per pick ----
@pytest.mark.parametrize("name,fold,batch", Q.GREEDY_CASES)
def test_applications_per_pick_are_those_of_the_exact_preconditioner(name, fold, batch):
    ref = Q.greedy_reference(name, fold, batch)
    ge = eig_of(name, fold=fold, batch=batch)
    inf = ge.info()
    assert inf["fold"] == fold and inf["batch"] == batch and inf["form"] == ("dense" if name == "general150" else "chain")
    assert inf["ld"] == {"chain150": 192, "general150": 192, "chain129": 128}[name]
    sol, sel = ge.subset(Q.K_PICKS)
    inf = ge.info()
    assert picks_of(name, sel) == ref["run"]["order"].tolist()
    assert np.array_equal(inf["solved"], ref["run"]["solved"])
    assert inf["pending"] == Q.K_PICKS % fold
    check_counts(f"{name} fold {fold} batch {batch}", inf["applications"], ref)


# ---- 2. the Gauss-Jordan Sigma0 and the closed-form Sigma0 feed the same iteration ----
def test_dense_inverse_of_a_chain_counts_like_the_chain_form():
    ref = Q.greedy_reference("chain150", 3, 512)
    a, b = eig_of("chain150", fold=3), eig_of("chain150", fold=3, dense_inverse=True)
    assert a.info()["form"] == "chain" and b.info()["form"] == "dense"
    (_, sa), (_, sb) = a.subset(Q.K_PICKS), b.subset(Q.K_PICKS)
    assert picks_of("chain150", sa) == picks_of("chain150", sb) == ref["run"]["order"].tolist()
    check_counts("chain150 chain form", a.info()["applications"], ref)
    check_counts("chain150 dense inverse", b.info()["applications"], ref)


# ---- 3. round 0 of the exchange: removal columns, the trial column, the polish ----
@pytest.mark.parametrize("fold", Q.FOLDS)
def test_exchange_round_counts_are_those_of_the_exact_preconditioner(fold):
    """fold = 16 keeps the K = 8 loaded columns pending, so the trial column of every row lands next to them (fold = 3 folds them
    at the start of the round: 2 pending + 2 for a swap would not fit)."""
    ref = Q.exchange_reference(fold)
    run = ref["run"]
    ge = eig_of("chain40", fold=fold)
    sol, sel, info = ge.exchange(list(Q.exchange_start()), max_swaps=1)
    assert info["swaps"] == [run["swap"]] and len(info["solved"]) == 1
    assert info["solved"][0] == run["solved"] and info["removal_solves"][0] == Q.K_XCH
    check_counts(f"chain40 exchange fold {fold}", info["applies"][:1], ref)


# ---- 4. the counts are a function of the inputs ----
def test_select_counts_repeat_on_the_same_handle_and_on_a_fresh_one():
    ge, fresh = eig_of("chain150", fold=3, batch=64), eig_of("chain150", fold=3, batch=64)
    runs = []
    for h in (ge, ge, fresh):
        sol, sel = h.subset(Q.K_PICKS)
        inf = h.info()
        runs.append((sel, h.last_lambda2.copy(), inf["solved"], inf["applications"]))
    for sel, lam, solved, apps in runs[1:]:
        assert sel == runs[0][0] and np.array_equal(lam, runs[0][1]) and np.array_equal(solved, runs[0][2]) and np.array_equal(apps, runs[0][3])
