"""machip_lowest_pairs on the MI355X: the q lowest non-trivial eigenpairs, every column converged to the stop rule (DESIGN
section 24).  Each graph goes through Problem.lowest_pairs (L(x) assembled on the device) and find_lowest_pairs (a caller's CSR);
what is asserted of a result is tests/lowest_pairs_restatement.py::assert_pairs, against a dense eigh computed once per graph."""
import numpy as np
import pytest
import scipy.sparse as sp

import lowest_pairs_restatement as R
from conftest import load_golden
from mac_amd import _lib
from mac_amd.solvers import MAC
from mac_amd.utils.fiedler import find_fiedler_pair, find_lowest_pairs, reference_start_block
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu
TOL = 1e-8


def problem_of(n, i, j, w):
    """A handle whose L(x) is the graph's Laplacian: every edge but the last is fixed, the last is the one candidate, x = 1."""
    P = _lib.Problem(n, i[:-1], j[:-1], w[:-1], i[-1:], j[-1:], w[-1:])
    P.set_x(np.ones(1))
    return P


def golden_problem(name, x=None):
    g = load_golden(name)
    P = _lib.Problem(int(g["n"]), g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"])
    P.set_x(g["x"] if x is None else x)
    return P


def golden_L(name):
    g = load_golden(name)
    n = int(g["n"])
    return sp.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=(n, n))


def pose_case(name, at):
    g = load_golden(name)
    x = np.ones(len(g["cw"])) if at == "ones" else g["x_init"]
    return (lambda: golden_problem(name, x)), R.laplacian(*R.golden_graph(g, x))


def cases():
    out = {}
    for name, gr in R.small_graphs().items():
        out[name] = ((lambda gr=gr: problem_of(*gr)), R.laplacian(*gr), 4, 0)
    for name in ("er300_x0", "er2000_x0"):
        out[name] = ((lambda name=name: golden_problem(name)), golden_L(name), 4, 0)
    out["sphere2500_ones"] = pose_case("g2o_sphere2500", "ones") + (8, 0)
    out["sphere2500_init"] = pose_case("g2o_sphere2500", "init") + (8, 0)
    out["intel_init"] = pose_case("g2o_intel", "init") + (4, 20000)
    return out


CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_lowest_pairs_on_the_handle(name):
    make, L, q, max_steps = CASES[name]
    P = make()
    try:
        lams, V, info = P.lowest_pairs(q=q, tol=TOL, max_steps=max_steps, X0=R.reference_block(L.shape[0], q))
    finally:
        P.close()
    print(name, "handle", lams, info)
    R.assert_pairs(name, L, lams, V, info, TOL)
    assert info["reordered"] == int(info["first_rank"] != 0)


@pytest.mark.parametrize("name", list(CASES))
def test_find_lowest_pairs(name):
    _, L, q, max_steps = CASES[name]
    lams, V, info = find_lowest_pairs(L, q=q, tol=TOL, max_steps=max_steps)
    print(name, "csr", lams, info)
    R.assert_pairs(name, L, lams, V, info, TOL)
    assert info["gap"] == lams[1] - lams[0]


def test_exact_multiplicities_and_exhaustion():
    """K5: 5 four times, q = n - 1, every deflated column breaks down after one step.  C64: two exact double values.  P300: the
    deflated columns run their basis to n - 1 - c (more than 64 columns)."""
    for name, want in (("k5", np.full(4, 5.0)), ("petersen", np.full(4, 2.0)), ("star20", np.ones(4)),
                       ("c64", 2 - 2 * np.cos(2 * np.pi * np.array([1, 1, 2, 2]) / 64)), ("p300", 2 - 2 * np.cos(np.arange(1, 5) * np.pi / 300))):
        L = CASES[name][1]
        lams, _, info = find_lowest_pairs(L, q=4)
        assert np.abs(lams - want).max() <= TOL * R.lnorm_inf(L), (name, lams)
        if name == "k5":
            assert np.all(info["steps"][1:] <= _lib.PAIRS_CHUNK) and np.all(info["restarts"] == 0)
        if name == "p300":
            assert info["steps"].max() > 64


@pytest.mark.parametrize("name", ["er300_x0", "er2000_x0"])
def test_column_0_is_the_fiedler_solve(name):
    """Same start vector, same tolerance: same bits as machip_fiedler; and the handle's next Fiedler solve returns what it
    returns after a plain Fiedler solve in lowest_pairs' place."""
    n = CASES[name][1].shape[0]
    X = R.reference_block(n, 4)
    x0 = np.ascontiguousarray(X[:, 0])
    Pa, Pb = golden_problem(name), golden_problem(name)
    try:
        lams, V, info = Pa.lowest_pairs(q=4, tol=TOL, X0=X)
        lam, v, _ = Pb.fiedler(tol=TOL, x0=x0)
        assert info["reordered"] == 0
        assert lams[0] == lam and np.array_equal(V[:, 0], v)
        lam_a, v_a, _ = Pa.fiedler(tol=TOL, x0=x0)
        lam_b, v_b, _ = Pb.fiedler(tol=TOL, x0=x0)
        assert lam_a == lam_b and np.array_equal(v_a, v_b)
        ga, gb = Pa.gradient(), Pb.gradient()
        assert np.array_equal(ga, gb)
    finally:
        Pa.close(); Pb.close()


def test_every_column_obeys_the_stop_rule_where_the_x_block_does_not():
    """er300_x0: columns 1-3 of find_fiedler_pair's X are what the header says -- no eigenvectors; find_lowest_pairs' are."""
    L = CASES["er300_x0"][1]
    lnorm = R.lnorm_inf(L)
    _, _, X = find_fiedler_pair(L)
    lams, V, info = find_lowest_pairs(L, q=4)
    for c in (1, 2, 3):
        x = X[:, c]
        assert R.stop_rule_residual(L, float(x @ (L @ x)), x, lnorm) >= TOL
        assert R.stop_rule_residual(L, lams[c], V[:, c], lnorm) < TOL and info["residual"][c] < TOL


def test_order_check_on_the_mirror_graph():
    """Two mirrored clusters, v_2 vanishing where the landscape peaks: without the start's floor the Fiedler solve returns a true
    but higher eigenpair -- lowest_pairs still returns ev[1:5] in order and says so."""
    gr = R.mirror_graph()
    L = R.laplacian(*gr)
    ev, _, lnorm = R.dense_spectrum("mirror", L)
    n = gr[0]
    for floor in (0, None):
        P = problem_of(*gr)
        try:
            P.set_start(reference_start_block(n)[:, 0].copy())
            if floor is not None:
                P.set_option("start_floor_e6", floor)
            lam_plain, _, _ = P.fiedler(tol=TOL)
            lams, V, info = P.lowest_pairs(q=4, tol=TOL)
        finally:
            P.close()
        print("mirror floor", floor, lam_plain, lams, info)
        R.assert_pairs("mirror", L, lams, V, info, TOL)
        assert info["reordered"] == int(info["first_rank"] != 0)
        if abs(lam_plain - ev[2]) <= TOL * lnorm:
            assert info["reordered"] == 1 and info["first_rank"] == 1
        if floor is None:
            assert info["reordered"] == 0


def test_restarts_at_a_basis_cap():
    L = CASES["er300_x0"][1]
    X = R.reference_block(300, 4)
    Pa, Pb = golden_problem("er300_x0"), golden_problem("er300_x0")
    try:
        free, _, _ = Pa.lowest_pairs(q=4, tol=TOL, X0=X)
        Pb.set_option("pairs_vcap", 32)
        lams, V, info = Pb.lowest_pairs(q=4, tol=TOL, X0=X)
    finally:
        Pa.close(); Pb.close()
    print("vcap 32", info)
    R.assert_pairs("er300_x0", L, lams, V, info, TOL)
    assert np.all(info["restarts"][1:] >= 1) and np.all(info["steps"][1:] > 31)
    assert np.abs(lams - free).max() <= 2 * TOL * R.lnorm_inf(L)


def test_warm_block_ends_in_the_first_chunk():
    """The block fed back: every deflated column ends within its first chunk, because the check passes on the start vector itself.
    Column 0 is the unchanged Fiedler solve, which has its own first analysis point (192 steps here): it is bounded by the steps
    of the cold solve, not by the chunk."""
    L = CASES["er2000_x0"][1]
    P = golden_problem("er2000_x0")
    try:
        lams, V, info = P.lowest_pairs(q=4, tol=TOL, X0=R.reference_block(2000, 4))
        lams2, V2, info2 = P.lowest_pairs(q=4, tol=TOL, X0=V)
    finally:
        P.close()
    print("warm", info2)
    R.assert_pairs("er2000_x0", L, lams2, V2, info2, TOL)
    assert np.all(info2["steps"][1:] <= _lib.PAIRS_CHUNK) and info2["steps"][0] <= info["steps"][0]


@pytest.mark.parametrize("name", ["er2000_x0", "c64"])
def test_two_runs_return_the_same_bits(name):
    make, L, q, _ = CASES[name]
    out = []
    for _ in range(2):
        P = make()
        try:
            out.append(P.lowest_pairs(q=q, tol=TOL, X0=R.reference_block(L.shape[0], q)))
        finally:
            P.close()
    (l1, V1, i1), (l2, V2, i2) = out
    assert np.array_equal(l1, l2) and np.array_equal(V1, V2) and np.array_equal(i1["residual"], i2["residual"])
    assert np.array_equal(i1["steps"], i2["steps"])


def test_null_block_is_the_reference_block():
    """X0 = NULL: the stored start vector for column 0 and RandomState(7)'s columns 1 .. q-1, generated by the library itself --
    with the same column 0 (a Fiedler vector fed back, which the first check accepts) the two calls return the same bits."""
    L = CASES["er300_x0"][1]
    X = R.reference_block(300, 4)
    Pa, Pb = golden_problem("er300_x0"), golden_problem("er300_x0")
    try:
        _, v, _ = Pa.fiedler(tol=TOL, x0=X[:, 0].copy())
        X[:, 0] = v
        la, Va, ia = Pa.lowest_pairs(q=4, tol=TOL, X0=X)
        Pb.fiedler(tol=TOL, x0=R.reference_block(300, 4)[:, 0].copy())
        Pb.set_start(v)
        lb, Vb, ib = Pb.lowest_pairs(q=4, tol=TOL)
    finally:
        Pa.close(); Pb.close()
    R.assert_pairs("er300_x0", L, lb, Vb, ib, TOL)
    assert np.abs(la - lb).max() <= 2 * TOL * R.lnorm_inf(L)
    assert np.array_equal(ia["steps"][1:], ib["steps"][1:]) and np.array_equal(Va[:, 1:], Vb[:, 1:])


def test_block_gradient():
    g = load_golden("er300_x0")
    fixed = [Edge(int(a), int(b), float(w)) for a, b, w in zip(g["fi"], g["fj"], g["fw"])]
    cand = [Edge(int(a), int(b), float(w)) for a, b, w in zip(g["ci"], g["cj"], g["cw"])]
    mac = MAC(fixed, cand, int(g["n"]))
    lams, G, V = mac.problem_block(g["x"], 4)
    ci, cj, cw = g["ci"], g["cj"], g["cw"]
    for c in range(4):
        d = V[ci, c] - V[cj, c]
        assert np.array_equal(G[:, c], (cw * d) * d)
    # the same x on a fresh MAC: the first solve of a handle either way, so the same bits
    lams2, V2, info = MAC(fixed, cand, int(g["n"])).lowest_pairs(g["x"], 4)
    assert np.array_equal(lams, lams2) and np.array_equal(V, V2)
    # ... and on the handle that has solved before (its column-0 solve may take another mode): both obey the stop rule
    lams3, _, _ = mac.lowest_pairs(g["x"], 4)
    assert np.abs(lams - lams3).max() <= 2 * TOL * R.lnorm_inf(CASES["er300_x0"][1])
    f, grad = mac.problem(g["x"])
    assert info["reordered"] == 0 and abs(f - lams[0]) <= TOL * R.lnorm_inf(CASES["er300_x0"][1])
    assert np.array_equal(mac._dev.gradient_block(V[:, :1])[:, 0], G[:, 0])      # (the handle's scratch, reused)


def test_refusals():
    gs = R.small_graphs()
    P = problem_of(*gs["petersen"])
    try:
        for q in (0, 10, 17):
            with pytest.raises(AssertionError, match="BAD_ARG"):
                P.lowest_pairs(q=q, X0=None)
    finally:
        P.close()
    # two components: as machip_fiedler answers
    i = np.array([0, 1, 2, 4, 5, 6]); j = np.array([1, 2, 3, 5, 6, 7])
    with pytest.raises(_lib.Disconnected):
        find_lowest_pairs(R.laplacian(8, i, j, np.ones(6)), q=2)
    # a step cap that cannot be met: said per column, raised only on request
    L = CASES["p300"][1]
    lams, V, info = find_lowest_pairs(L, q=4, max_steps=8)
    bad = info["status"] == _lib.NOT_CONVERGED
    assert bad.any() and np.all(info["residual"][bad] >= TOL) and np.all(info["status"][~bad] == _lib.OK)
    with pytest.raises(_lib.NotConverged):
        find_lowest_pairs(L, q=4, max_steps=8, raise_on_cap=True)
