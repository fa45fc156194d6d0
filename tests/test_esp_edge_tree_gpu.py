"""The edge-space relaxation over a spanning tree on the GPU (mac_amd/csrc/esp_relax_edge_tree.h; ``ESPRelaxation(edge_space="tree")``,
a handle made with ``matrix_free="tree", edge_relax="tree"``): its stored Gram matrix against the NumPy restatement
(tests/esp_edge_tree_restatement.py) bit for bit, F and the gradient against the node form on the device and, beyond that form's
limit, against sparse solves; the chain as input against the chain form; teacher forcing on restated iterates; the bound; repeatability;
the greedy's state; the refusals.

Tolerances are those of tests/test_esp_edge_gpu.py.  F: 10 max(d, 1e-13 |logdet M(x)|) with d the disagreement of two CPU routes for
the same quantity, computed per graph and x (esp_relax_restatement.F_tolerance; beyond the node limit d is the disagreement of the
sparse route and the restatement).  Gradient: 1e-10 of its largest entry.  The Gram matrix: 0 -- the device adds, adds and
subtracts four host-computed resistances in a stated association, and NumPy does the same.  Every figure is printed before it is
asserted (run with -s to see them).

Shapes: 3 000 nodes, 611 candidates (odd) and 40 seeds give M = 651 columns -- no multiple of 64 (ld = 704), and more than 512, so
a row loop of 256 lanes x double2 runs twice; a spine of 2 500 nodes gives a lifting table of 12 levels, a random recursive tree
one of 4; candidate 0 of every random graph touches node 0.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from conftest import load_golden
import esp_edge_restatement as E
import esp_edge_tree_restatement as T
import esp_relax_restatement as X
import esp_restatement as R
from mac_amd import _lib
from mac_amd.optimization.frankwolfe import frank_wolfe
from mac_amd.solvers import ESPRelaxation, GreedyESP
from mac_amd.utils.graphs import Edge

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-10


def edges(i, j, w):
    return [Edge(int(a), int(b), float(c)) for a, b, c in zip(i, j, w)]


@functools.lru_cache(maxsize=None)
def graph(case):
    if case == "deep":
        return T.random_tree(3000, 40, 611, 7, deep=2500)
    if case == "shallow":
        return T.random_tree(3000, 40, 611, 7)
    if case == "shallow_r0":
        return T.random_tree(3000, 0, 611, 9)
    if case == "awkward12":
        return T.awkward12()
    if case == "intel_fixed50":
        return T.intel_fixed50()
    if case == "big":
        return T.random_tree(20000, 40, 500, 8)
    g = load_golden("g2o_" + case)
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def relax_of(g, edge_space="tree"):
    n, fi, fj, fw, ci, cj, cw = g
    return ESPRelaxation(edges(fi, fj, fw), edges(ci, cj, cw), n, edge_space=edge_space)


def heaviest(g, k):
    x = np.zeros(len(g[6]))
    x[np.argsort(-g[6], kind="stable")[:k]] = 1.0
    return x


def x_of(kind, m):
    if kind == "zero":
        return np.zeros(m)
    if kind == "uniform":
        return np.random.default_rng(17).random(m)
    if kind == "vertex":
        return E.vertex_x(m)
    return E.wild_x(m)


def check_F(tag, F_dev, F_ref, tol, d):
    print(f"{tag}: F_dev={F_dev:.15g} F_ref={F_ref:.15g} |err|={abs(F_dev - F_ref):.3e} tol={tol:.3e} d={d:.3e}")
    assert abs(F_dev - F_ref) <= tol


def check_grad(tag, g_dev, g_ref):
    err, top = float(np.max(np.abs(g_dev - g_ref))), float(np.max(np.abs(g_ref)))
    print(f"{tag}: max|grad err|={err:.3e} max g={top:.6g} rel={err / top:.3e} tol={GRAD_RTOL:.0e}")
    assert err <= GRAD_RTOL * top


def depth_of(g):
    return int(T.root_paths(T.plan_of(g)["parent"], np.arange(g[0]))[1].max()) - 1


# ---- 1. the Gram matrix ----
@pytest.mark.parametrize("case,levels_min,levels_max", [("deep", 12, 12), ("shallow", 1, 6)])
def test_gram_matrix_equals_the_restatement_bit_for_bit(case, levels_min, levels_max):
    g = graph(case)
    plan = T.plan_of(g)
    m, r = len(g[6]), len(plan["seeds"][2])
    levels = max(1, depth_of(g).bit_length())
    print(f"{case}: m={m} r={r} depth={depth_of(g)} levels={levels}")
    assert (m, r) == (611, 40) and (m + r) % 64 and m + r > 512 and levels_min <= levels <= levels_max
    assert 0 in (int(g[4][0]), int(g[5][0]))
    dev = relax_of(g)._dev
    assert dev.relax_info() == dict(form="edge_tree", ld=704) and dev.info()["form"] == "tree_free" and dev.info()["seeds"] == r
    G = dev.relax_gram()
    ref = T.G_of(g, plan)
    assert G.shape == (m + r, m + r)
    print(f"{case}: entries that differ: {int(np.sum(G != ref))}, max |G|={np.max(np.abs(ref)):.6g}")
    assert np.array_equal(G, ref)
    assert np.array_equal(G, G.T)
    assert np.array_equal(dev.relax_gram(), G)                  # (kept, not rebuilt into something else)
    assert dev.relax_info() == dict(form="edge_tree", ld=704)


def test_gram_matrix_of_the_awkward_graph_has_its_exact_zeros():
    g = graph("awkward12")
    plan = T.plan_of(g)
    dev = relax_of(g)._dev
    G = dev.relax_gram()
    assert G.shape == (16, 16) and np.array_equal(G, T.G_of(g, plan)) and np.array_equal(G, G.T)
    loop = [a == b for a, b in zip(g[4], g[5])].index(True)
    assert not G[loop].any() and not G[:, loop].any()
    assert dev.relax_eval(np.full(len(g[6]), 0.5))[1][loop] == 0.0


# ---- 2. F and the gradient against the node form on the device ----
@functools.lru_cache(maxsize=None)
def pair_of(case):
    g = graph(case)
    return relax_of(g), relax_of(g, edge_space=False)


@pytest.mark.parametrize("kind", ["zero", "uniform", "vertex", "wild"])
@pytest.mark.parametrize("case", ["awkward12", "deep", "shallow", "shallow_r0"])
def test_value_and_gradient_agree_with_the_node_form_on_the_device(case, kind):
    g = graph(case)
    m = len(g[6])
    tree, node = pair_of(case)
    assert tree.info()["relax_form"] == "edge_tree" and node.info()["relax_form"] == "node"
    assert tree.info()["seeds"] == len(T.plan_of(g)["seeds"][2]) == (0 if case == "shallow_r0" else 4 if case == "awkward12" else 40)
    x = x_of(kind, m)
    Ft, gt = tree.problem(x)
    Fn, gn = node.problem(x)
    tol, d, _ = X.F_tolerance(g, x)
    check_F(f"{case} {kind} tree vs node on the device", Ft, Fn, tol, d)
    check_grad(f"{case} {kind} tree vs node on the device", gt, gn)
    assert tree.evaluate_objective(x) == Ft
    if kind == "zero":
        assert Ft == 0.0


# ---- 3. beyond the node form's limit ----
def test_beyond_the_node_forms_limit_matches_sparse_solves():
    from scipy.sparse.linalg import splu
    g = graph("big")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    plan = T.plan_of(g)
    assert n == 20000 and m == 500 and len(plan["seeds"][2]) == 40
    x = np.random.default_rng(43).random(m)
    Mx = X.M_of(g, x, sparse=True)
    ldx = R.logdet_sparse(Mx)
    F_sparse = ldx - R.logdet_sparse(X.M_of(g, np.zeros(m), sparse=True))
    Gr = T.G_of(g, plan)
    F_rest = T.objective(g, x, Gr, plan)
    d = abs(F_sparse - F_rest)
    tol = 10.0 * max(d, 1e-13 * abs(ldx))
    A = np.zeros((n, m))
    ar = np.arange(m)
    np.add.at(A, (ci, ar), 1.0)
    np.add.at(A, (cj, ar), -1.0)
    A = A[1:]
    g_sparse = cw * np.einsum("ij,ij->j", A, splu(Mx).solve(A))
    relax = relax_of(g)
    assert relax._dev.relax_info() == dict(form="edge_tree", ld=576)
    F, gr = relax.problem(x)
    print(f"tree20000: logdet M(x)={ldx:.15g}")
    check_F("tree20000 vs sparse LU", F, F_sparse, tol, d)
    check_F("tree20000 vs restatement", F, F_rest, tol, d)
    check_grad("tree20000 vs sparse solves", gr, g_sparse)
    check_grad("tree20000 vs restatement", gr, T.gradient(g, x, Gr, plan))
    assert relax.problem(np.zeros(m))[0] == 0.0
    assert np.array_equal(relax._dev.relax_gram(), Gr)
    # the node form refuses this graph: its fixed edges are no chain, so the dense handle itself is refused at n > 16384
    with pytest.raises(AssertionError, match="BAD_ARG.*num_nodes must be <= 16384"):
        relax_of(g, edge_space=False)
    with pytest.raises(AssertionError, match="BAD_ARG.*needs a chain"):
        relax_of(g, edge_space=True)                                     # (and the chain's edge form does not take it either)


# ---- 4. the chain as input ----
def test_chain_input_agrees_with_the_chain_form():
    g = graph("intel")
    m = len(g[6])
    tree, chain = relax_of(g), relax_of(g, edge_space=True)
    assert tree.info()["seeds"] == 0 and tree.info()["relax_form"] == "edge_tree" and chain.info()["relax_form"] == "edge"
    for kind in ("zero", "uniform", "vertex", "wild"):
        x = x_of(kind, m)
        Ft, gt = tree.problem(x)
        Fc, gc = chain.problem(x)
        tol, d, _ = X.F_tolerance(g, x)
        check_F(f"intel {kind} tree vs chain form", Ft, Fc, tol, d)
        check_grad(f"intel {kind} tree vs chain form", gt, gc)
    assert tree.info()["relax_ld"] == chain.info()["relax_ld"] == 832


# ---- 5. teacher forcing ----
def test_teacher_forcing_on_the_restated_iterates_every_vertex():
    g = graph("intel_fixed50")
    k, run = T.teacher_run()
    print("restated margins:", " ".join(f"{v:.2e}" for v in run["margin"]))
    assert len(run["iterates"]) == 20 and min(run["margin"]) >= 1e-7
    dev = relax_of(g)._dev
    for t in range(20):
        x, s = run["iterates"][t], run["vertex"][t]
        F, gr = dev.relax_eval(x)
        check_grad(f"iterate {t}", gr, run["grad"][t])
        one = dev.relax_run(k, x, max_iters=1, gap_tol=0.0, grad_tol=0.0)      # step 2 / (2 + 0) = 1: the iterate it returns is the vertex
        assert one["iters"] == 1 and one["f"][0] == F
        assert np.array_equal(one["x"] > 0.5, s > 0.5), f"iterate {t}"
        assert np.array_equal(X.lp_vertex(gr, k), s), f"iterate {t}"
    for t in (0, 19):
        tol, d, _ = X.F_tolerance(g, run["iterates"][t])
        check_F(f"iterate {t}", dev.relax_eval(run["iterates"][t], want_grad=False)[0], run["F"][t], tol, d)


# ---- 6. solve and the bound ----
def test_solve_bounds_the_tree_greedy_and_the_driver_reproduces_it():
    g = graph("intel_fixed50")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    k = m // 5
    x0 = heaviest(g, k)
    relax = relax_of(g)
    out = relax.solve(k, x0)
    assert isinstance(out, tuple) and len(out) == 3
    rounded, unrounded, upper = out
    greedy = GreedyESP(edges(fi, fj, fw), edges(ci, cj, cw), n, matrix_free="tree")
    gx, _ = greedy.subset(k)
    Fg, Fr = relax.evaluate_objective(gx), relax.evaluate_objective(rounded)
    tol, d, _ = X.F_tolerance(g, gx)
    gains = float(np.sum(np.log1p(greedy.last_gains)))
    print(f"K={k}: upper={upper:.15g} F(greedy)={Fg:.15g} sum log1p(gains)={gains:.15g} F(rounded)={Fr:.12g} iterations={len(relax.trace)}")
    assert gx.sum() == k and upper >= Fg and upper >= Fr and upper >= relax.evaluate_objective(x0)
    check_F("F(greedy) vs sum log1p(last_gains)", Fg, gains, tol, d)
    assert rounded.sum() == k and set(np.unique(rounded)) <= {0.0, 1.0}
    assert unrounded.min() >= 0.0 and unrounded.max() <= 1.0 and unrounded.sum() <= k * (1 + 1e-12)
    ups = [t[1] for t in relax.trace]
    assert all(a >= b for a, b in zip(ups, ups[1:])) and ups[-1] == upper
    x, u = frank_wolfe(x0, relax.problem, lambda gr: X.lp_vertex(gr, k), maxiter=20, relative_duality_gap_tol=1e-4, grad_norm_tol=1e-8,
                       inner=relax.inner)
    print(f"upper solve={upper!r} driver={float(u)!r}; max|x diff|={np.max(np.abs(x - unrounded)):.3e}")
    assert np.array_equal(x, unrounded) and u == upper
    info = relax.info()
    assert info["relax_form"] == "edge_tree" and info["seeds"] == 50 and info["relax_ld"] == 832 and info["iterations"] == len(relax.trace)


# ---- 7. repeatability ----
def test_two_solves_are_bit_identical():
    g = graph("intel_fixed50")
    k = len(g[6]) // 5
    x0 = heaviest(g, k)
    a, b = relax_of(g)._dev, relax_of(g)._dev
    r1 = a.relax_run(k, x0)
    r2 = a.relax_run(k, x0)
    r3 = b.relax_run(k, x0)
    assert r1["iters"] > 1
    for r in (r2, r3):
        assert r["iters"] == r1["iters"] and r["upper"] == r1["upper"] and np.array_equal(r["x"], r1["x"])
        for key in ("f", "dual", "gnorm"):
            assert np.array_equal(r[key], r1[key]), key


# ---- 8. the greedy is untouched ----
def test_relaxation_calls_leave_the_greedy_state_alone():
    g = graph("intel_fixed50")
    n, fi, fj, fw, ci, cj, cw = g
    m = len(cw)
    k = m // 4
    fresh = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free="tree")
    order0, gain0, _ = fresh.select([k])
    wr0 = fresh.weighted_resistances()
    # relaxation first, on a handle whose seeds have not been run
    dev = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free="tree", edge_relax="tree")
    dev.relax_eval(np.random.default_rng(1).random(m))
    order, gain, _ = dev.select([k])
    before = dev.weighted_resistances().copy()
    info = dev.info()
    assert info["pending"] == k and info["seeds"] == 50
    assert np.array_equal(order, order0) and np.array_equal(gain, gain0) and np.array_equal(before, wr0)
    dev.relax_eval(np.random.default_rng(2).random(m))
    dev.relax_run(k, heaviest(g, k), max_iters=3)
    dev.relax_gram()
    after = dev.weighted_resistances()
    assert np.array_equal(before, after) and dev.info() == info
    order2, gain2, _ = dev.select([k])
    assert np.array_equal(order2, order0) and np.array_equal(gain2, gain0)
    assert np.array_equal(dev.weighted_resistances(), wr0)


# ---- 9. refusals ----
def test_refusals():
    g = graph("big")
    n, fi, fj, fw = g[:4]
    rng = np.random.default_rng(7)
    # 400 more fixed links on the 20 000-node tree (with the 40 it has: some may repeat a link, so r is read from the handle)
    fi2 = np.concatenate([fi, rng.integers(0, n, 400)]); fj2 = np.concatenate([fj, rng.integers(0, n, 400)])
    fw2 = np.concatenate([fw, rng.uniform(0.5, 2.0, 400)])
    big_m = 16000
    big = _lib.Esp(n, fi2, fj2, fw2, rng.integers(0, n, big_m), rng.integers(0, n, big_m), rng.uniform(0.5, 2.0, big_m),
                   matrix_free="tree", edge_relax="tree")
    r = big.info()["seeds"]
    print(f"m = {big_m}, r = {r}")
    assert 385 <= r <= 440 and big_m + r > 16384
    for call in (lambda: big.relax_eval(np.zeros(big_m)), lambda: big.relax_run(5, np.zeros(big_m)),
                 lambda: big.relax_inner(np.zeros(big_m), np.zeros(big_m))):
        t0 = time.perf_counter()
        with pytest.raises(AssertionError, match=f"BAD_ARG.*MACHIP_ESP_EDGE_RELAX_TREE.*16384.*m = {big_m}, r = {r}"):
            call()
        dt = time.perf_counter() - t0
        print(f"m + r = {big_m + r}: refused in {dt * 1e3:.2f} ms")
        assert dt < 0.5                                                  # (a host check: no allocation, no launch)
    lib = _lib.load()
    assert lib.machip_esp_relax_gram(big._h, _lib.p_f64(np.zeros(1)), big_m + r) == _lib.BAD_ARG and "16384" in _lib.last_error()      # (refused before a byte is copied)
    order, gain, _ = big.select([3])                                     # the greedy of that handle keeps working
    assert len(set(order.tolist())) == 3
    big.close()
    # relax_gram on the other kinds of handle
    c = graph("intel")
    t = graph("awkward12")
    out = np.zeros((4, 4))
    for dev in (_lib.Esp(*c), _lib.Esp(*c, matrix_free=True, edge_relax=True), _lib.Esp(*t, matrix_free="tree"), _lib.Esp(*c, matrix_free=True)):
        with pytest.raises(AssertionError, match="BAD_ARG.*MACHIP_ESP_EDGE_RELAX_TREE"):
            dev.relax_gram()
        assert lib.machip_esp_relax_gram(dev._h, _lib.p_f64(out), 4) == _lib.BAD_ARG
    with pytest.raises(AssertionError, match="BAD_ARG"):                 # a plain tree handle still has no relaxation
        _lib.Esp(*t, matrix_free="tree").relax_eval(np.zeros(len(t[6])))
    ok = _lib.Esp(*t, matrix_free="tree", edge_relax="tree")
    assert lib.machip_esp_relax_gram(ok._h, _lib.p_f64(np.zeros((17, 17))), 17) == _lib.BAD_ARG and "m + r = 16" in _lib.last_error()
    assert lib.machip_esp_relax_gram(ok._h, None, 16) == _lib.BAD_ARG
    assert ok.relax_gram().shape == (16, 16)
    # the flag's combinations through the raw C call, on a machine that has a device: still decided on the host, no handle
    i32, f64, p_i32, p_f64 = _lib.i32, _lib.f64, _lib.p_i32, _lib.p_f64
    for flags, words in ((32, ("unknown flags", "MACHIP_ESP_EDGE_RELAX_TREE")), (32 | 2, ("unknown flags", "MACHIP_ESP_EDGE_RELAX_TREE")),
                         (32 | 2 | 8 | 16, ("MACHIP_ESP_EDGE_RELAX_TREE", "MACHIP_ESP_EDGE_RELAX ")),
                         (32 | 2 | 8 | 1, ("MACHIP_ESP_EDGE_RELAX_TREE", "MACHIP_ESP_DENSE_INVERSE")), (2 | 8 | 16, ("MACHIP_ESP_EDGE_RELAX ", "MACHIP_ESP_SPANNING_TREE"))):
        h = C.c_void_p()
        st = lib.machip_esp_create(0, t[0], len(t[3]), p_i32(i32(t[1])), p_i32(i32(t[2])), p_f64(f64(t[3])), len(t[6]), p_i32(i32(t[4])),
                                   p_i32(i32(t[5])), p_f64(f64(t[6])), 0, flags, C.byref(h))
        msg = _lib.last_error()
        assert st == _lib.BAD_ARG and not h.value and all(w in msg for w in words), (flags, msg)
