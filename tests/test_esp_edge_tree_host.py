"""The edge-space relaxation over a spanning tree without a GPU: its NumPy restatement (tests/esp_edge_tree_restatement.py) against
the node-space one (tests/esp_relax_restatement.py, any fixed graph), the flag's rules, the public surface, the new entry point's
presence, and the teacher-forcing input of the device test.

Tolerances are those of tests/test_esp_edge_host.py: F within esp_relax_restatement.F_tolerance (10 max(d, 1e-13 |logdet M(x)|), d
the disagreement of two CPU routes for logdet M(x)), the gradient within 1e-10 of its largest entry."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import esp_edge_restatement as E
import esp_edge_tree_restatement as T
import esp_relax_restatement as X
from mac_amd import _lib

GRAD_RTOL = 1e-10

GRAPHS = dict(intel_fixed50=T.intel_fixed50, tree40=T.tree40, star=T.star, awkward12=T.awkward12)


def x_of(kind, m):
    if kind == "zero":
        return np.zeros(m)
    if kind == "uniform":
        return np.random.default_rng(17).random(m)
    if kind == "vertex":
        return E.vertex_x(m)
    return E.wild_x(m)


# ---- 1. the restatement against the node restatement ----
@pytest.mark.parametrize("kind", ["zero", "uniform", "vertex", "wild"])
@pytest.mark.parametrize("case", list(GRAPHS))
def test_tree_restatement_agrees_with_the_node_restatement(case, kind):
    g = GRAPHS[case]()
    m = len(g[6])
    x = x_of(kind, m)
    plan = T.plan_of(g)
    G = T.G_of(g, plan)
    tol, d, _ = X.F_tolerance(g, x)
    Fe, Fn = T.objective(g, x, G, plan), X.objective(g, x)
    print(f"{case} {kind}: F_tree={Fe:.15g} F_node={Fn:.15g} |diff|={abs(Fe - Fn):.3e} tol={tol:.3e} d={d:.3e}")
    assert abs(Fe - Fn) <= tol
    if kind == "zero":
        assert Fe == 0.0
    ge, gn = T.gradient(g, x, G, plan), X.gradient(g, x)
    err, top = float(np.max(np.abs(ge - gn))), float(np.max(np.abs(gn)))
    print(f"{case} {kind}: max|grad diff|={err:.3e} max g={top:.6g} rel={err / top:.3e}")
    assert err <= GRAD_RTOL * top


def test_graphs_have_the_inputs_they_are_there_for():
    g = T.intel_fixed50()
    assert g[0] == 1728 and len(g[6]) == 735 and len(T.plan_of(g)["seeds"][2]) == 50
    g = T.tree40()
    assert g[0] == 40 and len(g[3]) == 39 + 6 and len(T.plan_of(g)["seeds"][2]) == 6
    assert len(T.plan_of(T.star())["seeds"][2]) == 0
    n, fi, fj, fw, ci, cj, cw = g = T.awkward12()
    plan = T.plan_of(g)
    su, sv, sw = plan["seeds"]
    links = [(min(a, b), max(a, b)) for a, b in zip(fi.tolist(), fj.tolist())]
    assert n == 12 and links.count((4, 5)) == 2 and links.count((1, 11)) == 2 and any(a > b for a, b in zip(fi, fj))
    assert len(sw) == 4 and len(set(links)) == (n - 1) + len(sw)
    pairs = list(zip(ci.tolist(), cj.tolist()))
    assert pairs.count((5, 2)) == 2 and pairs.count((2, 5)) == 2 and any(0 in p for p in pairs) and pairs.count((6, 6)) == 1
    seeds = {(min(a, b), max(a, b)) for a, b in zip(su.tolist(), sv.tolist())}
    tree = {(min(v, int(p)), max(v, int(p))) for v, p in enumerate(plan["parent"]) if p >= 0}
    assert any((min(p), max(p)) in tree for p in pairs) and any((min(p), max(p)) in seeds for p in pairs)


def test_gram_matrix_is_bit_symmetric_and_a_self_loop_is_exactly_zero():
    g = T.awkward12()
    plan = T.plan_of(g)
    G = T.G_of(g, plan)
    m, r = len(g[6]), len(plan["seeds"][2])
    assert G.shape == (m + r, m + r) and np.array_equal(G, G.T)
    loop = [a == b for a, b in zip(g[4], g[5])].index(True)
    assert not G[loop].any() and not G[:, loop].any() and T.gradient(g, np.full(m, 0.5), G, plan)[loop] == 0.0
    assert np.array_equal(G[0], G[2]) and np.array_equal(G[0], -G[1])          # (5, 2) twice; (2, 5) is the same column reversed


def test_lowest_common_ancestors_by_bisection_equal_the_plain_walk():
    for g in (T.awkward12(), T.tree40(), T.star()):
        plan = T.plan_of(g)
        nodes = np.arange(g[0])
        L = T.lca_pairs(plan["parent"], nodes)
        for a in nodes:
            for b in nodes:
                assert L[a, b] == T.lca_walk(plan["parent"], a, b)


# ---- 2. flag, ValueError, header and export rules ----
def test_header_declares_and_library_exports_relax_gram():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert re.search(r"#define\s+MACHIP_ESP_EDGE_RELAX_TREE\s+32\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+machip_esp_relax_gram\s*\(\s*machip_esp\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)", hdr)
    lib = _lib.load()
    assert hasattr(lib, "machip_esp_relax_gram") and "machip_esp_relax_gram" in _lib.SIGNATURES
    out = np.zeros(1)
    assert lib.machip_esp_relax_gram(None, _lib.p_f64(out), 1) == _lib.BAD_ARG and "NULL" in _lib.last_error()
    assert hasattr(_lib.Esp, "relax_gram")


def test_flag_is_a_new_power_of_two_and_bit_4_stays_unknown():
    others = [_lib.ESP_DENSE_INVERSE, _lib.ESP_MATRIX_FREE, _lib.ESP_SPANNING_TREE, _lib.ESP_EDGE_RELAX]
    f = _lib.ESP_EDGE_RELAX_TREE
    assert others == [1, 2, 8, 16] and f == 32 and f & (f - 1) == 0 and f not in others
    assert 4 not in others + [f]


def test_edge_relax_and_edge_space_stay_keyword_only_and_off_by_default():
    from mac_amd.solvers import ESPRelaxation
    for fn, name in ((_lib.Esp.__init__, "edge_relax"), (ESPRelaxation.__init__, "edge_space")):
        p = inspect.signature(fn).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_value_errors_come_before_a_device_is_asked_for(monkeypatch):
    from mac_amd.solvers import ESPRelaxation
    from mac_amd.utils.graphs import Edge

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_device", no_device)
    args = (3, [0, 1], [1, 2], [1.0, 1.0], [0], [2], [1.0])
    for kw in (dict(), dict(matrix_free=False), dict(matrix_free=True), dict(matrix_free="tree", dense_inverse=True),
               dict(matrix_free=True, dense_inverse=True)):
        with pytest.raises(ValueError, match="edge_relax"):
            _lib.Esp(*args, edge_relax="tree", **kw)
    with pytest.raises(ValueError, match="edge_relax"):
        _lib.Esp(*args, matrix_free="tree", edge_relax="chain")
    with pytest.raises(ValueError, match="edge_relax"):               # edge_relax=True keeps its rules
        _lib.Esp(*args, matrix_free="tree", edge_relax=True)
    with pytest.raises(ValueError, match="edge_space"):
        ESPRelaxation([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3, edge_space="chain")
    # the well-formed pairing gets as far as the device
    with pytest.raises(AssertionError, match="the device was asked for"):
        _lib.Esp(*args, matrix_free="tree", edge_relax="tree")
    with pytest.raises(AssertionError, match="the device was asked for"):
        ESPRelaxation([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3, edge_space="tree")


def test_create_decides_the_flag_errors_before_a_device_is_needed():
    lib = _lib.load()
    i32, f64, p_i32, p_f64 = _lib.i32, _lib.f64, _lib.p_i32, _lib.p_f64

    def create(flags, fixed=([0, 1, 1], [1, 2, 3], [1.0, 1.0, 1.0]), n=4):
        fi, fj, fw = i32(fixed[0]), i32(fixed[1]), f64(fixed[2])
        ci, cj, cw = i32([0]), i32([3]), f64([1.0])
        h = C.c_void_p()
        st = lib.machip_esp_create(0, n, len(fw), p_i32(fi), p_i32(fj), p_f64(fw), 1, p_i32(ci), p_i32(cj), p_f64(cw), 0, flags, C.byref(h))
        msg = _lib.last_error()
        if st == _lib.OK:
            lib.machip_esp_destroy(h)
        else:
            assert not h.value
        return st, msg

    TREE, FREE, SPAN, EDGE, DENSE = _lib.ESP_EDGE_RELAX_TREE, _lib.ESP_MATRIX_FREE, _lib.ESP_SPANNING_TREE, _lib.ESP_EDGE_RELAX, _lib.ESP_DENSE_INVERSE
    for flags in (TREE, TREE | FREE, TREE | SPAN):
        st, msg = create(flags)
        assert st == _lib.BAD_ARG and msg.startswith("unknown flags") and "MACHIP_ESP_EDGE_RELAX_TREE" in msg, (flags, msg)
    st, msg = create(TREE | FREE | SPAN | EDGE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX_TREE" in msg and re.search(r"MACHIP_ESP_EDGE_RELAX\b(?!_TREE)", msg), msg
    st, msg = create(TREE | FREE | SPAN | DENSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX_TREE" in msg and "MACHIP_ESP_DENSE_INVERSE" in msg, msg
    st, msg = create(TREE | FREE | SPAN | 4)
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    st, msg = create(TREE | FREE | SPAN | 64)
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    # the answers that were there before stay
    st, msg = create(FREE | SPAN | EDGE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "MACHIP_ESP_SPANNING_TREE" in msg and "EDGE_RELAX_TREE" not in msg
    # a fixed graph that is not connected is still the spanning-tree route's refusal
    st, msg = create(TREE | FREE | SPAN, fixed=([0, 2], [1, 3], [1.0, 1.0]))
    assert st == _lib.BAD_ARG and "connected" in msg
    # a well-formed request gets past the argument checks: without a device the answer is NO_DEVICE, not BAD_ARG
    st, msg = create(TREE | FREE | SPAN)
    assert st == (_lib.OK if _lib.device_count() > 0 else _lib.NO_DEVICE), msg


# ---- 3. the teacher-forcing input of the device test ----
def test_teacher_forcing_input_keeps_its_lp_margins():
    """The 20 restated iterates of intel with 50 closures fixed at K = 50 %: at every iterate the K-th and (K+1)-th gradient values are
    at least 1e-7 of the largest entry apart -- 1 000 x the gradient tolerance -- so a device gradient within that tolerance has the
    restatement's LP vertex.  (Smallest margin over the 20 iterates: 5.86e-6.)"""
    g = T.intel_fixed50()
    k, run = T.teacher_run()
    assert k == int(0.5 * len(g[6])) and len(run["iterates"]) == 20
    print("restated margins:", " ".join(f"{v:.2e}" for v in run["margin"]))
    assert min(run["margin"]) >= 1e-7 and np.isclose(1e-7, 1000 * GRAD_RTOL)
    for x, s in zip(run["iterates"], run["vertex"]):
        assert x.min() >= 0.0 and x.max() <= 1.0 and s.sum() == k
    # the node restatement sees the same function at these iterates (first, a middle one and the last)
    for t in (0, 9, 19):
        x = run["iterates"][t]
        tol, d, _ = X.F_tolerance(g, x)
        assert abs(run["F"][t] - X.objective(g, x)) <= tol
        gn = X.gradient(g, x)
        assert np.max(np.abs(run["grad"][t] - gn)) <= GRAD_RTOL * np.max(np.abs(gn))
        assert np.array_equal(run["vertex"][t], X.lp_vertex(gn, k))
