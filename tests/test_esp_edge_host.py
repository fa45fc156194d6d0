"""The edge-space relaxation without a GPU: its NumPy restatement (tests/esp_edge_restatement.py) against the node-space one
(tests/esp_relax_restatement.py), the public surface, the new entry point's presence and the argument errors that need no device.

Tolerances are those of the node form's tests: F within esp_relax_restatement.F_tolerance (10 max(d, 1e-13 |logdet M(x)|), d the
disagreement of two CPU routes for logdet M(x)), the gradient within 1e-10 of its largest entry."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
import esp_edge_restatement as E
import esp_relax_restatement as X
from mac_amd import _lib

GRAD_RTOL = 1e-10


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def graph(case):
    if case == "er40":
        return X.chain_er(40, 0.1, 3)
    if case == "awkward12":
        return E.awkward12()
    return arrays(load_golden("g2o_" + case))


def x_of(kind, m):
    if kind == "zero":
        return np.zeros(m)
    if kind == "uniform":
        return np.random.default_rng(17).random(m)        # seeded uniform in [0, 1)
    if kind == "vertex":
        return E.vertex_x(m)                              # m // 3 ones at seeded random places
    return E.wild_x(m)                                    # 30 % exact zeros, the rest 10^U(-14, 0), seed 29


@pytest.mark.parametrize("kind", ["zero", "uniform", "vertex", "wild"])
@pytest.mark.parametrize("case", ["er40", "awkward12", "intel", "kitti_05"])
def test_edge_restatement_agrees_with_the_node_restatement(case, kind):
    g = graph(case)
    m = len(g[6])
    x = x_of(kind, m)
    tol, d, _ = X.F_tolerance(g, x)
    Fe, Fn = E.objective(g, x), X.objective(g, x)
    print(f"{case} {kind}: F_edge={Fe:.15g} F_node={Fn:.15g} |diff|={abs(Fe - Fn):.3e} tol={tol:.3e} d={d:.3e}")
    assert abs(Fe - Fn) <= tol
    if kind == "zero":
        assert Fe == 0.0
    ge, gn = E.gradient(g, x), X.gradient(g, x)
    err, top = float(np.max(np.abs(ge - gn))), float(np.max(np.abs(gn)))
    print(f"{case} {kind}: max|grad diff|={err:.3e} max g={top:.6g} rel={err / top:.3e}")
    assert err <= GRAD_RTOL * top


def test_awkward_chain_has_the_inputs_it_is_there_for():
    n, fi, fj, fw, ci, cj, cw = E.awkward12()
    assert n == 12
    hops = sorted(zip(np.minimum(fi, fj).tolist(), np.maximum(fi, fj).tolist()))
    assert hops.count((4, 5)) == 2 and any(a > b for a, b in zip(fi, fj))               # parallel links, a reversed link
    pairs = list(zip(ci.tolist(), cj.tolist()))
    assert pairs.count((5, 2)) == 2 and pairs.count((2, 5)) == 2
    assert any(0 in p for p in pairs) and any(a == b for a, b in pairs)
    G = E.G_of((n, fi, fj, fw, ci, cj, cw))
    assert np.array_equal(G, G.T)
    loop = [a == b for a, b in pairs].index(True)
    assert not G[loop].any() and E.gradient((n, fi, fj, fw, ci, cj, cw), np.full(len(cw), 0.5))[loop] == 0.0
    assert np.array_equal(G[0], G[1]) and np.array_equal(G[0], G[2])                    # (5, 2) and (2, 5) are one interval


def test_restatement_refuses_a_fixed_graph_that_is_not_the_chain():
    with pytest.raises(AssertionError):
        E.G_of(X.petersen())
    with pytest.raises(AssertionError):
        E.G_of(X.disconnected())


def test_header_declares_and_library_exports_relax_info():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert re.search(r"#define\s+MACHIP_ESP_EDGE_RELAX\s+16\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+machip_esp_relax_info\s*\(\s*machip_esp\s*\*\s*\w+\s*,\s*int32_t\s*\*", hdr)
    lib = _lib.load()
    assert hasattr(lib, "machip_esp_relax_info") and "machip_esp_relax_info" in _lib.SIGNATURES
    a = np.zeros(2, dtype=np.int32)
    assert lib.machip_esp_relax_info(None, _lib.p_i32(a)) == _lib.BAD_ARG and "NULL" in _lib.last_error()
    assert hasattr(_lib.Esp, "relax_info")


def test_flag_does_not_collide_with_the_other_three():
    flags = [_lib.ESP_DENSE_INVERSE, _lib.ESP_MATRIX_FREE, _lib.ESP_SPANNING_TREE, _lib.ESP_EDGE_RELAX]
    assert _lib.ESP_EDGE_RELAX == 16 and all(f > 0 and f & (f - 1) == 0 for f in flags) and len(set(flags)) == 4
    assert 4 not in flags                                  # (bit 4 stays an unknown flag)


def test_edge_relax_and_edge_space_are_keyword_only_and_off_by_default():
    from mac_amd.solvers import ESPRelaxation
    for f, name in ((_lib.Esp.__init__, "edge_relax"), (ESPRelaxation.__init__, "edge_space")):
        p = inspect.signature(f).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_esp_raises_value_error_for_combinations_without_a_meaning_before_a_device_is_asked_for(monkeypatch):
    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_device", no_device)
    args = (3, [0, 1], [1, 2], [1.0, 1.0], [0], [2], [1.0])
    for kw in (dict(), dict(matrix_free=False), dict(matrix_free="tree"), dict(matrix_free=True, dense_inverse=True)):
        with pytest.raises(ValueError, match="edge_relax"):
            _lib.Esp(*args, edge_relax=True, **kw)


def test_create_decides_the_flag_errors_before_a_device_is_needed():
    lib = _lib.load()
    i32, f64, p_i32, p_f64 = _lib.i32, _lib.f64, _lib.p_i32, _lib.p_f64

    def create(fi, fj, fw, flags, n=4):
        fi, fj, fw = i32(fi), i32(fj), f64(fw)
        ci, cj, cw = i32([0]), i32([3]), f64([1.0])
        h = C.c_void_p()
        st = lib.machip_esp_create(0, n, len(fw), p_i32(fi), p_i32(fj), p_f64(fw), 1, p_i32(ci), p_i32(cj), p_f64(cw), 0, flags, C.byref(h))
        msg = _lib.last_error()
        if st == _lib.OK:
            lib.machip_esp_destroy(h)
        else:
            assert not h.value
        return st, msg

    chain = ([0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0])
    star = ([0, 1, 1], [1, 2, 3], [1.0, 1.0, 1.0])
    EDGE, FREE = _lib.ESP_EDGE_RELAX, _lib.ESP_MATRIX_FREE
    st, msg = create(*chain, EDGE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "only together with MACHIP_ESP_MATRIX_FREE" in msg
    st, msg = create(*chain, EDGE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg
    st, msg = create(*chain, EDGE | FREE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "MACHIP_ESP_DENSE_INVERSE" in msg
    st, msg = create(*chain, EDGE | FREE | _lib.ESP_SPANNING_TREE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_EDGE_RELAX" in msg and "MACHIP_ESP_SPANNING_TREE" in msg
    st, msg = create(*star, EDGE | FREE)
    assert st == _lib.BAD_ARG and "needs a chain" in msg and "MACHIP_ESP_EDGE_RELAX" in msg
    st, msg = create(*chain, EDGE | FREE | 4)
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    # a well-formed request gets past the argument checks: without a device the answer is NO_DEVICE, not BAD_ARG
    st, msg = create(*chain, EDGE | FREE)
    assert st == (_lib.OK if _lib.device_count() > 0 else _lib.NO_DEVICE), msg
