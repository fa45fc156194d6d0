"""The relaxation of GreedyESP's problem without a GPU: the NumPy restatement (tests/esp_relax_restatement.py) against itself
and against the greedy's restatement, the public surface, the C entry points' presence and the argument errors that need no
device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
import esp_relax_restatement as X
import esp_restatement as R
from mac_amd import _lib


def arrays(g):
    return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
            np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))


def graph(case):
    if case == "petersen":
        return X.petersen()
    if case == "er300":
        return X.chain_er(300, 0.03, 0)
    return arrays(load_golden("g2o_intel"))


CASES = ["petersen", "er300", "intel"]


def test_esp_relaxation_is_exported_from_mac_amd_and_mac_solvers():
    import mac_amd.solvers
    from mac_amd.solvers import ESPRelaxation
    assert "ESPRelaxation" in mac_amd.solvers.__all__ and ESPRelaxation.__module__ == "mac_amd.solvers.esp_relax"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from mac.solvers import ESPRelaxation\nfrom mac.solvers.esp_relax import ESPRelaxation as E2\nimport mac_amd.solvers\n"
            "assert ESPRelaxation is E2 is mac_amd.solvers.ESPRelaxation\nprint('ok')" % (ROOT, os.path.join(ROOT, "compat")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp", timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-1500:]


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("machip_esp_relax_eval", "machip_esp_relax_run", "machip_esp_relax_inner"):
        assert re.search(r"\bint\s+%s\s*\(\s*machip_esp\s*\*" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.Esp, "relax_eval") and hasattr(_lib.Esp, "relax_run")


def test_entry_points_reject_a_null_handle_and_null_outputs_without_a_device():
    lib = _lib.load()
    F = C.c_double()
    assert lib.machip_esp_relax_eval(None, None, C.byref(F), None) == _lib.BAD_ARG
    assert "NULL" in _lib.last_error()
    it, up = C.c_int(), C.c_double()
    assert lib.machip_esp_relax_run(None, 3, 5, 1e-4, 1e-8, None, None, None, None, C.byref(it), C.byref(up)) == _lib.BAD_ARG
    assert "NULL" in _lib.last_error()
    assert lib.machip_esp_relax_inner(None, None, None, C.byref(up)) == _lib.BAD_ARG


def test_frank_wolfe_driver_forms_the_dual_value_through_inner_when_given():
    from mac_amd.optimization.frankwolfe import frank_wolfe
    A = np.diag([1.0, 2.0, 3.0, 4.0])
    prob = lambda x: (float(-0.5 * x @ A @ x + x.sum()), -A @ x + 1.0)         # concave
    lp = lambda g: X.lp_vertex(g, 2)
    calls = []

    def inner(a, b):
        calls.append((a.copy(), b.copy()))
        return float(a @ b)
    x0 = np.array([1.0, 1.0, 0.0, 0.0])
    x1, u1 = frank_wolfe(x0, prob, lp, maxiter=7)
    x2, u2 = frank_wolfe(x0, prob, lp, maxiter=7, inner=inner)
    assert np.array_equal(x1, x2) and u1 == u2 and len(calls) == 7
    x3, u3 = frank_wolfe(x0, prob, lp, maxiter=7, inner=lambda a, b: float(a @ b) + 1.0)
    assert np.array_equal(x1, x3) and abs(u3 - (u1 + 1.0)) < 1e-12


def test_construction_without_a_device_raises_machip_error(monkeypatch):
    from mac_amd.solvers import ESPRelaxation
    from mac_amd.utils.graphs import Edge
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.MachipError) as ei:
        ESPRelaxation([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3)
    assert ei.value.status == _lib.NO_DEVICE


@pytest.mark.parametrize("case", CASES)
def test_objective_of_a_selection_is_the_logdet_growth_and_the_sum_of_the_greedy_gains(case):
    g = graph(case)
    m = len(g[6])
    k = max(1, m // 3)
    order, gains, _ = R.greedy(*g, k)
    x = np.zeros(m); x[order] = 1.0
    F = X.objective(g, x)
    sparse_growth = R.logdet_sparse(X.M_of(g, x, sparse=True)) - R.logdet_sparse(X.M_of(g, np.zeros(m), sparse=True))
    tol = X.F_tolerance(g, x)[0]
    assert abs(F - sparse_growth) <= tol
    assert abs(F - np.sum(np.log1p(gains))) <= tol + 1e-9 * abs(F)          # (the gains carry the greedy's own 1e-9)
    assert X.objective(g, np.zeros(m)) == 0.0


@pytest.mark.parametrize("case", CASES)
def test_gradient_is_the_score_of_the_inverse_and_the_slope_of_the_objective(case):
    g = graph(case)
    rng = np.random.default_rng(11)
    m = len(g[6])
    x = rng.random(m)
    gr = X.gradient(g, x)
    ref = R.scores(np.linalg.inv(X.M_of(g, x)), g[4], g[5], g[6])
    assert np.max(np.abs(gr - ref)) <= 1e-10 * np.max(ref)
    d = rng.standard_normal(m)
    h = 1e-6
    xp, xm = np.clip(x + h * d, 0, None), np.clip(x - h * d, 0, None)
    slope = X.objective(g, xp) - X.objective(g, xm)
    assert abs(slope - gr @ (xp - xm)) <= 1e-5 * abs(gr @ (xp - xm)) + 1e-9


def test_lp_vertex_takes_ties_by_lowest_index():
    s = X.lp_vertex(np.array([1.0, 3.0, 2.0, 3.0, 2.0, 2.0]), 3)
    assert np.array_equal(s, [0, 1, 1, 1, 0, 0])
    assert X.lp_margin(np.array([1.0, 3.0, 2.0, 3.0, 2.0, 2.0]), 3) == 0.0
    assert X.lp_margin(np.array([4.0, 3.0, 1.0]), 2) == 0.5


@pytest.mark.parametrize("case", CASES)
def test_dual_bound_of_every_iterate_dominates_the_greedy_and_random_selections(case):
    g = graph(case)
    m = len(g[6])
    k = max(1, m // 2)
    x0 = np.zeros(m); x0[np.argsort(-g[6], kind="stable")[:k]] = 1.0
    run = X.frank_wolfe(g, k, x0, max_iters=8 if case == "intel" else 20)
    order, _, _ = R.greedy(*g, k)
    x = np.zeros(m); x[order] = 1.0
    values = [X.objective(g, x)]
    rng = np.random.default_rng(5)
    for _ in range(50):
        x = np.zeros(m); x[rng.choice(m, k, replace=False)] = 1.0
        values.append(X.objective(g, x))
    best = max(values)
    assert min(run["dual"]) >= best - 1e-9 * abs(best)
    assert run["upper"] == min(run["dual"])
    assert all(0.0 <= v <= 1.0 for v in run["x"]) and run["x"].sum() <= k * (1 + 1e-12)
