"""GreedyKirchhoff without a GPU: the NumPy restatement (tests/kirchhoff_restatement.py) against brute-force pseudo-inverses, the
public surface, the C entry points' presence and the argument errors that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import kirchhoff_restatement as KR
from mac_amd import _lib

ENTRY_POINTS = ("machip_esp_kirchhoff_select", "machip_esp_kirchhoff_gains", "machip_esp_kirchhoff_eval")


def chain_er(n, p, seed):
    """tests/test_esp_gpu.py's generator: links (i, i+1) and ER candidates off the chain, weights uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < p
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


@pytest.mark.parametrize("n,p,seed,K", [(40, 0.1, 1, 20), (100, 0.05, 3, 40), (130, 0.03, 5, 60)])
def test_restatement_gains_equal_the_brute_force_drops_of_the_trace(n, p, seed, K):
    g = chain_er(n, p, seed)
    _, fi, fj, fw, ci, cj, cw = g
    assert len(cw) >= K
    order, gains, margins, drift = KR.greedy(*g, K)
    edges = list(zip(fi, fj, fw))
    before = KR.exact_trace(n, edges)
    first = before
    for k, e in enumerate(order):
        edges.append((ci[e], cj[e], cw[e]))
        after = KR.exact_trace(n, edges)
        assert abs(gains[k] - (before - after)) <= 1e-8 * (before - after), (k, gains[k], before - after)
        before = after
    assert abs(gains.sum() - (first - before)) <= 1e-8 * first
    assert margins.min() >= 1e-6 and drift < 1e-8
    o2, g2, _, _ = KR.greedy(*g, K, fold=7)              # the fold structure changes rounding, not the run
    assert np.array_equal(order, o2) and np.allclose(gains, g2, rtol=1e-9, atol=0)
    assert len(set(order.tolist())) == K


def test_restatement_trace_formula_and_a_greedy_step_by_exhaustion():
    g = chain_er(40, 0.1, 1)
    n, fi, fj, fw, ci, cj, cw = g
    Sig, _ = KR.R.initial_sigma(n, fi, fj, fw)
    base = KR.exact_trace(n, zip(fi, fj, fw))
    assert abs(KR.trace_of(Sig, n) - base) <= 1e-10 * base
    drops = np.array([base - KR.exact_trace(n, list(zip(fi, fj, fw)) + [(ci[e], cj[e], cw[e])]) for e in range(len(cw))])
    gains = KR.exact_scores(Sig, n, ci, cj, cw)[3]
    assert np.allclose(gains, drops, rtol=1e-8, atol=0)
    order, _, _, _ = KR.greedy(*g, 1)
    assert order[0] == int(np.argmax(drops))


def test_greedy_kirchhoff_is_exported_from_mac_amd_and_mac_solvers():
    import mac_amd.solvers
    from mac_amd.solvers import GreedyKirchhoff
    assert "GreedyKirchhoff" in mac_amd.solvers.__all__ and GreedyKirchhoff.__module__ == "mac_amd.solvers.kirchhoff"
    for name in ("subset", "subsets", "gains", "kirchhoff_index", "info"):
        assert callable(getattr(GreedyKirchhoff, name))
    assert not hasattr(GreedyKirchhoff, "subset_lazy") and not hasattr(GreedyKirchhoff, "subsets_lazy")      # not submodular: no lazy variant
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from mac.solvers import GreedyKirchhoff\nfrom mac.solvers.kirchhoff import GreedyKirchhoff as G2\nimport mac_amd.solvers\n"
            "assert GreedyKirchhoff is G2 is mac_amd.solvers.GreedyKirchhoff\nprint('ok')" % (ROOT, os.path.join(ROOT, "compat")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp", timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-1500:]


def test_header_declares_library_exports_and_binding_lists_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 21
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.machip_version() >= 21
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*machip_esp\s*\*" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["machip_esp_kirchhoff_select"] == _lib.SIGNATURES["machip_esp_select"]      # the same shapes
    for name in ("kirchhoff_select", "kirchhoff_gains", "kirchhoff_eval"):
        assert callable(getattr(_lib.Esp, name))


def test_entry_points_reject_a_null_handle_and_null_outputs_without_a_device():
    lib = _lib.load()
    ks = (C.c_int64 * 1)(3)
    order, gain, t = np.zeros(3, dtype=np.int32), np.zeros(3), np.zeros(1)
    assert lib.machip_esp_kirchhoff_select(None, 1, ks, _lib.p_i32(order), _lib.p_f64(gain), _lib.p_f64(t)) == _lib.BAD_ARG
    assert "NULL handle" in _lib.last_error()
    assert lib.machip_esp_kirchhoff_gains(None, _lib.p_f64(gain)) == _lib.BAD_ARG
    assert "NULL handle" in _lib.last_error()
    out2 = np.zeros(2)
    assert lib.machip_esp_kirchhoff_eval(None, 0, None, _lib.p_f64(out2)) == _lib.BAD_ARG
    assert "NULL handle" in _lib.last_error()
