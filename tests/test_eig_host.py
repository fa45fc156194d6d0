"""GreedyEig without a GPU: the public surface, the C entry points, the helper methods against direct NumPy, and the NumPy
restatement of the rule (tests/eig_restatement.py) against itself: brute force vs the secular equation, bound >= value,
lambda_2 non-decreasing over the picks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import eig_restatement as R
from mac_amd import _lib


def chain_closures(n, p, seed):
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < p
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def test_greedy_eig_is_exported_and_both_compat_import_lines_work():
    import mac_amd.solvers
    from mac_amd.solvers import GreedyEig
    assert "GreedyEig" in mac_amd.solvers.__all__ and GreedyEig.__module__ == "mac_amd.solvers.greedy_eig"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from mac.solvers.greedy_eig import GreedyEig\nfrom mac.solvers import GreedyEig as G2\nimport mac_amd.solvers\n"
            "assert GreedyEig is G2 is mac_amd.solvers.GreedyEig\nprint('ok')" % (ROOT, os.path.join(ROOT, "compat")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp", timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-1500:]


def test_header_declares_and_library_exports_the_eig_entry_points():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 8
    lib = _lib.load()
    for name in ("machip_eig_create", "machip_eig_destroy", "machip_eig_select", "machip_eig_candidate_lambda2",
                 "machip_eig_candidate_bounds", "machip_eig_info"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_construction_without_a_device_raises_machip_error(monkeypatch):
    from mac_amd.solvers import GreedyEig
    from mac_amd.utils.graphs import Edge
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.MachipError) as ei:
        GreedyEig([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3)
    assert ei.value.status == _lib.NO_DEVICE


def _bare(n, fi, fj, fw, ci, cj, cw):
    """A GreedyEig with everything but the device handle (the helper methods are host code)."""
    from mac_amd.solvers import GreedyEig
    from mac_amd.utils.graphs import Edge, weight_graph_lap_from_edge_list
    g = GreedyEig.__new__(GreedyEig)
    g.L_odom = weight_graph_lap_from_edge_list([Edge(int(a), int(b), float(c)) for a, b, c in zip(fi, fj, fw)], n)
    g.num_poses = n
    g.weights = np.asarray(cw, dtype=np.float64)
    g.edge_list = np.stack([ci, cj], axis=1).astype(np.int64)
    return g


def test_grad_from_fiedler_and_combined_laplacian_match_direct_numpy():
    n, fi, fj, fw, ci, cj, cw = chain_closures(30, 0.1, 3)
    g = _bare(n, fi, fj, fw, ci, cj, cw)
    rng = np.random.default_rng(0)
    v = rng.normal(size=n)
    assert np.allclose(g.grad_from_fiedler(v), [w * (v[a] - v[b]) ** 2 for a, b, w in zip(ci, cj, cw)], rtol=1e-14, atol=0)
    x = rng.random(len(cw))
    x[::3] = 0.0
    x[1] = 5e-11                                        # below tol: dropped
    keep = x > 1e-10
    ref = R.laplacian(n, np.concatenate([fi, ci[keep]]), np.concatenate([fj, cj[keep]]), np.concatenate([fw, (x * cw)[keep]]))
    assert np.allclose(g.combined_laplacian(x).toarray(), ref, rtol=1e-14, atol=1e-15)


def test_restatement_brute_force_and_secular_agree():
    for seed in (0, 1):
        g = chain_closures(30, 0.1, seed)
        a = R.greedy(*g, 6, method="brute")
        b = R.greedy(*g, 6, method="secular")
        assert np.array_equal(a["order"], b["order"])
        d = np.abs(np.array(a["values"]) - np.array(b["values"]))
        assert np.nanmax(d) < 1e-12
        assert np.array_equal(np.isnan(a["values"]), np.isnan(b["values"]))


def test_restatement_bound_dominates_and_lambda2_never_decreases():
    g = chain_closures(40, 0.1, 1)
    r = R.greedy(*g, 12)
    for vals, u in zip(r["values"], r["bounds"]):
        ok = ~np.isnan(vals)
        assert np.all(u[ok] >= vals[ok] - 1e-12)
    lam = np.concatenate([[r["lam_before"][0]], r["lam2"]])
    assert np.all(np.diff(lam) >= -1e-12)
    assert np.allclose(r["lam_before"][1:], r["lam2"][:-1], rtol=0, atol=1e-12)     # the pick's value is the next graph's lambda_2


def test_restatement_scan_is_first_past_the_tolerance():
    assert R.scan(np.array([1.0, 1.0 + 0.9e-8, 1.0 + 1.8e-8]))[0] == 2
    assert R.scan(np.array([1.0, 1.0 + 0.9e-8]))[0] == 0
    assert R.scan(np.array([np.nan, 0.5e-8]))[0] == -1
