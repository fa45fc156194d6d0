"""machip_lowest_pairs without a device: the NumPy restatement of its algorithm (tests/lowest_pairs_restatement.py) against dense
eigh on every graph the GPU tests use -- which also pins that those inputs are within reach of the method --, the exported
symbols, and the argument checks that are made before a device is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import lowest_pairs_restatement as R
from conftest import load_golden
from mac_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_L(name):
    g = load_golden(name)
    n = int(g["n"])
    return sp.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=(n, n))


def pose_L(name, at):
    g = load_golden(name)
    return R.laplacian(*R.golden_graph(g, np.ones(len(g["cw"])) if at == "ones" else g["x_init"]))


CASES = {name: (lambda gr=gr: R.laplacian(*gr), 4, 0) for name, gr in R.small_graphs().items()}
CASES.update({
    "mirror": (lambda: R.laplacian(*R.mirror_graph()), 4, 0),
    "er300_x0": (lambda: golden_L("er300_x0"), 4, 0),
    "er2000_x0": (lambda: golden_L("er2000_x0"), 4, 0),
    "sphere2500_ones": (lambda: pose_L("g2o_sphere2500", "ones"), 8, 0),
    "sphere2500_init": (lambda: pose_L("g2o_sphere2500", "init"), 8, 0),
    "intel_init": (lambda: pose_L("g2o_intel", "init"), 4, 20000),
})


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_finds_the_lowest_pairs(name):
    make, q, max_steps = CASES[name]
    L = make()
    lams, V, info = R.lowest_pairs(L, q, max_steps=max_steps)
    R.assert_pairs(name, L, lams, V, info)
    assert info["reordered"] == 0 and info["first_rank"] == 0


def test_restatement_multiplicities_and_restarts():
    """Exact multiplicities come out of fresh start vectors (K5: 5 four times, one step per column; C64: two double values; P300
    runs its basis to n - 1 - c), and a basis cap of 32 forces restarts on er300_x0 without changing what is found."""
    gs = R.small_graphs()
    lams, _, info = R.lowest_pairs(R.laplacian(*gs["k5"]), 4)
    assert np.allclose(lams, 5.0, atol=1e-12) and np.all(info["steps"] <= 4) and np.all(info["restarts"] == 0)
    lams, _, _ = R.lowest_pairs(R.laplacian(*gs["c64"]), 4)
    assert np.allclose(lams, 2 - 2 * np.cos(2 * np.pi * np.array([1, 1, 2, 2]) / 64), atol=1e-12)
    lams, _, info = R.lowest_pairs(R.laplacian(*gs["p300"]), 4)
    assert np.allclose(lams, 2 - 2 * np.cos(np.arange(1, 5) * np.pi / 300), atol=1e-12) and info["steps"].max() >= 290
    L = golden_L("er300_x0")
    free, _, _ = R.lowest_pairs(L, 4)
    lams, V, info = R.lowest_pairs(L, 4, vcap=32)
    R.assert_pairs("er300_x0", L, lams, V, info)
    assert np.all(info["restarts"] >= 1) and np.abs(lams - free).max() <= 2e-8 * R.lnorm_inf(L)


def test_restatement_reports_a_capped_column():
    L = R.laplacian(*R.small_graphs()["p300"])
    lams, V, info = R.lowest_pairs(L, 4, max_steps=8)
    bad = info["status"] == R.NOT_CONVERGED
    assert bad.any() and np.all(info["residual"][bad] >= 1e-8)


def test_library_exports_and_abi():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 19
    lib = _lib.load()
    assert lib.machip_version() >= 19
    for name in ("machip_lowest_pairs", "machip_lowest_pairs_csr", "machip_lowest_pairs_time", "machip_gradient_block"):
        assert re.search(r"\b%s\(" % name, hdr) and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["machip_lowest_pairs_csr"][1][-8:] == _lib.SIGNATURES["machip_lowest_pairs"][1][-8:]
    assert "pairs_vcap" in _lib.option_names()
    from mac_amd.solvers import MAC
    from mac_amd.utils import fiedler
    assert hasattr(fiedler, "find_lowest_pairs") and hasattr(MAC, "lowest_pairs") and hasattr(MAC, "problem_block")
    assert hasattr(_lib.Problem, "lowest_pairs") and _lib.PAIRS_CHUNK == R.CHUNK
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from mac.utils.fiedler import find_lowest_pairs; "
            "import mac_amd.utils.fiedler as f; assert find_lowest_pairs is f.find_lowest_pairs" % (ROOT, os.path.join(ROOT, "compat")))
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0      # the reference's module path, through compat/


@pytest.mark.parametrize("n,q", [(5, 0), (5, -1), (40, 17), (5, 5), (3, 3)])
def test_q_out_of_range_is_refused_before_any_device_call(n, q):
    """1 <= q <= min(16, n - 1): BAD_ARG (an AssertionError here, as for every argument the reference asserts on) -- on a
    machine without a GPU too, so the check comes before the device is looked for."""
    L = R.laplacian(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1))
    with pytest.raises(AssertionError, match="BAD_ARG"):
        _lib.lowest_pairs_csr(L.indptr, L.indices, L.data, n, q=q, X0=None)
