"""The preconditioned deflated columns of machip_lowest_pairs without a device: the NumPy restatement
(tests/lowest_pairs_lob_restatement.py) on every input tests/test_lowest_pairs_lob_gpu.py runs, its damaged variants, and the
interface -- exports, option, the `method` keyword.

The GPU tests allow the device no restart and no Lanczos finish, so the restatement must stay inside that itself on every input:
it does, with drift max |Q^T x| / ||x|| <= 2.1e-15 (allowed 1e-12)."""
import inspect
import os
import re

import numpy as np
import pytest

import lowest_pairs_lob_restatement as PL
import lowest_pairs_restatement as R
from mac_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(PL.SYNTH) + list(PL.GOLDEN) + list(PL.SMALL)


@pytest.mark.parametrize("name", ALL)
def test_restatement_converges_without_restart_or_drift(name):
    I = PL.problem(name)
    lams, V, info = PL.reference(name)
    print(name, "n", I.L.shape[0], "closures", I.s, "exact", I.exact, "J_ref", info["J_ref"], "drift", info["drift"])
    assert np.all(info["status"] == PL.OK) and np.all(info["restarts"] == 0)
    assert np.all(info["drift"] <= 1e-12)
    PL.assert_values(name, I.L, lams, V, info)


@pytest.mark.parametrize("name", ["g2o_intel", "n1025_s65_kinds", "c64", "tri_n300_s30"])
@pytest.mark.parametrize("variant", ["no_projection", "skip_last_locked"])
def test_a_missing_projection_shows_in_the_values(name, variant):
    """Without the projection, or with the newest locked column left out of it, a column converges to an eigenpair that is locked
    already: the sorted values repeat one and miss another by far more than the stop rule resolves."""
    I = PL.problem(name)
    ev, _, lnorm = R.dense_spectrum(name, I.L)
    lams, _, info = PL.lowest_pairs(I.L, I.q, I.exact, lob_chunk=I.lob_chunk, variant=variant, cap=2000)
    dev = np.abs(lams - ev[1:I.q + 1])
    print(name, variant, dev / lnorm, info["drift"])
    assert np.any(dev > 1e-8 * lnorm) and info["drift"].max() > 1e-3


def test_exports_and_option():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 20
    lib = _lib.load()
    assert lib.machip_version() >= 20
    for name in ("machip_lowest_pairs_info", "machip_lowest_pairs_csr2"):
        assert re.search(r"\b%s\(" % name, hdr) and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["machip_lowest_pairs_csr2"][1][:18] == _lib.SIGNATURES["machip_lowest_pairs_csr"][1]
    assert "pairs_precond" in _lib.option_names() and "pairs_precond" in hdr
    assert _lib.PAIRS_METHODS == {"lanczos": 0, "lobpcg": 1}
    src = open(os.path.join(ROOT, "mac_amd", "csrc", "solver_pairs.h")).read()
    assert int(re.search(r"kPairsModeFinished = (\d+)", src).group(1)) == _lib.PAIRS_MODE_FINISHED


def test_method_keyword_everywhere():
    from mac_amd.solvers import MAC
    from mac_amd.utils import fiedler
    for f in (fiedler.find_lowest_pairs, _lib.Problem.lowest_pairs, _lib.lowest_pairs_csr, MAC.lowest_pairs, MAC.problem_block):
        assert inspect.signature(f).parameters["method"].default == "lanczos", f
    import subprocess
    import sys
    code = ("import sys, inspect; sys.path.insert(0, %r); sys.path.insert(0, %r); from mac.utils.fiedler import find_lowest_pairs; "
            "from mac.solvers import MAC; assert 'method' in inspect.signature(find_lowest_pairs).parameters; "
            "assert 'method' in inspect.signature(MAC.lowest_pairs).parameters" % (ROOT, os.path.join(ROOT, "compat")))
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0      # compat/ inherits the keyword


def test_an_unknown_method_is_refused_before_any_device_call():
    L = R.laplacian(*R.small_graphs()["k5"])
    with pytest.raises(KeyError):
        _lib.lowest_pairs_csr(L.indptr, L.indices, L.data, 5, q=2, X0=None, method="tracemin")
