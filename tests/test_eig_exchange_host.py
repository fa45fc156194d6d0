"""The best-swap local search on lambda_2 without a GPU: the two NumPy restatements (tests/eig_exchange_restatement.py) against
each other, the two concavity bounds on every pair, the properties of the input the device test pins a sequence on, the entry
point's presence and the public surface.

Tolerances.  A bound is compared with the value it bounds at 1e-10 (both come from numpy.linalg.eigh of the same 40 to 80 row
matrices).  tol = 1e-8 + 2e-8 ||L||_inf is what a device pick may fall short of the maximum by (tests/test_eig_gpu.py); the pinned
input keeps 100 tol between what decides a round and its nearest competitor."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eig_exchange_restatement as E
import eig_restatement as R
from mac_amd import _lib


def chain_er(n, p, seed):
    """tests/test_eig_gpu.py's generator: links (i, i+1) and ER candidates off the chain, weights uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    iu, ju = np.triu_indices(n, 2)
    pick = rng.random(len(iu)) < p
    return n, fi, fj, fw, iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def random_general(n=200, mc=300, seed=4):
    """tests/test_eig_gpu.py's generator: a random spanning tree plus extra fixed edges; random candidates (some touching node 0)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, n // 2)]); fj = np.concatenate([par, rng.integers(0, n, n // 2)])
    fw = rng.uniform(0.5, 2.0, len(fi))
    ci = np.concatenate([rng.integers(0, n, mc), np.zeros(20, dtype=np.int64)]); cj = rng.integers(0, n, mc + 20)
    return n, fi, fj, fw, ci, cj, rng.uniform(0.5, 2.0, mc + 20)


@functools.lru_cache(maxsize=None)
def pinned():
    """The input of the device's pinned sequence: (graph, greedy start, brute-force run)."""
    g = chain_er(40, 0.1, 1)
    start = E.greedy_start(g, 8)
    return g, start, E.brute(g, start, 100)


# ---- 1. the two restatements ----
@pytest.mark.parametrize("name,start,k,cap", [("chain40", "greedy", 8, 100), ("chain40", "naive", 8, 100), ("general80", "naive", 10, 4)])
def test_pruned_takes_the_swaps_of_brute_and_solves_fewer_pairs(name, start, k, cap):
    g = chain_er(40, 0.1, 1) if name == "chain40" else random_general(80, 60, 4)
    m = len(g[6])
    s = E.greedy_start(g, k) if start == "greedy" else E.naive_start(g, k)
    a = pinned()[2] if (name, start) == ("chain40", "greedy") else E.brute(g, s, cap)
    b = E.pruned(g, s, cap, batch=8)
    solved = [len(r["values"]) for r in b["rounds"]]
    print(f"{name} {start}: swaps {a['swaps']}, lambda_2 {a['lambda2'][0]:.6f} -> {a['lambda2'][-1]:.6f}, solved per round {solved} of {k * (m - k)}")
    assert len(a["swaps"]) >= 1 and a["swaps"] == b["swaps"] and a["converged"] == b["converged"] and a["selection"] == b["selection"]
    assert np.array_equal(a["lambda2"], b["lambda2"])
    assert all(0 < n < k * (m - k) for n in solved)
    for ra, rb in zip(a["rounds"], b["rounds"]):                     # what was solved has brute's value; what was not cannot win
        assert all(abs(v - ra["values"][key]) <= 1e-10 for key, v in rb["values"].items())
        skipped = [v for key, v in ra["values"].items() if key not in rb["values"]]
        assert max(skipped) <= max(rb["top"], rb["tau"]) + 1e-10


# ---- 2. the bounds ----
@pytest.mark.parametrize("name,k", [("chain40", 8), ("general80", 10)])
def test_both_concavity_bounds_hold_on_every_pair(name, k):
    g = chain_er(40, 0.1, 1) if name == "chain40" else random_general(80, 60, 4)
    rows = E.naive_start(g, k)
    vals = E.brute_round(g, rows)["values"]
    U, U1 = E.bound_matrix(g, rows), E.one_pair_bounds(g, rows)
    slack = [min(U[r, f] - vals[(e, f)], U1[r, f] - vals[(e, f)]) for r, e in enumerate(rows) for f in range(len(g[6])) if (e, f) in vals]
    print(f"{name}: {len(slack)} pairs, smallest bound - value = {min(slack):.3e}")
    assert len(slack) == k * (len(g[6]) - k) and min(slack) >= -1e-10


# ---- 3. the input of the device's pinned sequence ----
def test_pinned_input_keeps_its_gaps_and_the_greedy_start_is_not_swap_optimal():
    """chain_er(40, 0.1, 1), K = 8, from the greedy's selection: six swaps, lambda_2 0.167277 -> 0.219864.  At every round the best
    and the second-best swap value are at least 100 tol apart (smallest measured: 8.9e-4), and at the stopping round the best value
    is at least 100 tol away from the acceptance threshold tau + 1e-8 (measured: 7.4e-4): a device whose values are right to tol
    takes these swaps and stops here.  A seed that loses this fails here, not on the GPU."""
    g, start, run = pinned()
    tol = 1e-8 + 2e-8 * max(r["norm"] for r in run["rounds"])
    gaps = [r["best"] - r["second"] for r in run["rounds"]]
    last = abs(run["rounds"][-1]["best"] - (run["rounds"][-1]["tau"] + 1e-8))
    print(f"swaps {run['swaps']}, gaps {['%.2e' % x for x in gaps]}, distance from the threshold at the last round {last:.2e}, 100 tol {100 * tol:.2e}")
    assert run["converged"] and len(run["swaps"]) == 6 and len(run["rounds"]) == 7
    assert abs(run["lambda2"][0] - 0.167277) < 1e-6 and abs(run["lambda2"][-1] - 0.219864) < 1e-6
    assert min(gaps) >= 100 * tol and last >= 100 * tol
    assert all(r["swap"] is not None and r["value"] == r["best"] for r in run["rounds"][:-1])      # the scan's winner is the maximum


# ---- 4. the entry point ----
def test_header_declares_and_library_exports_the_exchange():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 15
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    w = r"\s+\w+\s*"
    ip, dp = r",\s*int32_t\s*\*\s*\w+\s*", r",\s*double\s*\*\s*\w+\s*"
    sig = (r"\bint\s+machip_eig_exchange\s*\(\s*machip_eig\s*\*\s*\w+\s*,\s*int64_t" + w + r",\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int64_t" + w +
           r",\s*double" + w + ip + ip + ip + dp + r",\s*int64_t\s*\*\s*\w+\s*" + ip + ip + dp + r"\)")
    assert re.search(sig, hdr)
    lib = _lib.load()
    assert hasattr(lib, "machip_eig_exchange") and "machip_eig_exchange" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["machip_eig_exchange"]
    assert res is C.c_int and len(args) == 13
    buf = np.zeros(1, dtype=np.int32)
    st = lib.machip_eig_exchange(None, 1, _lib.p_i32(buf), 0, 0.0, None, None, None, None, None, None, None, None)
    assert st == _lib.BAD_ARG and "NULL" in _lib.last_error()
    assert hasattr(_lib.Eig, "exchange") and "eig_xch_max_mb" in _lib.option_names()


# ---- 5. the public surface ----
def test_exchange_signatures_and_solve_option():
    from mac_amd.solvers import MAC, GreedyEig
    p = inspect.signature(MAC.solve).parameters["exchange"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for cls in (GreedyEig, MAC):
        q = inspect.signature(cls.exchange).parameters
        assert list(q) == ["self", "selection", "max_swaps", "min_gain"] and q["max_swaps"].default is None and q["min_gain"].default == 0.0


def test_compat_package_has_the_same_classes():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import mac.solvers as ms
        from mac.solvers.greedy_eig import GreedyEig as by_module
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    import mac_amd.solvers as mine
    assert ms.GreedyEig is mine.GreedyEig is by_module and ms.MAC is mine.MAC
    assert hasattr(ms.GreedyEig, "exchange") and hasattr(ms.MAC, "exchange")


class _NoDevice:
    """Stands where the handle would be: any use of it is device work."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


def test_value_errors_come_before_a_device_is_asked_for(monkeypatch):
    from mac_amd.solvers import MAC, GreedyEig

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_device", no_device)
    ge = GreedyEig.__new__(GreedyEig)
    ge.weights, ge.edge_list, ge._dev = np.ones(3), np.array([[0, 2], [1, 3], [0, 3]]), _NoDevice()
    mac = MAC.__new__(MAC)
    mac.weights, mac._dev, mac._greedy_eig, mac._edges, mac.num_nodes = np.ones(3), _NoDevice(), None, ([], [], 0), 4
    for obj in (ge, mac):
        for sel in (np.zeros((2, 2)), np.array([0.5, 1.0]), np.array([1.0, 2.0, 0.0]), ["a"]):
            with pytest.raises(ValueError, match="selection must be"):
                obj.exchange(sel)
    with pytest.raises(AssertionError, match="the device was asked for"):      # a proper selection gets as far as the device
        ge.exchange([0])
    with pytest.raises(AssertionError, match="the device was asked for"):
        ge.exchange(np.array([1.0, 0.0, 0.0]))
    with pytest.raises(AssertionError, match="the device was asked for"):
        mac.exchange([0])
