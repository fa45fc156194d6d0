"""GreedyEig.exchange_free without a GPU: the blocked history load against the sequential one and against the inverse it stands for
(tests/eig_exchange_free_restatement.py), the compaction rule, the two new entry points' presence, the public surface, and the
properties of the three inputs the device test pins sequences on.

Tolerances.  Blocked against sequential: 1e-12 relative to the largest entry (the algebra is exact; both are a few hundred
floating-point operations per entry on matrices whose condition is below 1e4).  Against numpy.linalg.inv: 1e-12 relative as well
(measured: 2.4e-13 at 299 rows, 7.5e-14 at 39).  tol = 1e-8 + 2e-8 ||L||_inf is what a device pick may
fall short of the maximum by (tests/test_eig_gpu.py); a pinned input keeps 100 tol between what decides a round and its nearest
competitor."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eig_exchange_free_restatement as X
import eig_exchange_restatement as E
import eig_restatement as R
from mac_amd import _lib
from test_eig_exchange_host import _NoDevice, chain_er


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- 1. the blocked load ----
def load_case(g, picks, removed):
    """Edges to load: the candidates `picks` in order, then the negated copies of picks[removed] (downdates), then the rest."""
    n, fi, fj, fw, ci, cj, cw = g
    head, tail = picks[:len(picks) // 2], picks[len(picks) // 2:]
    seq = [(e, 1.0) for e in head] + [(head[r], -1.0) for r in removed] + [(e, 1.0) for e in tail]
    idx = np.array([e for e, _ in seq])
    w = np.array([s * cw[e] for e, s in seq])
    left = sorted(set(head) - {head[r] for r in removed}) + list(tail)
    return X.incidence(n, np.asarray(ci)[idx], np.asarray(cj)[idx]), w, left


@pytest.mark.parametrize("block", [1, 7, 64])
@pytest.mark.parametrize("name", ["chain40", "chain300"])
def test_blocked_load_equals_sequential_and_the_inverse(name, block):
    g = chain_er(40, 0.1, 1) if name == "chain40" else chain_er(300, 0.03, 0)
    n, fi, fj, fw = g[:4]
    picks = list(range(12)) if name == "chain40" else list(range(0, 150, 2))      # (75 edges: a full block of 64 and a short one)
    A, w, left = load_case(g, picks, removed=[1, 4])
    neg = np.flatnonzero(w < 0)
    assert len(neg) == 2 and (block == 1 or any(q % block > 0 for q in neg))      # a downdate inside a block
    S0 = X.sigma0_of(n, fi, fj, fw)
    Zs, cs = X.sequential(S0, A, w)
    Zb, cb = X.blocked(S0, A, w, block=block)
    inv = np.linalg.inv(E.lap_of(g, left)[1:, 1:])
    errs = rel(Zb, Zs), rel(cb, cs), rel(X.implied_inverse(S0, Zb, cb), inv)
    print(f"{name} block {block}: Z {errs[0]:.2e}, c {errs[1]:.2e}, inverse {errs[2]:.2e}")
    assert errs[0] <= 1e-12 and errs[1] <= 1e-12 and errs[2] <= 1e-12
    assert np.all(cb[w < 0] < 0)                                # a downdate's coefficient keeps its sign: 1 - w_e s_e > 0


def test_blocked_load_on_a_tree_with_seeds():
    """The tree route's history: Sigma0 of the spanning tree, the fixed links outside it first (sequentially, as the handle seeds
    them), then the selection as one block."""
    g = X.with_closures(chain_er(40, 0.1, 1), 5)
    n, fi, fj, fw, ci, cj, cw = g
    plan = _lib.host_esp_tree(n, fi, fj, fw)
    su, sv, sw = plan["seeds"]
    assert len(sw) == 5
    S0 = X.sigma0_of(n, *X.tree_edges(plan["parent"], plan["R"]))
    Z1, c1 = X.sequential(S0, X.incidence(n, su, sv), sw)
    sel = [0, 3, 4, 9, 11, 17, 20, 21]
    Z2, c2 = X.blocked(X.implied_inverse(S0, Z1, c1), X.incidence(n, ci[sel], cj[sel]), cw[sel])
    got = X.implied_inverse(S0, np.hstack([Z1, Z2]), np.concatenate([c1, c2]))
    assert rel(got, np.linalg.inv(E.lap_of(g, sel)[1:, 1:])) <= 1e-12


def test_compaction_rule():
    assert X.compaction_rule(8, 5, 32, 11) == (0, 5 + 8 + 22)
    assert X.compaction_rule(8, 5, 2, 11) == (5, 5 + 8 + 2)       # rounds 3, 5, 7, 9, 11 compact; the stopping round 12 does not
    assert X.compaction_rule(8, 5, 1, 11) == (11, 5 + 8)          # every round after the first, the stopping one included
    assert X.compaction_rule(8, 0, 1, 3, converged=False) == (2, 8 + 2)
    assert X.compaction_rule(8, 0, 0, 0, converged=False) == (0, 8)


# ---- 2. the entry points ----
def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 18
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    w = r"\s+\w+\s*"
    ip, dp, lp = r",\s*int32_t\s*\*\s*\w+\s*", r",\s*double\s*\*\s*\w+\s*", r",\s*int64_t\s*\*\s*\w+\s*"
    sig = (r"\bint\s+machip_eig_exchange_free\s*\(\s*machip_eig\s*\*\s*\w+\s*,\s*int64_t" + w + r",\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int64_t" + w +
           r",\s*double" + w + ip + ip + ip + dp + lp + ip + ip + dp + lp + r"\)")
    assert re.search(sig, hdr)
    assert re.search(r"\bint\s+machip_eig_history\s*\(\s*machip_eig\s*\*\s*\w+\s*,\s*int64_t" + w + dp + dp + lp + r"\)", hdr)
    lib = _lib.load()
    for name, nargs in (("machip_eig_exchange_free", 14), ("machip_eig_history", 5)):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    assert _lib.SIGNATURES["machip_eig_exchange_free"][1][:13] == _lib.SIGNATURES["machip_eig_exchange"][1]
    buf = np.zeros(1, dtype=np.int32)
    st = lib.machip_eig_exchange_free(None, 1, _lib.p_i32(buf), 0, 0.0, None, None, None, None, None, None, None, None, None)
    assert st == _lib.BAD_ARG and "NULL" in _lib.last_error()
    st = lib.machip_eig_history(None, 0, None, None, None)
    assert st == _lib.BAD_ARG and "NULL" in _lib.last_error()
    assert hasattr(_lib.Eig, "exchange_free") and hasattr(_lib.Eig, "history")


def test_option_is_in_the_table():
    assert "eig_xch_free_swaps" in _lib.option_names() and "eig_xch_max_mb" in _lib.option_names()


# ---- 3. the public surface ----
def test_signatures():
    from mac_amd.solvers import MAC, GreedyEig
    for cls in (GreedyEig, MAC):
        q = inspect.signature(cls.exchange_free).parameters
        assert list(q) == ["self", "selection", "max_swaps", "min_gain"] and q["max_swaps"].default is None and q["min_gain"].default == 0.0


def test_value_errors_come_before_a_device_is_asked_for(monkeypatch):
    from mac_amd.solvers import MAC, GreedyEig

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_device", no_device)

    def stand_in(matrix_free):
        ge = GreedyEig.__new__(GreedyEig)
        ge.weights, ge.edge_list, ge._dev, ge._matrix_free = np.ones(3), np.array([[0, 2], [1, 3], [0, 3]]), _NoDevice(), matrix_free
        return ge
    mac = MAC.__new__(MAC)
    mac.weights, mac._dev, mac._greedy_eig, mac._greedy_eig_free, mac._edges, mac.num_nodes = np.ones(3), _NoDevice(), None, None, ([], [], 0), 4
    for obj in (stand_in(True), stand_in("tree"), stand_in(False), mac):
        for sel in (np.zeros((2, 2)), np.array([0.5, 1.0]), np.array([1.0, 2.0, 0.0]), ["a"]):
            with pytest.raises(ValueError, match="selection must be"):
                obj.exchange_free(sel)
    for sel in ([0], np.array([1.0, 0.0, 0.0])):
        with pytest.raises(ValueError, match="use exchange$"):                 # a dense handle: named, and no device work
            stand_in(False).exchange_free(sel)
        for mf in (True, "tree"):
            with pytest.raises(AssertionError, match="the device was asked for"):  # a proper selection gets as far as the device
                stand_in(mf).exchange_free(sel)
    with pytest.raises(AssertionError, match="the device was asked for"):
        mac.exchange_free([0])


# ---- 4. the inputs of the device's pinned sequences ----
@functools.lru_cache(maxsize=None)
def pinned(case):
    """(graph, start, brute-force run) of the device test's cases (a), (b), (c)."""
    if case == "a":
        g = chain_er(40, 0.1, 1)
        start = E.greedy_start(g, 8)
    elif case == "b":
        g = X.with_closures(chain_er(40, 0.1, 2), 5)
        start = E.naive_start(g, 8)
    else:
        g = X.with_closures(chain_er(40, 0.1, 1), 5)
        start = E.greedy_start(g, 8)
    return g, start, E.brute(g, start, 100)


def gaps_of(run):
    """(smallest best - second-best over the rounds, the last round's distance to tau + 1e-8), in units of tol."""
    tol = 1e-8 + 2e-8 * max(r["norm"] for r in run["rounds"])
    gaps = [r["best"] - r["second"] for r in run["rounds"]]
    last = abs(run["rounds"][-1]["best"] - (run["rounds"][-1]["tau"] + 1e-8))
    return min(gaps) / tol, last / tol, tol


@pytest.mark.parametrize("case,swaps", [("a", 6), ("b", 4), ("c", 11)])
def test_pinned_inputs_keep_their_gaps(case, swaps):
    """(a) six swaps, the pinned case of tests/test_eig_exchange_host.py.  (b) four swaps, smallest gap 2 100 tol.  (c) eleven swaps,
    smallest gap 926 tol.  All converge; every round keeps 100 tol between the best and the second-best swap, and the stopping round
    100 tol between its best value and the threshold: a device whose values are right to tol takes these swaps and stops there."""
    g, start, run = pinned(case)
    gap, last, tol = gaps_of(run)
    print(f"({case}) swaps {run['swaps']}, smallest gap {gap:.0f} tol, last round's distance to the threshold {last:.0f} tol, tol {tol:.2e}")
    assert run["converged"] and len(run["swaps"]) == swaps and len(run["rounds"]) == swaps + 1
    assert gap >= 100 and last >= 100
    assert all(r["swap"] is not None and r["value"] == r["best"] for r in run["rounds"][:-1])      # the scan's winner is the maximum
    if case != "a":
        assert len(_lib.host_esp_tree(g[0], g[1], g[2], g[3])["seeds"][2]) == 5
