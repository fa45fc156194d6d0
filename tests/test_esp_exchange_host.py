"""The exchange on the log tree count without a GPU: the swap formula against log-determinants, the two NumPy restatements
(tests/esp_exchange_restatement.py) against each other, the properties of the inputs the device tests compare sequences on,
the new entry point's presence and the public surface.

Tolerance of a swap's ratio: log Delta against log det M' - log det M, within the sum of esp_relax_restatement.F_tolerance at the
two selections (each 10 max(d, 1e-13 |logdet|), d the disagreement of dense LU and SuperLU on that matrix); nothing is
hard-coded."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
import esp_exchange_restatement as E
import esp_relax_restatement as X
from mac_amd import _lib

SEPARATION_FLOOR = 1e-6


def small_random():
    return X.chain_er(30, 0.08, 3)


# ---- 1. the formula ----
@pytest.mark.parametrize("case,k", [("petersen", 2), ("small_random", 5)])
def test_swap_formula_equals_the_ratio_of_determinants_for_every_pair(case, k):
    g = X.petersen() if case == "petersen" else small_random()
    m = len(g[6])
    sel = E.naive_start(g, k)
    unsel = np.setdiff1d(np.arange(m), sel)
    assert len(unsel) >= 2
    D, _ = E.delta_matrix(g, np.linalg.inv(X.M_of(g, E.indicator(m, sel))), sel, unsel)
    worst = 0.0
    for a, e in enumerate(sel):
        for b, f in enumerate(unsel):
            ref, tol = E.log_ratio_check(g, sel, e, f)
            err = abs(np.log(D[a, b]) - ref)
            worst = max(worst, err / tol)
            assert err <= tol, (e, f, D[a, b], np.exp(ref), err, tol)
    print(f"{case}: {D.size} pairs, largest |log Delta - (logdet M' - logdet M)| / tolerance = {worst:.3g}")


# ---- 2. the two restatements ----
@pytest.mark.parametrize("k", [164, 273])
def test_the_two_restatements_take_the_same_swaps_from_the_greedy_start(k):
    g = X.random_general()
    start = E.greedy_start(g, k)
    a, b = E.from_scratch(g, start, 10 * k), E.incremental(g, start, 10 * k)
    print(f"K={k}: out={a['out']} in={a['in']} growth={np.sum(np.log(a['ratios'])):.6f}")
    assert len(a["out"]) >= 1 and a["converged"] == 1 and b["converged"] == 1
    assert a["out"] == b["out"] and a["in"] == b["in"] and np.array_equal(a["selection"], b["selection"])
    for t, (ra, rb) in enumerate(zip(a["ratios"], b["ratios"])):
        assert abs(np.log(ra) - np.log(rb)) <= 1e-10, (t, ra, rb)      # (two routes to one number; the device's tolerance is test 1's)


# ---- 3. the inputs of the device's sequence comparisons ----
@functools.lru_cache(maxsize=None)
def graph_of(name):
    if name == "intel":
        g = load_golden("g2o_intel")
        return (int(g["n"]), np.asarray(g["fi"]), np.asarray(g["fj"]), np.asarray(g["fw"], dtype=np.float64),
                np.asarray(g["ci"]), np.asarray(g["cj"]), np.asarray(g["cw"], dtype=np.float64))
    return {"petersen": X.petersen, "general500": X.random_general, "awkward65": lambda: E.awkward(65), "awkward66": lambda: E.awkward(66)}[name]()


# (graph, start, K or None for m - 1 / m // 3, max_swaps or None for 10 K) of every sequence comparison of tests/test_esp_exchange_gpu.py;
# the graph and the start of a case are built when that case runs, not at collection and not once per case
SEQUENCE_INPUTS = [("petersen", "naive", 2, 20), ("general500", "greedy", 164, None), ("general500", "greedy", 273, None),
                   ("general500", "naive", 164, 40),
                   ("awkward65", "naive", 1, None), ("awkward65", "naive", 37, None), ("awkward65", "naive", "m-1", None),
                   ("awkward66", "naive", 1, None), ("awkward66", "naive", 37, None), ("awkward66", "naive", "m-1", None),
                   ("intel", "greedy", "m//3", None)]


@pytest.mark.parametrize("name,start,k,cap", SEQUENCE_INPUTS)
def test_sequence_inputs_keep_their_separation(name, start, k, cap):
    """On every graph and start the device tests compare swap sequences on -- against the restatement, or, on intel, between the
    chain form and the dense form -- the restatement takes at least one swap and the best and the second-best Delta are at
    least 1e-6 (relative) apart at every round, the stopping round included: a device whose Delta is right to 1e-9 takes the
    same swaps, and no round may be left out of a comparison.  Smallest separations measured: Petersen 8.3e-2 at its one swap
    and 3.3e-2 at the stopping round; general500 greedy starts 2.7e-5 and 3.7e-4 (5 and 4 swaps); general500 naive start
    K = 164 1.1e-4 over the first 40 swaps; the ld = 64 / 128 graphs >= 4.7e-5; intel 7.9e-6 (43 swaps)."""
    g = graph_of(name)
    m = len(g[6])
    k = {"m-1": m - 1, "m//3": m // 3}.get(k, k)
    sel = E.naive_start(g, k) if start == "naive" else E.greedy_start(g, k)
    run = (E.incremental if name == "intel" else E.from_scratch)(g, sel, 10 * k if cap is None else cap)      # (intel: 44 inverses of 1 727 rows otherwise)
    print(f"{name} {start} K={k}: swaps={len(run['out'])} converged={run['converged']} smallest separation={min(run['separations']):.3e}")
    assert len(run["out"]) >= 1
    assert min(run["separations"]) >= SEPARATION_FLOOR


def test_twin_graph_has_exact_ties_and_nothing_else_near_the_best():
    """Every candidate of twins() is listed twice: the separation is exactly 0 at every round.  What the device's tie rule is
    tested on: at every round the pairs within 1e-6 of the best are the winner (e, f), (e, f's twin) and -- only where e and its
    twin have both been selected since the start, so that the same arithmetic has run on both -- the same two with e's twin.
    The lowest (e, f) is then decided by exact equality alone, on the device as here.  No edge is ever exchanged for its twin."""
    g = E.twins()
    start = E.naive_start(g, 10)
    run = E.from_scratch(g, start, 100)
    assert run["converged"] == 1 and len(run["out"]) >= 3 and all(s == 0.0 for s in run["separations"][:-1])
    sel = np.sort(start)
    both = 0
    for t, (e, f) in enumerate(zip(run["out"], run["in"])):
        near = E.near_best(g, sel, SEPARATION_FLOOR)
        es = [e]
        if (e ^ 1) in sel and e in start and (e ^ 1) in start and not {e, e ^ 1} & set(run["in"][:t]):
            es, both = [e, e ^ 1], both + 1
        assert es[0] % 2 == 0 or len(es) == 1
        assert near == [(a, b) for a in es for b in (f, f + 1)] and f % 2 == 0, (e, f, near)
        assert e // 2 != f // 2
        sel = np.sort(np.append(sel[sel != e], f))
    assert both >= 1                                 # (ties in e as well as in f are on the path)
    assert np.array_equal(sel, run["selection"])


def test_awkward_graphs_have_the_shapes_they_are_there_for():
    for n, ld in ((65, 64), (66, 128)):
        g = E.awkward(n)
        m = len(g[6])
        assert (n - 1 + 63) // 64 * 64 == ld and m % 256 != 0 and 37 % 64 != 0
        assert np.all(np.asarray(g[4])[:7:2] == 0) and g[4][5] == g[5][5]
        for k in (1, 37, m - 1):
            assert 5 not in E.from_scratch(g, E.naive_start(g, k), 10 * k)["in"]      # the self-loop is never swapped in


# ---- 4. the entry point ----
def test_header_declares_and_library_exports_the_exchange():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    w = r"\s+\w+\s*"
    sig = (r"\bint\s+machip_esp_exchange\s*\(\s*machip_esp\s*\*\s*\w+\s*,\s*int64_t" + w + r",\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int64_t" + w +
           r",\s*double" + w + r",\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,"
           r"\s*int64_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)")
    assert re.search(sig, hdr)
    lib = _lib.load()
    assert hasattr(lib, "machip_esp_exchange") and "machip_esp_exchange" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["machip_esp_exchange"]
    assert res is C.c_int and len(args) == 12
    buf, d = np.zeros(1, dtype=np.int32), np.zeros(6)
    n, conv = C.c_int64(0), C.c_int32(0)
    st = lib.machip_esp_exchange(None, 1, _lib.p_i32(buf), 0, 1e-9, _lib.p_i32(buf), _lib.p_i32(buf), _lib.p_i32(buf), _lib.p_f64(d),
                                 C.byref(n), C.byref(conv), _lib.p_f64(d))
    assert st == _lib.BAD_ARG and "NULL" in _lib.last_error()
    assert hasattr(_lib.Esp, "exchange")
    for name in ("esp_xch_lds_kb", "esp_xch_max_mb"):
        assert name in _lib.option_names()


# ---- 5. the public surface ----
def test_exchange_is_keyword_only_and_off_by_default_on_solve():
    from mac_amd.solvers import ESPRelaxation, GreedyESP
    p = inspect.signature(ESPRelaxation.solve).parameters["exchange"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for cls in (GreedyESP, ESPRelaxation):
        q = inspect.signature(cls.exchange).parameters
        assert list(q) == ["self", "selection", "max_swaps", "min_gain"] and q["max_swaps"].default is None and q["min_gain"].default == 1e-9


def test_compat_package_has_the_same_classes():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import mac.solvers as ms
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    import mac_amd.solvers as mine
    assert ms.GreedyESP is mine.GreedyESP and ms.ESPRelaxation is mine.ESPRelaxation
    assert hasattr(ms.GreedyESP, "exchange") and hasattr(ms.ESPRelaxation, "exchange")


class _NoDevice:
    """Stands where the handle would be: any use of it is device work."""
    matrix_free = True

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


def test_value_errors_come_before_a_device_is_asked_for(monkeypatch):
    from mac_amd.solvers import ESPRelaxation, GreedyESP
    from mac_amd.utils.graphs import Edge

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_device", no_device)
    cand = [Edge(0, 2, 1.0), Edge(1, 3, 1.0), Edge(0, 3, 1.0)]
    for space in (True, "tree"):
        relax = ESPRelaxation.__new__(ESPRelaxation)
        relax.all_candidate_edges, relax.weights, relax.edge_space, relax.trace, relax._dev = cand, np.ones(3), space, [], _NoDevice()
        with pytest.raises(ValueError, match="edge_space"):
            relax.solve(1, np.array([1.0, 0.0, 0.0]), exchange=True)
        with pytest.raises(ValueError, match="edge_space"):
            relax.exchange([0])
        with pytest.raises(AssertionError, match="the device was asked for"):      # without the option the call gets as far as the device
            relax.solve(1, np.array([1.0, 0.0, 0.0]))
    ge = GreedyESP.__new__(GreedyESP)
    ge.all_candidate_edges, ge._dev = cand, _NoDevice()
    for sel in ([0], np.array([1.0, 0.0, 0.0])):
        with pytest.raises(ValueError, match="matrix_free"):
            ge.exchange(sel)
