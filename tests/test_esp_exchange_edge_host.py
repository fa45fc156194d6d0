"""The exchange in edge space without a GPU: the edge restatement (tests/esp_exchange_edge_restatement.py) against the node-space
restatement that inverts M(S) every round (esp_exchange_restatement.from_scratch), the properties of the inputs the device tests
compare sequences on, the new entry point's presence and the public surface.

Two routes to one number: the restatements' ratios are compared at 1e-10 in the logarithm, as the two node-space restatements are
in tests/test_esp_exchange_host.py; the device's tolerances are those of tests/test_esp_exchange_edge_gpu.py."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import esp_edge_tree_restatement as T
import esp_exchange_edge_restatement as EE
import esp_exchange_restatement as E
import esp_relax_restatement as X
from mac_amd import _lib

SEPARATION_FLOOR = 1e-6


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """(graph, spanning-tree form?)"""
    return {"chain60": lambda: (X.chain_er(60, 0.05, 1), False), "tree40": lambda: (T.tree40(), True),
            "awkward12": lambda: (T.awkward12(), True), "rt70": lambda: (T.random_tree(70, 5, 123, 7), True),
            "rt130deep": lambda: (T.random_tree(130, 9, 190, 9, deep=40), True), "intel50": lambda: (T.intel_fixed50(), True),
            "twins": lambda: (E.twins(), True), "chain100k": lambda: (EE.long_chain(), False),
            "tree40k": lambda: (EE.large_tree(False), True), "tree40kdeep": lambda: (EE.large_tree(True), True)}[name]()


# (graph, start, K or "m//3" / "m-1") of every sequence comparison of tests/test_esp_exchange_edge_gpu.py but the tie graph
SMALL_INPUTS = [("chain60", "naive", 28), ("chain60", "greedy", 28), ("chain60", "naive", 42), ("chain60", "greedy", 42),
                ("tree40", "naive", "m//3"), ("tree40", "naive", 1), ("tree40", "naive", "m-1"),
                ("awkward12", "naive", 1), ("awkward12", "naive", 4), ("awkward12", "naive", "m-1"),
                ("rt70", "naive", "m//3"), ("rt130deep", "naive", "m//3"), ("intel50", "greedy", 245)]
LARGE_INPUTS = [("chain100k", "naive", 100), ("tree40k", "naive", 100), ("tree40kdeep", "naive", 100)]


def start_of(g, start, k):
    m = len(g[6])
    k = {"m-1": m - 1, "m//3": m // 3}.get(k, k)
    return k, (E.naive_start(g, k) if start == "naive" else E.greedy_start(g, k))


@functools.lru_cache(maxsize=None)
def edge_run(name, start, k):
    g, tree = graph_of(name)
    k, sel = start_of(g, start, k)
    return k, sel, EE.run(g, tree, sel, 10 * k)


# ---- 1. the edge restatement against the node-space one ----
@pytest.mark.parametrize("name,start,k", SMALL_INPUTS + [("twins", "naive", 20)])
def test_edge_restatement_takes_the_swaps_of_the_node_space_restatement(name, start, k):
    g, _ = graph_of(name)
    k, sel, run = edge_run(name, start, k)
    ref = (E.incremental if name == "intel50" else E.from_scratch)(g, sel, 10 * k)      # (intel: 42 inverses of 1 727 rows otherwise)
    worst = max([abs(np.log(a) - np.log(b)) for a, b in zip(run["ratios"], ref["ratios"])], default=0.0)
    print(f"{name} {start} K={k}: swaps edge={len(run['out'])} node={len(ref['out'])} largest |log ratio edge - node|={worst:.3e}")
    assert run["out"] == ref["out"] and run["in"] == ref["in"] and run["converged"] == ref["converged"] == 1
    assert np.array_equal(run["selection"], ref["selection"])
    assert worst <= 1e-10


# ---- 2. the inputs of the device's sequence comparisons ----
@pytest.mark.parametrize("name,start,k", SMALL_INPUTS + LARGE_INPUTS)
def test_sequence_inputs_keep_their_separation(name, start, k):
    """The best and the second-best Delta are at least 1e-6 (relative) apart at every round, the stopping round included, on every
    input the device tests compare sequences on: a device whose Delta is right to 1e-9 takes the same swaps.  Smallest
    separations measured on the CPU: rt70 1.6e-4, rt130deep 9.1e-4, intel50 from the greedy start 2.4e-4 (41 swaps), the
    100 000-node chain 2.2e-3 (23 swaps), the large deep tree 1.5e-4."""
    k, _, run = edge_run(name, start, k)
    print(f"{name} {start} K={k}: swaps={len(run['out'])} converged={run['converged']} smallest separation={min(run['separations']):.3e}")
    assert run["converged"] == 1
    assert min(run["separations"]) >= SEPARATION_FLOOR
    if name == "intel50":
        assert len(run["out"]) == 41
    if name == "chain100k":
        assert len(run["out"]) == 23


def test_self_loops_tie_exactly_at_all_but_one_on_the_random_trees():
    """Why K = m - 1 is not compared on the two random trees: their self-loop candidates have Delta = 1 exactly, whichever e."""
    for name in ("rt70", "rt130deep"):
        g, _ = graph_of(name)
        assert np.sum(np.asarray(g[4]) == np.asarray(g[5])) >= 1


def test_twin_graph_has_exact_ties_and_nothing_else_near_the_best():
    """twins() at K = 20 from the naive start: at every round the pairs within 1e-6 of the best are the winner (e, f), (e, f's twin)
    and -- only where e and its twin have both been selected since the start -- the same two with e's twin; the separation is
    exactly 0.  The lowest (e, f) is then decided by exact equality alone.  No edge is exchanged for its twin."""
    g, _ = graph_of("twins")
    k, start, run = edge_run("twins", "naive", 20)
    assert run["converged"] == 1 and len(run["out"]) >= 3 and all(s == 0.0 for s in run["separations"][:-1])
    sel = np.sort(start)
    for t, (e, f) in enumerate(zip(run["out"], run["in"])):
        near = E.near_best(g, sel, SEPARATION_FLOOR)
        es = [e]
        if (e ^ 1) in sel and e in start and (e ^ 1) in start and not {e, e ^ 1} & set(run["in"][:t]):
            es = [e, e ^ 1]
        assert es[0] % 2 == 0 or len(es) == 1
        assert near == [(a, b) for a in es for b in (f, f + 1)] and f % 2 == 0, (e, f, near)
        assert e // 2 != f // 2
        sel = np.sort(np.append(sel[sel != e], f))
    assert np.array_equal(sel, run["selection"])


def test_inputs_have_the_shapes_they_are_there_for():
    shapes = {"chain60": (85, 0, 128), "tree40": (None, 6, 128), "awkward12": (12, 4, 64), "rt70": (123, 5, 128),
              "rt130deep": (190, 9, 256), "intel50": (735, 50, 832), "chain100k": (300, 0, 320), "tree40k": (300, 20, 320),
              "tree40kdeep": (300, 20, 320)}
    for name, (m_want, r_want, ld_want) in shapes.items():
        g, tree = graph_of(name)
        m = len(g[6])
        r = len(T.plan_of(g)["seeds"][2]) if tree else 0
        print(f"{name}: m={m} r={r} ld={(m + r + 63) // 64 * 64}")
        assert (m_want is None or m == m_want) and r == r_want and (m + r + 63) // 64 * 64 == ld_want
    g, _ = graph_of("tree40")
    assert len(g[6]) + 6 == 76
    g, _ = graph_of("rt130deep")
    assert 9 + len(g[6]) // 3 > 64                        # the seeds and the selection cross a fold during the load


# ---- 3. the entry point ----
def test_header_declares_and_library_exports_the_edge_exchange():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 14
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    w = r"\s+\w+\s*"
    sig = (r"\bint\s+machip_esp_exchange_edge\s*\(\s*machip_esp\s*\*\s*\w+\s*,\s*int64_t" + w + r",\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int64_t" + w +
           r",\s*double" + w + r",\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,"
           r"\s*int64_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)")
    assert re.search(sig, hdr)
    lib = _lib.load()
    assert hasattr(lib, "machip_esp_exchange_edge") and "machip_esp_exchange_edge" in _lib.SIGNATURES
    assert _lib.SIGNATURES["machip_esp_exchange_edge"] == _lib.SIGNATURES["machip_esp_exchange"]
    buf, d = np.zeros(1, dtype=np.int32), np.zeros(6)
    n, conv = C.c_int64(0), C.c_int32(0)
    st = lib.machip_esp_exchange_edge(None, 1, _lib.p_i32(buf), 0, 1e-9, _lib.p_i32(buf), _lib.p_i32(buf), _lib.p_i32(buf), _lib.p_f64(d),
                                      C.byref(n), C.byref(conv), _lib.p_f64(d))
    assert st == _lib.BAD_ARG and "NULL" in _lib.last_error()
    assert hasattr(_lib.Esp, "exchange_edge")
    assert list(inspect.signature(_lib.Esp.exchange_edge).parameters) == list(inspect.signature(_lib.Esp.exchange).parameters)


# ---- 4. the public surface ----
def test_exchange_edge_has_the_signature_of_exchange():
    from mac_amd.solvers import ESPRelaxation
    from mac_amd.solvers.esp import exchange_on
    q = inspect.signature(ESPRelaxation.exchange_edge).parameters
    assert list(q) == ["self", "selection", "max_swaps", "min_gain"] and q["max_swaps"].default is None and q["min_gain"].default == 1e-9
    p = inspect.signature(exchange_on).parameters["edge"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


class _NoDevice:
    """Stands where the handle would be: any use of it is device work."""
    matrix_free = True

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for ({name})")


def test_value_errors_come_before_a_device_is_asked_for(monkeypatch):
    from mac_amd.solvers import ESPRelaxation
    from mac_amd.utils.graphs import Edge

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_device", no_device)
    cand = [Edge(0, 2, 1.0), Edge(1, 3, 1.0), Edge(0, 3, 1.0)]
    x0 = np.array([1.0, 0.0, 0.0])

    def relax_of(space):
        relax = ESPRelaxation.__new__(ESPRelaxation)
        relax.all_candidate_edges, relax.weights, relax.edge_space, relax.trace, relax._dev = cand, np.ones(3), space, [], _NoDevice()
        return relax
    node = relax_of(False)
    with pytest.raises(ValueError, match="edge_space"):
        node.exchange_edge([0])
    with pytest.raises(ValueError, match="edge_space"):
        node.solve(1, x0, exchange="edge")
    for space in (False, True, "tree"):
        with pytest.raises(ValueError, match="exchange must be"):
            relax_of(space).solve(1, x0, exchange="node")
    for space in (True, "tree"):
        relax = relax_of(space)
        with pytest.raises(ValueError, match="edge_space"):              # the pinned refusals stay, and point at the new spelling
            relax.solve(1, x0, exchange=True)
        with pytest.raises(ValueError, match="edge_space.*exchange_edge"):
            relax.exchange([0])
        with pytest.raises(AssertionError, match="the device was asked for"):      # the new spelling gets as far as the device
            relax.exchange_edge([0])
        with pytest.raises(AssertionError, match="the device was asked for"):
            relax.solve(1, x0, exchange="edge")
        with pytest.raises(ValueError, match="selection"):
            relax.exchange_edge(np.array([0.5, 2.0]))
