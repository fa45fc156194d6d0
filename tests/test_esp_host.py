"""GreedyESP without a GPU: the public surface, the error paths of the C entry point (checked on the host before any device
work) and the NumPy restatement of the rule against closed forms."""
import ctypes as C
import os
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest

from conftest import ROOT
import esp_restatement as R
from mac_amd import _lib


def test_greedy_esp_is_exported_from_mac_amd_and_mac_solvers():
    import mac_amd.solvers
    from mac_amd.solvers import GreedyESP
    assert "GreedyESP" in mac_amd.solvers.__all__ and GreedyESP.__module__ == "mac_amd.solvers.esp"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from mac.solvers import GreedyESP\nimport mac_amd.solvers\nassert GreedyESP is mac_amd.solvers.GreedyESP\nprint('ok')"
            % (ROOT, os.path.join(ROOT, "compat")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp", timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-1500:]


def test_construction_without_a_device_raises_machip_error(monkeypatch):
    from mac_amd.solvers import GreedyESP
    from mac_amd.utils.graphs import Edge
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.MachipError) as ei:
        GreedyESP([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3)
    assert ei.value.status == _lib.NO_DEVICE


def _create_status(n, fixed, cand, fold=64, flags=0):
    lib = _lib.load()
    fi, fj, fw = (np.array([e[q] for e in fixed], dtype=t) for q, t in ((0, np.int32), (1, np.int32), (2, np.float64)))
    ci, cj, cw = (np.array([e[q] for e in cand], dtype=t) for q, t in ((0, np.int32), (1, np.int32), (2, np.float64)))
    h = C.c_void_p()
    st = lib.machip_esp_create(0, n, len(fw), _lib.p_i32(fi), _lib.p_i32(fj), _lib.p_f64(fw), len(cw), _lib.p_i32(ci),
                               _lib.p_i32(cj), _lib.p_f64(cw), fold, flags, C.byref(h))
    if st == _lib.OK:
        lib.machip_esp_destroy(h)
    return st, _lib.last_error()


def test_create_rejects_sizes_beyond_the_dense_limits():
    n = 40000
    st, msg = _create_status(n, [(i, i + 1, 1.0) for i in range(n - 1)], [(0, 5, 1.0)])
    assert st == _lib.BAD_ARG and "32768" in msg
    n = 20000
    st, msg = _create_status(n, [(i, i + 1, 1.0) for i in range(n - 1)] + [(0, 2, 1.0)], [(0, 5, 1.0)])
    assert st == _lib.BAD_ARG and "16384" in msg
    st, msg = _create_status(n, [(i, i + 1, 1.0) for i in range(n - 1)], [(0, 5, 1.0)], flags=_lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "16384" in msg


def test_create_rejects_bad_arguments_and_an_unconnected_node():
    chain = [(i, i + 1, 1.0) for i in range(5)]
    assert _create_status(6, chain, [(0, 9, 1.0)])[0] == _lib.BAD_ARG         # node id out of range
    assert _create_status(6, chain, [(0, 3, 1.0)], fold=257)[0] == _lib.BAD_ARG
    assert _create_status(6, chain, [(0, 3, 1.0)], flags=2)[0] == _lib.BAD_ARG
    st, msg = _create_status(6, [(0, 1, 1.0), (1, 2, 1.0), (3, 4, 1.0)], [(0, 5, 1.0)])     # node 5 has no fixed edge
    assert st == _lib.DISCONNECTED and "node 5" in msg


def test_restatement_chain_resistance_is_the_sum_of_link_resistances():
    rng = np.random.default_rng(3)
    n = 40
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.3, 3.0, n - 1)
    Sig, beta = R.initial_sigma(n, fi, fj, fw)
    assert beta == 0.0
    ci = rng.integers(0, n, 200); cj = rng.integers(0, n, 200); cw = rng.uniform(0.5, 2.0, 200)
    s = R.scores(Sig, ci, cj, cw)
    link = np.concatenate([[0.0], np.cumsum(1.0 / fw)])     # resistance from node 0
    closed = cw * np.abs(link[ci] - link[cj])
    assert np.allclose(s, closed, rtol=1e-11, atol=1e-13)


def test_restatement_tree_path_resistance_on_petersen():
    G = nx.petersen_graph()
    T = nx.minimum_spanning_tree(G)
    rng = np.random.default_rng(5)
    for a, b in T.edges:
        T[a][b]["weight"] = float(rng.uniform(0.5, 2.0))
    fi, fj = np.array([a for a, _ in T.edges]), np.array([b for _, b in T.edges])
    fw = np.array([T[a][b]["weight"] for a, b in T.edges])
    cand = list(nx.difference(G, T).edges)
    ci, cj = np.array([a for a, _ in cand]), np.array([b for _, b in cand])
    cw = rng.uniform(0.5, 2.0, len(cand))
    Sig, beta = R.initial_sigma(10, fi, fj, fw)
    assert beta == 0.0
    s = R.scores(Sig, ci, cj, cw)
    H = nx.Graph()
    H.add_weighted_edges_from((a, b, 1.0 / T[a][b]["weight"]) for a, b in T.edges)
    path = np.array([nx.shortest_path_length(H, a, b, weight="weight") for a, b in cand])
    assert np.allclose(s, cw * path, rtol=1e-12)


def test_restatement_beta_rule():
    assert R.beta_of(4, [0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0]) == 0.0
    assert R.beta_of(4, [0, 2], [1, 3], [1.0, 1.0]) == 1e-4
    with pytest.raises(ValueError):
        R.beta_of(4, [0, 1], [1, 2], [1.0, 1.0])


def test_restatement_logdet_identity_on_a_small_graph():
    rng = np.random.default_rng(11)
    n = 60
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    ci = rng.integers(0, n, 150); cj = rng.integers(0, n, 150); cw = rng.uniform(0.5, 2.0, 150)
    order, gains, _ = R.greedy(n, fi, fj, fw, ci, cj, cw, 40, fold=7)
    L0 = R.reduced_laplacian(n, fi, fj, fw)
    LK = R.reduced_laplacian(n, np.concatenate([fi, ci[order]]), np.concatenate([fj, cj[order]]), np.concatenate([fw, cw[order]]))
    growth = np.linalg.slogdet(LK)[1] - np.linalg.slogdet(L0)[1]
    assert abs(np.sum(np.log1p(gains)) - growth) <= 1e-11 * abs(growth)
