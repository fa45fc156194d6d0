"""GreedyESP's spanning-tree matrix-free route without a GPU: the C surface, the argument errors, the host construction
(machip_esp_tree_plan through _lib.host_esp_tree) against networkx / SciPy, and the NumPy restatement
(tests/esp_tree_restatement.py) against the dense restatement and against itself in two precisions."""
import ctypes as C
import inspect
import os
import re

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from conftest import ROOT
import esp_free_restatement as F
import esp_restatement as R
import esp_tree_restatement as T
from mac_amd import _lib


def random_general(n, extra, seed):
    """A random spanning tree plus `extra` more fixed edges (duplicates of links and self-loops may occur among them)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    par = [perm[rng.integers(0, k)] for k in range(1, n)]
    fi = np.concatenate([perm[1:], rng.integers(0, n, extra)])
    fj = np.concatenate([par, rng.integers(0, n, extra)])
    return fi, fj, rng.uniform(0.5, 2.0, len(fi))


# ---- the C surface ----
def test_header_and_library_carry_the_spanning_tree_flag():
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 11
    assert int(re.search(r"#define MACHIP_ESP_SPANNING_TREE (\d+)", hdr).group(1)) == 8 == _lib.ESP_SPANNING_TREE
    assert int(re.search(r"#define MACHIP_ESP_MATRIX_FREE (\d+)", hdr).group(1)) == 2 == _lib.ESP_MATRIX_FREE
    lib = _lib.load()
    assert lib.machip_version() >= 11
    for name in ("machip_esp_tree_plan", "machip_esp_seeds"):
        assert re.search(r"\b%s\(" % name, hdr) and hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_matrix_free_keeps_its_default_and_takes_tree():
    from mac_amd.solvers import GreedyESP
    for f in (GreedyESP.__init__, _lib.Esp.__init__):
        p = inspect.signature(f).parameters["matrix_free"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    with pytest.raises(ValueError, match="matrix_free"):
        _lib.Esp(3, [0, 1], [1, 2], [1.0, 1.0], [0], [2], [1.0], matrix_free="chain")      # (refused before a device is asked for)


def test_argument_errors_are_decided_before_a_device_is_needed():
    lib = _lib.load()
    i32, f64, p_i32, p_f64 = _lib.i32, _lib.f64, _lib.p_i32, _lib.p_f64
    TREE = _lib.ESP_MATRIX_FREE | _lib.ESP_SPANNING_TREE

    def create(fi, fj, fw, flags, n=4, fold=0):
        fi, fj, fw = i32(fi), i32(fj), f64(fw)
        ci, cj, cw = i32([0]), i32([3]), f64([1.0])
        h = C.c_void_p()
        st = lib.machip_esp_create(0, n, len(fw), p_i32(fi), p_i32(fj), p_f64(fw), 1, p_i32(ci), p_i32(cj), p_f64(cw), fold, flags,
                                   C.byref(h))
        if st == _lib.OK:
            lib.machip_esp_destroy(h)
        return st, _lib.last_error()

    star = ([0, 1, 1], [1, 2, 3], [1.0, 1.0, 1.0])
    st, msg = create(*star, _lib.ESP_SPANNING_TREE)                                   # flag 8 without flag 2
    assert st == _lib.BAD_ARG and "MACHIP_ESP_SPANNING_TREE" in msg and "MACHIP_ESP_MATRIX_FREE" in msg
    st, msg = create(*star, _lib.ESP_SPANNING_TREE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_SPANNING_TREE" in msg
    st, msg = create(*star, TREE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_DENSE_INVERSE" in msg
    st, msg = create(*star, TREE, fold=64)
    assert st == _lib.BAD_ARG and "fold" in msg
    st, msg = create([0, 2], [1, 3], [1.0, 1.0], TREE)                               # two components, every node has an edge
    assert st == _lib.BAD_ARG and "connected fixed graph" in msg
    st, msg = create([0, 1], [1, 2], [1.0, 1.0], TREE)                               # node 3 has no fixed edge at all
    assert st == _lib.BAD_ARG and "connected fixed graph" in msg
    st, msg = create([0, 1, 1, 3], [1, 2, 3, 1], [1.0, 1.0, 1.0, -1.0], TREE)        # the link 1-3 sums to 0
    assert st == _lib.BAD_ARG
    # the pins that do not move
    st, msg = create([0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0], 4)
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    st, msg = create([0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0], 16)
    assert st == _lib.BAD_ARG and "unknown flags" in msg
    st, msg = create(*star, _lib.ESP_MATRIX_FREE)
    assert st == _lib.BAD_ARG and "needs a chain" in msg
    # a well-formed request gets past the argument checks: without a device the answer is NO_DEVICE, not BAD_ARG
    st, msg = create(*star, TREE)
    assert st in (_lib.OK, _lib.NO_DEVICE), msg
    for flags in (TREE, _lib.ESP_SPANNING_TREE):
        h = C.c_void_p()
        fi = np.arange(3)
        st = lib.machip_eig_create(0, 4, 3, p_i32(i32(fi)), p_i32(i32(fi + 1)), p_f64(f64(np.ones(3))), 1, p_i32(i32([0])),
                                   p_i32(i32([3])), p_f64(f64([1.0])), 0, 0, flags, C.byref(h))
        assert st == _lib.BAD_ARG and "not available" in _lib.last_error() and not h.value


# ---- the host construction ----
def nx_bfs(n, fi, fj):
    """parent by networkx: its adjacency keeps insertion order, so neighbours come in order of first appearance."""
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for a, b in zip(fi.tolist(), fj.tolist()):
        if a != b:
            G.add_edge(a, b)
    parent = np.full(n, -1)
    for child, par in nx.bfs_predecessors(G, 0):
        parent[child] = par
    return parent


def check_plan(n, fi, fj, fw, H):
    """Everything host_esp_tree returns against what it must satisfy."""
    parent, Rr, pre, end = H["parent"], H["R"], H["pre"], H["end"]
    su, sv, sw = H["seeds"]
    assert np.array_equal(parent, nx_bfs(n, fi, fj))
    # merged links
    W = {}
    for a, b, w in zip(fi.tolist(), fj.tolist(), fw.tolist()):
        if a != b:
            W[(min(a, b), max(a, b))] = W.get((min(a, b), max(a, b)), 0.0) + w
    assert len(sw) == len(W) - (n - 1)
    tree = {(min(v, int(parent[v])), max(v, int(parent[v]))) for v in range(1, n)}
    seeds = [(min(a, b), max(a, b)) for a, b in zip(su.tolist(), sv.tolist())]
    first = [k for k in dict.fromkeys((min(a, b), max(a, b)) for a, b in zip(fi.tolist(), fj.tolist()) if a != b) if k not in tree]
    assert seeds == first                                                            # order of first appearance
    assert all(W[k] == w for k, w in zip(seeds, sw.tolist()))                        # summed in list order: equal bits
    # preorder intervals: a permutation, a child's interval inside its parent's, subtree sizes
    assert sorted(pre.tolist()) == list(range(n)) and pre[0] == 0 and end[0] == n - 1
    size = np.ones(n, dtype=np.int64)
    depth = np.zeros(n, dtype=np.int64)
    order = np.argsort(pre)
    for v in order[1:]:
        depth[v] = depth[parent[v]] + 1
    for v in order[::-1][:-1]:
        size[parent[v]] += size[v]
    assert np.array_equal(end, pre + size - 1)
    v = np.arange(1, n)
    assert np.all(pre[parent[v]] < pre[v]) and np.all(end[v] <= end[parent[v]])
    # R from sparse solves: R[v] = (M_T^-1)_vv
    wup = np.array([0.0] + [W[(min(x, int(parent[x])), max(x, int(parent[x])))] for x in range(1, n)])
    M = T.tree_laplacian(n, dict(parent=parent.astype(np.int64), w=wup))
    diag = np.array([splu(M).solve(np.eye(n - 1)[:, k])[k] for k in range(n - 1)]) if n <= 400 else None
    if diag is not None:
        assert np.allclose(Rr[1:], diag, rtol=1e-11, atol=0) and Rr[0] == 0.0
    return depth


def test_plan_on_a_random_tree_plus_extra_edges_matches_networkx_and_sparse_solves():
    for n, extra, seed in ((300, 150, 1), (257, 40, 2), (50, 0, 3)):
        fi, fj, fw = random_general(n, extra, seed)
        H = _lib.host_esp_tree(n, fi, fj, fw)
        check_plan(n, fi, fj, fw, H)
        P = T.plan(n, fi, fj, fw)                                   # the restatement's own construction: equal, bit for bit
        assert np.array_equal(H["parent"], P["parent"]) and np.array_equal(H["R"], P["R"])
        assert np.array_equal(H["pre"], P["pre"]) and np.array_equal(H["end"], P["end"])
        assert all(np.array_equal(a, b) for a, b in zip(H["seeds"], P["seeds"]))


def test_plan_on_a_chain_has_no_seeds_and_the_chain_routes_R_bits():
    rng = np.random.default_rng(7)
    n = 1000
    fi = np.arange(n - 1); fw = rng.uniform(0.5, 2.0, n - 1)
    # some links given twice and reversed: summed in list order, as the chain route sums them
    fi2 = np.concatenate([fi, fi[::7] + 1]); fj2 = np.concatenate([fi + 1, fi[::7]]); fw2 = np.concatenate([fw, rng.uniform(0.5, 2.0, len(fi[::7]))])
    for a, b, w in ((fi, fi + 1, fw), (fi2, fj2, fw2)):
        H = _lib.host_esp_tree(n, a, b, w)
        assert len(H["seeds"][2]) == 0
        assert np.array_equal(H["R"], F.chain_resistances(n, a, b, w))
        assert np.array_equal(H["parent"], np.arange(-1, n - 1)) and np.array_equal(H["pre"], np.arange(n))
        assert np.array_equal(H["end"], np.full(n, n - 1))


def test_plan_with_parallel_reversed_and_self_loop_fixed_edges():
    #        link 0-1 three times (one reversed), a self-loop at 2, 3-1 reversed, a cycle 1-2-3 -> one seed
    fi = np.array([0, 1, 2, 1, 0, 3, 2, 3, 4])
    fj = np.array([1, 0, 2, 2, 1, 1, 3, 4, 3])
    fw = np.array([1.0, 0.25, 9.0, 2.0, 0.5, 4.0, 8.0, 1.5, 0.5])
    H = _lib.host_esp_tree(5, fi, fj, fw)
    check_plan(5, fi, fj, fw, H)
    assert H["parent"].tolist() == [-1, 0, 1, 1, 3]
    assert H["R"].tolist() == [0.0, 1.0 / (1.0 + 0.25 + 0.5), 1.0 / 1.75 + 1.0 / 2.0, 1.0 / 1.75 + 1.0 / 4.0, 1.0 / 1.75 + 1.0 / 4.0 + 1.0 / (1.5 + 0.5)]
    su, sv, sw = H["seeds"]
    assert (su.tolist(), sv.tolist(), sw.tolist()) == ([2], [3], [8.0])
    with pytest.raises(AssertionError, match="BAD_ARG.*connected fixed graph"):
        _lib.host_esp_tree(5, fi[:7], fj[:7], fw[:7])                # node 4 unreachable
    with pytest.raises(AssertionError, match="BAD_ARG"):
        _lib.host_esp_tree(3, [0, 1, 2], [1, 2, 1], [1.0, 1.0, -1.0])      # the link 1-2 sums to 0


# ---- the restatement ----
def test_restatement_matches_the_dense_restatement_on_a_general_graph():
    n = 300
    fi, fj, fw = random_general(n, 150, 11)
    rng = np.random.default_rng(12)
    ci = np.concatenate([rng.integers(0, n, 400), [0, 0, 9]]); cj = np.concatenate([rng.integers(0, n, 400), [17, 200, 9]])
    cw = rng.uniform(0.5, 2.0, len(ci))
    K = 120
    od, gd, md = R.greedy(n, fi, fj, fw, ci, cj, cw, K)
    ot, gt, mt = T.greedy(n, fi, fj, fw, ci, cj, cw, K)
    ol, gl, _ = T.greedy(n, fi, fj, fw, ci, cj, cw, K, dtype=np.longdouble)
    assert md.min() > 1e-8
    assert np.array_equal(od, ot) and np.array_equal(od, ol)
    print("tree restatement vs dense restatement %.3g, float64 vs longdouble %.3g"
          % (np.max(np.abs(gt - gd) / gd), np.max(np.abs(gt - gl) / gl)))
    assert np.all(np.abs(gt - gd) <= 1e-9 * np.abs(gd)) and np.all(np.abs(gl - gd) <= 1e-9 * np.abs(gd))


def test_restatement_on_a_chain_matches_the_chain_restatement():
    rng = np.random.default_rng(5)
    n = 400
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    ci = rng.integers(0, n, 300); cj = rng.integers(0, n, 300); cw = rng.uniform(0.5, 2.0, 300)
    of, gf, _ = F.greedy(n, fi, fj, fw, ci, cj, cw, 100)
    # float64: the rows come from SuperLU solves against the chain's Laplacian, condition number about 4 n^2 w_max / (pi^2 w_min)
    # = 2.6e5 here, so eps x condition = 6e-11 and the bound is 100 times that; longdouble: the elimination on the tree has no such
    # factor and the bound is the float64 chain restatement's own error (1e-11, as tests/test_esp_free_host.py bounds it).
    for dt, tol in ((np.float64, 6e-9), (np.longdouble, 1e-11)):
        ot, gt, _ = T.greedy(n, fi, fj, fw, ci, cj, cw, 100, dtype=dt)
        print("%s: gains vs the chain restatement %.3g" % (dt.__name__, np.max(np.abs(gt - gf) / gf)))
        assert np.array_equal(of, ot) and np.all(np.abs(gt - gf) <= tol * np.abs(gf))
