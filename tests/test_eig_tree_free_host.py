"""GreedyEig's spanning-tree matrix-free route without a GPU: the C surface and the flag rules of machip_eig_create (all decided on
the host), the interval formula of mac_amd/csrc/eig_free_tree.h against the inverse of the tree's reduced Laplacian, and the
conditions under which tests/test_eig_tree_free_gpu.py can pin the new kernels through ``info()["applications"]``.

As in tests/test_eig_free_host.py the device test compares the applications per pick with those of the NumPy restatement under the
exact preconditioner, A_ref, and allows D / 4: D[k] the smallest excess of any damaged variant of tests/eig_tree_free_restatement.py
that can differ at pick k (a variant that runs into the 500-iteration cap counts as infinite).  Asserted here:
    the interval formula is inv(M_T) to 64 n eps relative (measured against numpy.linalg.solve), whatever the chunking, on the three
        inputs and on a 3 000-node tree of depth > 1 000; the Rt[lca] row differences equal the sweeps on indicator columns likewise
    D[k] >= 0.05 A_ref[k] at every pick of every case
    the route's own algebra with no term broken reproduces the exact run's picks with counts within D / 20; so does, for the first 5
        picks, the exact operator with the application perturbed by 1e-13 relative and every start vector by 1e-9."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import eig_lobpcg_restatement as Q
import eig_tree_free_restatement as T
import esp_tree_restatement as TR
from mac_amd import _lib
from mac_amd._lib import f64, i32, p_f64, p_i32

FREE = _lib.ESP_MATRIX_FREE | 64
TREE = FREE | 128
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(autouse=True, scope="module")
def one_blas_thread():
    """The restatement's matrices are 150 x 240 at the most: a BLAS thread pool only spends CPU time on them."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=1):
        yield


# ---- the C surface and the flag rules ----
def eig_create(fi, fj, fw, flags, fold=0, batch=0, n=None):
    lib = _lib.load()
    n = int(max(np.max(fi), np.max(fj))) + 1 if n is None else n
    h = C.c_void_p()
    st = lib.machip_eig_create(0, n, len(fw), p_i32(i32(fi)), p_i32(i32(fj)), p_f64(f64(fw)), 1, p_i32(i32([0])), p_i32(i32([n - 1])),
                               p_f64(f64([1.0])), fold, batch, flags, C.byref(h))
    msg = _lib.last_error()
    if h.value:
        lib.machip_eig_destroy(h)
    assert (st == _lib.OK) == bool(h.value)
    return st, msg


CHAIN = ([0, 1, 2], [1, 2, 3], [1.0, 2.0, 0.5])
STAR = ([0, 0, 0], [1, 2, 3], [1.0, 2.0, 0.5])
CYCLE = ([0, 1, 2, 3, 1], [1, 2, 3, 0, 3], [1.0, 2.0, 0.5, 0.25, 3.0])


def test_header_library_and_python_carry_the_flag_and_the_seed_count():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "machip.h")).read()
    assert "#define MACHIP_EIG_MATRIX_FREE_TREE 128" in hdr and _lib.EIG_MATRIX_FREE_TREE == 128
    assert int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1)) >= 17
    lib = _lib.load()
    assert re.search(r"\bint machip_eig_seeds\(machip_eig\* h, int64_t\* seeds_out\);", hdr)
    assert hasattr(lib, "machip_eig_seeds") and "machip_eig_seeds" in _lib.SIGNATURES
    r = C.c_int64(7)
    assert lib.machip_eig_seeds(None, C.byref(r)) == _lib.BAD_ARG and "NULL" in _lib.last_error() and r.value == 7
    from mac_amd.solvers import GreedyEig
    for f in (GreedyEig.__init__, _lib.Eig.__init__):
        p = inspect.signature(f).parameters["matrix_free"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_a_well_formed_request_passes_the_argument_checks():
    for fixed in (CHAIN, STAR, CYCLE, ([0, 1, 2, 1, 2], [1, 2, 3, 2, 2], [1.0, 2.0, 0.5, 0.25, 9.0])):      # (parallel links, a self-loop)
        st, msg = eig_create(*fixed, TREE)
        assert st in (_lib.OK, _lib.NO_DEVICE), msg


def test_new_refusals_name_the_flag_or_the_argument():
    st, msg = eig_create(*STAR, 128 | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_EIG_MATRIX_FREE_TREE" in msg
    st, msg = eig_create(*STAR, 128 | _lib.ESP_MATRIX_FREE)          # (without MACHIP_EIG_MATRIX_FREE: the pinned refusal of flag 2)
    assert st == _lib.BAD_ARG and msg == "GreedyEig solves against the dense inverse: MACHIP_ESP_MATRIX_FREE is not available here"
    st, msg = eig_create(*STAR, 128)
    assert st == _lib.BAD_ARG and "MACHIP_EIG_MATRIX_FREE_TREE" in msg and "MACHIP_ESP_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE_TREE" in msg
    st, msg = eig_create(*STAR, 128 | 64)
    assert st == _lib.BAD_ARG and "MACHIP_EIG_MATRIX_FREE_TREE" in msg
    st, msg = eig_create(*STAR, TREE | _lib.ESP_DENSE_INVERSE)
    assert st == _lib.BAD_ARG and "MACHIP_ESP_DENSE_INVERSE" in msg
    st, msg = eig_create(*STAR, TREE, fold=3)
    assert st == _lib.BAD_ARG and "fold" in msg
    for extra in (_lib.ESP_EDGE_RELAX, _lib.ESP_EDGE_RELAX_TREE, 256):
        st, msg = eig_create(*STAR, TREE | extra)
        assert st == _lib.BAD_ARG and "unknown flags" in msg
    st, msg = eig_create(*STAR, TREE, batch=5000)
    assert st == _lib.BAD_ARG and "batch" in msg
    # the spanning-tree plan's own refusals, with their messages
    st, msg = eig_create([0, 1], [1, 3], [1.0, 1.0], TREE)                       # node 2 has no fixed edge
    assert st == _lib.BAD_ARG and "spanning-tree route needs a connected fixed graph" in msg
    st, msg = eig_create([0, 1, 2, 1], [1, 2, 3, 2], [1.0, 2.0, 0.5, -2.0], TREE)  # the links between 1 and 2 sum to 0
    assert st == _lib.BAD_ARG and "positive link weights" in msg
    st, msg = eig_create([0, 1, 2, 1], [1, 2, 3, 2], [1.0, 2.0, 0.5, -3.0], TREE)  # ... to -1
    assert st == _lib.BAD_ARG and "positive link weights" in msg and "nodes 1 and 2" in msg


def test_a_callers_spanning_tree_flag_stays_refused_and_esp_create_does_not_know_the_new_flag():
    for flags in (_lib.ESP_SPANNING_TREE, _lib.ESP_SPANNING_TREE | 128, TREE | _lib.ESP_SPANNING_TREE, FREE | _lib.ESP_SPANNING_TREE):
        st, msg = eig_create(*STAR, flags)
        assert st == _lib.BAD_ARG and "not available" in msg, (flags, msg)
    st, msg = eig_create(*STAR, _lib.ESP_SPANNING_TREE | 128)
    assert msg == "GreedyEig solves against the dense inverse: MACHIP_ESP_SPANNING_TREE is not available here"
    lib = _lib.load()
    fi, fj, fw = STAR
    for flags in (128, TREE, _lib.ESP_MATRIX_FREE | _lib.ESP_SPANNING_TREE | 128):
        h = C.c_void_p()
        st = lib.machip_esp_create(0, 4, 3, p_i32(i32(fi)), p_i32(i32(fj)), p_f64(f64(fw)), 1, p_i32(i32([0])), p_i32(i32([3])),
                                   p_f64(f64([1.0])), 0, flags, C.byref(h))
        assert st == _lib.BAD_ARG and "unknown flags" in _lib.last_error() and not h.value


def test_python_refuses_before_a_device_is_asked_for(monkeypatch):
    from mac_amd.solvers import GreedyEig
    from mac_amd.utils.graphs import Edge
    monkeypatch.setattr(_lib, "require_device", lambda: pytest.fail("a device was asked for"))
    odom = [Edge(0, i + 1, 1.0) for i in range(3)]
    lc = [Edge(1, 3, 1.0)]
    for fold in (3, 16):
        with pytest.raises(ValueError, match="fold"):
            GreedyEig(odom, lc, 4, matrix_free="tree", fold=fold)
    with pytest.raises(ValueError, match="fold"):
        _lib.Eig(4, [0, 0, 0], [1, 2, 3], [1.0, 1.0, 1.0], [1], [3], [1.0], fold=16, matrix_free="tree")
    with pytest.raises(ValueError, match="dense_inverse"):
        GreedyEig(odom, lc, 4, matrix_free="tree", dense_inverse=True)
    with pytest.raises(ValueError, match="dense_inverse"):
        _lib.Eig(4, [0, 0, 0], [1, 2, 3], [1.0, 1.0, 1.0], [1], [3], [1.0], dense_inverse=True, matrix_free="tree")
    for bad in ("chain", "Tree", 1, 2, None, 1.0):
        with pytest.raises(ValueError, match="matrix_free"):
            GreedyEig(odom, lc, 4, matrix_free=bad)
        with pytest.raises(ValueError, match="matrix_free"):
            _lib.Eig(4, [0, 0, 0], [1, 2, 3], [1.0, 1.0, 1.0], [1], [3], [1.0], matrix_free=bad)


# ---- the interval formula ----
def deep_tree(n=3000, seed=11, back=3):
    """A random tree whose node k hangs below one of the `back` nodes before it: depth about n / 2."""
    rng = np.random.default_rng(seed)
    k = np.arange(1, n)
    par = np.maximum(k - rng.integers(1, back + 1, n - 1), 0)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])          # (node 0 stays the root; the labels below it are shuffled)
    return n, perm[k], perm[par], rng.uniform(0.5, 2.0, n - 1)


def formula_error(n, fi, fj, fw, rows, B=9):
    P = TR.plan(n, fi, fj, fw)
    Tb = T.tables(n, P)
    A = np.random.default_rng(5).standard_normal((n - 1, B))
    MT = TR.tree_laplacian(n, P).toarray()
    ref = np.linalg.solve(MT, A)
    got = T.sweep_apply(n, Tb, A, rows)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))), P, Tb, ref, A


@pytest.mark.parametrize("name,rows", [("general150", 32), ("general150", 7), ("general150", 192), ("deep150", 32), ("deep129", 32),
                                       ("deep129", 5)])
def test_interval_formula_is_the_inverse_of_the_reduced_tree(name, rows):
    n, fi, fj, fw = T.graph(name)[:4]
    err, P, Tb, ref, A = formula_error(n, fi, fj, fw, rows)
    print(name, rows, "relative error", err, "bound", 64 * n * EPS)
    assert err <= 64 * n * EPS
    for d in ("sub_end", "no_close", "down_carry", "up_carry"):          # each damage is one
        lost = T.sweep_apply(n, Tb, A, 32, damage=d)
        assert np.max(np.abs(lost - ref)) > 1e-3 * np.max(np.abs(ref)), d


def test_interval_formula_on_a_tree_of_depth_over_1000():
    n, fi, fj, fw = deep_tree()
    err, P, Tb, ref, A = formula_error(n, fi, fj, fw, 32, B=5)
    depth = np.zeros(n, dtype=np.int64)
    for x in P["order"][1:]:
        depth[x] = depth[P["parent"][x]] + 1
    print("deep tree: depth", int(depth.max()), "relative error", err, "bound", 64 * n * EPS)
    assert depth.max() > 1000 and len(P["seeds"][2]) == 0
    assert err <= 64 * n * EPS


@pytest.mark.parametrize("name", T.NAMES)
def test_tree_row_differences_are_the_sweeps_on_indicator_columns(name):
    g = T.graph(name)
    n, ci, cj = g[0], np.asarray(g[4]), np.asarray(g[5])
    M = T.TreeFree(g)
    S0 = TR.Sigma0(n, M.P, np.float64)
    es = np.arange(0, len(ci), 7)
    want = np.stack([S0.row(int(ci[e]), int(cj[e]))[1:] for e in es], axis=1)
    got = T.sweep_apply(n, M.Tb, Q.incidence(n, ci[es], cj[es]), T.ROWS)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(name, "row differences: relative error", err)
    assert err <= 64 * n * EPS


def test_the_inputs_are_what_the_cases_need():
    facts = {name: T.model_facts(name) for name in T.NAMES}
    print(facts)
    assert facts["general150"][:2] == (74, 8) and T.ld_of("general150") == 192
    assert facts["deep150"][:2] == (5, 38) and facts["deep129"][:2] == (5, 44)
    assert T.ld_of("deep129") == 128 == T.graph("deep129")[0] - 1
    assert len(T.graph("deep150")[6]) == 236 and len(T.graph("deep129")[6]) == 180
    assert {(5 + k) % 4 for k in range(Q.K_PICKS)} == {0, 1, 2, 3}


# ---- the inputs discriminate ----
def _show(tag, ref):
    print(tag, "A_ref", ref["A"].astype(int).tolist(), "D", ref["D"].tolist(), "min D / A_ref", float(np.min(ref["D"] / ref["A"])))
    for d, ex in ref["excess"].items():
        print("   ", d, "smallest excess / A_ref", float(np.nanmin(ex / ref["A"])))


@pytest.mark.parametrize("name,K,batch", T.CASES)
def test_every_broken_term_costs_at_least_a_twentieth_of_the_exact_count(name, K, batch):
    ref = T.reference(name, K, batch)
    _show(f"{name} K {K} batch {batch}:", ref)
    assert len(ref["D"]) == K and np.all(np.isfinite(ref["D"])) and np.all(ref["D"] >= 0.05 * ref["A"])
    assert len(set(ref["run"]["order"].tolist())) == K
    want = {"sub_end", "no_close", "down_carry", "up_carry", "no_seeds", "no_cand", "no_pending", "history_tail", "slice_lost"}
    assert set(ref["excess"]) == want | ({"history_block"} if name == "general150" else set())
    # what the device module reads: the recorded run is this one (counts to the noise allowance: another BLAS may move one by a few)
    rec = T.recorded(name, K, batch)
    assert np.array_equal(rec["order"], ref["run"]["order"]) and np.array_equal(rec["solved"], ref["run"]["solved"])
    assert np.all(np.abs(rec["A"] - ref["A"]) <= rec["D"] / 20) and np.all(np.abs(rec["D"] - ref["D"]) <= rec["D"] / 20)
    assert np.all(rec["D"] >= 0.05 * rec["A"])


@pytest.mark.parametrize("name,K,batch", T.CASES)
def test_rounding_size_noise_moves_the_counts_by_far_less(name, K, batch):
    g = T.graph(name)
    run = T.exact(name, K, batch)
    D = T.reference(name, K, batch)["D"]
    runs = {"noise": Q.select(g, min(K, 5), batch=batch, apply_noise=1e-13, start_noise=1e-9, seed=1),
            "route's algebra": Q.select(g, K, batch=batch, M=T.TreeFree(g)),
            "padding rows carried": Q.select(g, min(K, 5), batch=batch, M=T.TreeFree(g, "pad_rows"))}
    r = T.model_facts(name)[0]
    assert np.array_equal(runs["route's algebra"]["pending"], r + np.arange(K))
    for tag, rr in runs.items():
        k = len(rr["order"])
        dev = rr["applications"] - run["applications"][:k]
        print(f"{name} batch {batch} {tag}: largest |deviation| {int(np.max(np.abs(dev)))}, smallest D / 20 {float(np.min(D / 20))}")
        assert np.array_equal(rr["order"], run["order"][:k]) and np.array_equal(rr["solved"], run["solved"][:k])
        assert np.all(np.abs(dev) <= D[:k] / 20)
