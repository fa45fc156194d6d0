"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol include/machip.h
declares, host logic (tridiagonal analysis, rounding, FW driver, Laplacian builders), and the
product refuses to run without a device (no silent fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from mac_amd import _lib
from mac_amd.optimization import constraints, frankwolfe
from mac_amd.utils import graphs, rounding
from mac_amd.utils.fiedler import UnknownFiedlerMethod, find_fiedler_pair


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "machip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(machip_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"libmachip.so does not export {s}"
        assert s in _lib.SIGNATURES, f"ctypes binding lacks {s}"
    assert set(_lib.SIGNATURES) == set(syms)
    hdr = open(os.path.join(ROOT, "include", "machip.h")).read()
    assert lib.machip_version() == int(re.search(r"#define MACHIP_ABI_VERSION (\d+)", hdr).group(1))
    assert C.sizeof(_lib.SolveStats) == lib.machip_sizeof_stats()


def test_no_silent_cpu_fallback():
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    from mac_amd.solvers import MAC
    g = load_golden("petersen_solve_k3")
    fixed = [graphs.Edge(int(a), int(b), float(w)) for a, b, w in zip(g["fi"], g["fj"], g["fw"])]
    cand = [graphs.Edge(int(a), int(b), float(w)) for a, b, w in zip(g["ci"], g["cj"], g["cw"])]
    with pytest.raises(_lib.MachipError):
        MAC(fixed, cand, 10)
    L = graphs.weight_graph_lap_from_edge_list(fixed + cand, 10)
    with pytest.raises(_lib.MachipError):
        find_fiedler_pair(L)


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "mac_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M) and "oracle." not in src, f"{f} uses the oracle"


@pytest.mark.parametrize("J", [1, 2, 3, 17, 200, 1500])
def test_tridiag_smallest(J):
    rng = np.random.default_rng(J)
    a = rng.random(J) * 5 + 1
    b = np.zeros(J)
    b[1:] = rng.random(J - 1) * 2
    T = np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)
    w, V = np.linalg.eigh(T)
    th, s = _lib.host_tridiag_smallest(a, b)
    assert abs(th - w[0]) <= 1e-13 * abs(w).max()
    assert 1 - abs(s @ V[:, 0]) < 1e-10


def test_tridiag_clustered():
    # Lanczos-like T with a ghost (two nearly equal small eigenvalues)
    a = np.array([1.0, 3.0, 1.0 + 1e-9, 4.0, 2.0])
    b = np.array([0.0, 1e-7, 1e-7, 0.5, 0.3])
    T = np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)
    th, s = _lib.host_tridiag_smallest(a, b)
    assert abs(th - np.linalg.eigvalsh(T)[0]) < 1e-13


def test_laplacian_builders_match_reference_golden():
    g = load_golden("laplacian_petersen_weighted")        # reference tests/utils/test_graphs.py:27-50
    edges = [graphs.Edge(int(a), int(b), float(w)) for a, b, w in zip(g["ei"], g["ej"], g["ew"])]
    L1 = graphs.weight_graph_lap_from_edge_list(edges, 10)
    L2 = graphs.weight_graph_lap_from_edges(np.stack([g["ei"], g["ej"]], 1), g["ew"], 10)
    assert np.array_equal(L1.toarray(), g["L_dense"]) and np.array_equal(L2.toarray(), g["L_dense"])
    assert graphs.weight_reduced_graph_lap_from_edge_list(edges, 10).shape == (9, 9)


def test_frank_wolfe_driver_toy_problems():
    g = load_golden("fw_toy")                              # reference tests/optimization/test_frankwolfe.py
    x, u = frankwolfe.frank_wolfe(np.ones(3) * 0.7, lambda z: (-float(z @ z), -2.0 * z),
                                  constraints.solve_box_lp, maxiter=200)
    assert np.array_equal(x, g["x_box"]) and np.allclose(x, 0, atol=1e-2)
    x2, u2 = frankwolfe.frank_wolfe(np.array([1.0, 0.0]),
                                    lambda z: (-float((z - 0.5) @ (z - 0.5)), -2.0 * (z - 0.5)),
                                    lambda gr: constraints.solve_subset_box_lp(gr, 1), maxiter=300)
    assert np.array_equal(x2, g["x_subset"]) and np.allclose(x2, [0.5, 0.5], atol=0.01)
    # f ~ 0 at the start must not divide by zero (test_frankwolfe.py:54-73)
    x3, _ = frankwolfe.frank_wolfe(np.zeros(2), lambda z: (-float(z @ z), -2.0 * z),
                                   constraints.solve_box_lp, maxiter=5)
    assert np.all(np.isfinite(x3))


def test_rounding_matches_reference_golden():
    g = load_golden("rounding")
    k = int(g["k"])
    assert np.array_equal(rounding.round_nearest(g["w"], k, g["weights"], 10), g["nearest_tb"])

    class U:
        def rand(self):
            return float(g["madow_u"])
    assert np.array_equal(rounding.round_madow_base(g["madow_in"], k, U()), g["madow"])
    assert rounding.round_nearest(np.arange(5.0), 0).sum() == 0
    assert rounding.round_nearest(np.arange(5.0), 2).tolist() == [0, 0, 0, 1, 1]
    for nm in ["intel", "sphere2500"]:
        gg = load_golden("g2o_" + nm)

        class U2:
            def rand(self, gg=gg):
                return float(gg["madow_u"])
        assert np.array_equal(rounding.round_madow_base(gg["unrounded"], int(gg["k"]), U2()), gg["madow"])
        assert np.array_equal(rounding.round_nearest(gg["unrounded"], int(gg["k"]), gg["cw"], 10), gg["rounded"])


def test_unknown_method_raises_like_reference():
    import scipy.sparse as sp
    with pytest.raises(UnknownFiedlerMethod):
        find_fiedler_pair(sp.identity(4, format="csr"), method="bogus")


def test_method_strings_map_to_solver_modes():
    """fiedler_method -> machip_set_solver mode: the reference's direct-solver flavours and 'hip' pick
    automatically, 'tracemin_pcg' (the reference's preconditioned flavour, nx:22-76) asks for the
    preconditioned mode, the explicit 'hip_*' names force one."""
    from mac_amd.utils.fiedler import solver_mode, UnknownFiedlerMethod
    assert solver_mode("hip") == 0 and solver_mode("tracemin_lu") == 0 and solver_mode("tracemin_cholesky") == 0
    assert solver_mode("hip_lanczos") == 1
    assert solver_mode("tracemin_pcg") == 2 and solver_mode("hip_lobpcg") == 2
    with pytest.raises(UnknownFiedlerMethod):
        solver_mode("lobpcg")


@pytest.mark.parametrize("nm", ["intel", "sphere2500", "city10000", "kitti_05", "kitti_02", "ais2klinik"])
def test_g2o_reader_matches_reference_golden(nm):
    """Edge arrays produced by the reference's own reader (examples/pose_graph_utils.py) were
    captured in tests/golden/g2o_*.npz; the product parser must reproduce them."""
    from mac_amd.utils import g2o
    g = load_golden("g2o_" + nm)
    i, j, kap, n = g2o.read_g2o_edges(os.path.join(ROOT, "tests", "golden", "data", nm + ".g2o"))
    fixed = g2o.split_chain(i, j)
    assert n == int(g["n"])
    assert np.array_equal(i[fixed], g["fi"]) and np.array_equal(j[fixed], g["fj"])
    assert np.array_equal(i[~fixed], g["ci"]) and np.array_equal(j[~fixed], g["cj"])
    assert np.allclose(kap[fixed], g["fw"], rtol=1e-13, atol=0)
    assert np.allclose(kap[~fixed], g["cw"], rtol=1e-13, atol=0)
    if nm == "intel":
        edges, n2 = g2o.read_g2o_file(os.path.join(ROOT, "tests", "golden", "data", nm + ".g2o"))
        chain, loops = g2o.split_edges(edges)
        assert n2 == n and len(chain) == 1727 and len(loops) == 785


def test_graft_entry_build_runs():
    """The driver's build check: __graft_entry__.build() compiles libmachip.so for gfx950 and verifies the ABI version
    and exports (it once asserted a stale version number and would have failed the round's build check)."""
    import importlib
    ge = importlib.import_module("__graft_entry__")
    ge.build()


def test_bench_refuses_to_launch_ranks_without_devices():
    """bench.py --gpus 2 on a box with fewer than two GPUs (here: none) must refuse loudly instead of printing a line."""
    import subprocess
    import sys
    if _lib.device_count() >= 2:
        pytest.skip("two GPUs present")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "MACHIP_SHARE_GPU")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c3"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout) and '"metric"' not in r.stdout


@pytest.mark.parametrize("n,p,seed", [(3000, 0.01, 0), (6000, 0.002, 1), (300, 0.05, 3), (40, 0.6, 7)])
def test_bench_er_edges_are_networkx_fast_gnp_random_graph(n, p, seed):
    """bench.gnp_edges replays nx.fast_gnp_random_graph(n, p, seed) without building the graph: the same edges in G.edges() order."""
    import networkx as nx
    import bench
    i, j = bench.gnp_edges(n, p, seed)
    e = np.array([(min(a, b), max(a, b)) for a, b in nx.fast_gnp_random_graph(n, p, seed=seed).edges()], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(i, e[:, 0]) and np.array_equal(j, e[:, 1])


def test_bench_dump_outputs_writes_float64_within_the_size_cap(tmp_path):
    """bench.py --dump-outputs: float64 .npy files; an array above DUMP_MAX_ENTRIES becomes the same fixed sample every time."""
    import bench
    big = np.arange(bench.DUMP_MAX_ENTRIES + 5, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"f": np.array([1.5, 2.5]), "iters": np.array([3, 4], dtype=np.int32), "x": big})
    f, it, x = (np.load(tmp_path / "a" / (nm + ".npy")) for nm in ("f", "iters", "x"))
    assert f.dtype == it.dtype == x.dtype == np.float64 and list(it) == [3.0, 4.0]
    assert x.size == bench.DUMP_MAX_ENTRIES and np.all(np.diff(x) > 0) and np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))


def test_panel_plan_covers_every_row_and_column_within_the_kernel_limits():
    """Shape arithmetic of the column-panel Lanczos step (solver.h plan_panel, exported as machip_panel_plan; host only):
    the panels cover every column, the row blocks every row, a panel fits the LDS next to the row block's image
    (record form: RPT <= 13 records per worker thread; shifted recurrence, panel_u.h: an even panel width within what the chosen
    k_pan_mul8<LPT, TWT> instantiation holds), a worker wave owns at most 8 tiles, and the automatic rule turns the step on
    only for large, dense-enough matrices with rows the build kernels can describe (a hub row of up to 64 x 127 entries is
    admitted subject to the build's per-panel check, test_gpu_parity's hub cases)."""
    import ctypes as C
    lib = _lib.load()
    out = (C.c_int * 12)()
    with _lib.default_options(panel=None, panel_np=None, panel_nb=None, panel_u=None):
        # automatic rule (BASELINE configs[3]: on for the dense iterates only)
        for n, nnz, maxlen, want in ((100000, 700344, 30, 0), (100000, 1747218, 40, 1), (100000, 4044528, 70, 1), (100000, 4044528, 200, 1), (100000, 4044528, 9000, 0),
                                     (10000, 956618, 120, 0), (1728, 5496, 9, 0), (65536, 65536 * 20, 60, 1), (500000, 500000 * 30, 60, 0)):
            assert lib.machip_panel_plan(n, nnz, maxlen, out) == _lib.OK
            assert out[0] == want, (n, nnz, maxlen, list(out))
        assert list(out)[:1] == [0]
        lib.machip_panel_plan(100000, 2700000, 60, out)
        assert list(out)[:6] == [1, 6, 16668, 42, 38, 3] and list(out)[8:12] == [1, 9, 3, 1]      # the shape profiles/r6_panel_u.md measures
        with _lib.default_options(panel_u=0):
            lib.machip_panel_plan(100000, 2700000, 60, out)
            assert list(out)[:7] == [1, 12, 8334, 21, 75, 5, 9] and out[8] == 0       # the record form's (profiles/r3_c4_panel.md)
        with _lib.default_options(stream=0):           # (no step-by-step records, no drift monitor: record form)
            lib.machip_panel_plan(100000, 2700000, 60, out)
            assert list(out)[:3] == [1, 12, 8334] and out[8] == 0
        rng = np.random.default_rng(3)
        for n in [128, 129, 300, 2000, 8448, 8449, 65536, 100000, 123457, 399999, 1000003] + [int(t) for t in rng.integers(130, 3000000, 40)]:
            for extra in ({}, {"panel_np": int(rng.integers(1, 40))}, {"panel_nb": int(rng.integers(1, 400))}, {"panel_u": 0},
                          {"panel_u": 0, "panel_np": int(rng.integers(1, 40))}):
                with _lib.default_options(panel=1, **extra):          # (process defaults: what machip_panel_plan plans under)
                    assert lib.machip_panel_plan(n, 20 * n, 60, out) == _lib.OK
                on, NP, Cc, NB, NTB, TWW, RPT, g2, u, LPT, TWT, cells = list(out)
                if not on:
                    continue
                assert NP >= 1 and NP * Cc >= n and (NP - 1) * Cc < n          # every column in exactly one panel, none empty
                assert NB * NTB * 64 >= n and (NB - 1) * NTB * 64 < n          # every row in exactly one block, none empty
                if u:       # k_pan_mul8<LPT, TWT>: operand panel + row-block image within 160 KB of LDS, 16-byte loads on even columns
                    assert extra.get("panel_u") != 0 and cells == 1 and Cc % 2 == 0
                    assert TWT in (3, 5, 8) and TWW <= TWT and 1 <= LPT <= (9 if TWT == 3 else 8)
                    assert Cc <= min(1920 * LPT, ((163840 - 8 * 960 * TWT - 256) // 8) & ~1)
                else:
                    assert 1 <= RPT <= 13 and RPT * 960 >= Cc                  # the panel fits LDS / registers
                assert 1 <= TWW <= 8 and TWW * 15 >= NTB and NTB <= 120        # a worker wave's tiles
                assert 1 <= g2 <= 1024
        assert lib.machip_panel_plan(0, 0, 0, out) == _lib.BAD_ARG


def test_option_table_roundtrip_and_environment_is_read_once():
    """machip_set_option / machip_get_option (round 5: the MACHIP_* environment knobs of rounds 1-4 became a per-handle table):
    every name the library lists is settable as a process default, unknown names are BAD_ARG, MACHIP_OPTION_AUTO restores the
    default, and the environment is consulted ONCE, when the library is first used -- later changes of os.environ do nothing."""
    import ctypes as C
    import subprocess
    import sys
    lib = _lib.load()
    names = _lib.option_names()
    assert len(names) >= 40 and "panel" in names and "chunk" in names and len(set(names)) == len(names)
    v = C.c_int64(0)
    for nm in names:
        assert lib.machip_get_option(None, nm.encode(), C.byref(v)) == _lib.OK
        old = v.value
        assert lib.machip_set_option(None, nm.encode(), 7) == _lib.OK
        assert lib.machip_get_option(None, nm.encode(), C.byref(v)) == _lib.OK and v.value == 7
        assert lib.machip_set_option(None, nm.encode(), old) == _lib.OK
    assert lib.machip_set_option(None, b"no_such_option", 1) == _lib.BAD_ARG
    assert lib.machip_get_option(None, b"panel", None) == _lib.BAD_ARG
    code = ("import os, sys; sys.path.insert(0, %r)\n"
            "from mac_amd import _lib\n"
            "import ctypes as C\n"
            "lib = _lib.load(); v = C.c_int64(0)\n"
            "lib.machip_get_option(None, b'chunk', C.byref(v)); a = v.value\n"
            "os.environ['MACHIP_CHUNK'] = '48'; os.environ['MACHIP_PANEL'] = '1'\n"
            "lib.machip_get_option(None, b'chunk', C.byref(v)); b = v.value\n"
            "lib.machip_get_option(None, b'panel', C.byref(v)); c = v.value\n"
            "print(a, b, c == _lib.OPTION_AUTO)\n") % ROOT
    env = {k: v_ for k, v_ in os.environ.items() if not k.startswith("MACHIP_")}
    env["MACHIP_CHUNK"] = "16"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.split() == ["16", "16", "True"], r.stdout


def test_loading_the_library_leaves_the_process_environment_alone():
    """Round 3 set GPU_MAX_HW_QUEUES=16 when the library was loaded (a hardware queue per evaluation lane); VERDICT r3 item 7 /
    ADVICE: a drop-in must not mutate the host's environment.  The lanes' streams now get their own hardware queue by being
    created with a CU mask (machip.hip, create_lane_stream; measured: profiles/r4_lane_queues.txt), so importing the binding
    and loading libmachip.so must leave the variable exactly as the application set it -- or unset."""
    import subprocess
    import sys
    code = "import os, sys; sys.path.insert(0, '.'); from mac_amd import _lib; _lib.load(); print(os.environ.get('GPU_MAX_HW_QUEUES'))"
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "None", (out.stdout, out.stderr[-500:])
    env["GPU_MAX_HW_QUEUES"] = "6"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "6", out.stderr[-500:]
    hip_src = open(os.path.join(ROOT, "mac_amd", "csrc", "machip.hip")).read()
    assert "setenv(" not in hip_src and "putenv" not in hip_src
    assert "GPU_MAX_HW_QUEUES" not in open(os.path.join(ROOT, "mac_amd", "_lib.py")).read()


def test_fiedler_csr_rejects_malformed_row_pointers_before_touching_the_matrix():
    """machip_fiedler_csr takes arbitrary caller matrices (the bare find_fiedler_pair(L) surface, mac/utils/fiedler.py:9-44): the
    row pointers are validated as a whole on the host before anything is read through them and before the first device call
    (`indptr = [0, 100, 5]` used to walk 100 entries of a 5-entry array).  BAD_ARG on any machine."""
    import pytest
    from mac_amd import _lib
    idx = np.zeros(5, dtype=np.int32); dat = np.ones(5)
    # (BAD_ARG surfaces as AssertionError in the binding: the reference asserts on bad sizes, mac/utils/fiedler.py:35-36)
    for indptr, what in [([0, 100, 5], "monotone"), ([1, 2, 3], "indptr[0]"), ([0, 2, -1], "indptr")]:
        with pytest.raises(AssertionError) as e:
            _lib.fiedler_csr(np.array(indptr, dtype=np.int32), idx, dat, 2)
        assert "BAD_ARG" in str(e.value) and what in str(e.value), str(e.value)
    with pytest.raises(AssertionError) as e:          # column out of range: also found on the host
        _lib.fiedler_csr(np.array([0, 2, 4], dtype=np.int32), np.array([0, 7, 0, 1], dtype=np.int32), np.ones(4), 2)
    assert "BAD_ARG" in str(e.value) and "column" in str(e.value)


def test_rccl_first_contact_watchdog_turns_a_stall_into_an_error():
    """The watchdog that guards ncclCommInitRank and a communicator's first ncclAllGather (machip.hip, run_with_watchdog),
    exercised with a sleeping stand-in: work that finishes inside the limit returns OK, work that does not comes back as
    MACHIP_RCCL_ERROR after the limit -- not after the work -- with a message that says what stalled."""
    import time
    lib = _lib.load()
    assert lib.machip_selftest_watchdog(20, 2000) == _lib.OK
    t0 = time.perf_counter()
    st = lib.machip_selftest_watchdog(3000, 200)
    el = time.perf_counter() - t0
    assert st == _lib.RCCL_ERROR and el < 1.5, (st, el)
    msg = _lib.last_error()
    assert "did not return within" in msg and "peer rank is missing" in msg


import scipy.sparse as sp  # noqa: E402


def _lanczos_records(L, u0, J):
    """Plain Lanczos on L restricted to the complement of the constant vector, in the conventions of the device records
    (kernels.h): beta_0 = ||u0 - mean||, v_0 = u0 / beta_0, beta_j couples v_{j-1} and v_j, l1_j = ||v_j||_1."""
    n = L.shape[0]
    alpha, beta, l1 = np.zeros(J), np.zeros(J + 1), np.zeros(J)
    u = u0 - u0.mean()
    vprev = np.zeros(n)
    for j in range(J + 1):
        beta[j] = np.linalg.norm(u)
        if j == J or beta[j] < 1e-13:
            break
        v = u / beta[j]
        l1[j] = np.abs(v).sum()
        w = L @ v
        w -= w.mean()
        alpha[j] = v @ w
        u = w - alpha[j] * v - beta[j] * vprev
        vprev = v
    return alpha, beta, l1


def _estimates(alpha, beta, l1, J):
    """est_a = beta_a |s_a| ||v_{a-1}||_1 for a = 1..J with LAPACK's eigenvectors (the quantity follow.h tracks)."""
    out = np.full(J + 1, np.inf)
    for a in range(1, J + 1):
        T = np.diag(alpha[:a]) + np.diag(beta[1:a], 1) + np.diag(beta[1:a], -1)
        w, V = np.linalg.eigh(T)
        out[a] = beta[a] * abs(V[a - 1, 0]) * l1[a - 1]
    return out


def test_record_follower_ends_a_sequence_on_the_records_alone():
    """Round 5, streamed records (mac_amd/csrc/follow.h through machip_host_follow_records): the analysis points are strictly
    increasing, at most a chunk apart, every point before the last has its estimate above the target and the last one below
    (estimates recomputed here with LAPACK); the last point is the first crossing (to within two steps); records beyond it do not
    matter, fewer records give a prefix of the same points; a breakdown ends the sequence where it happens; a constant start
    vector is refused.  (Estimates, breakdown and refusal are Follower::ingest, which the chunk-granular loop of solver_lanczos.h
    reads its records through as well.)"""
    rng = np.random.default_rng(3)
    n = 600
    a = rng.integers(0, n, 6 * n); b = rng.integers(0, n, 6 * n)
    keep = a != b
    W = sp.coo_matrix((rng.uniform(0.5, 1.5, keep.sum()), (a[keep], b[keep])), shape=(n, n))
    W = W + W.T + sp.diags(np.ones(n - 1), 1) + sp.diags(np.ones(n - 1), -1)
    L = (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    lnorm = abs(L).sum(axis=1).max()
    J = 160
    alpha, beta, l1 = _lanczos_records(L, rng.standard_normal(n), J)
    est = _estimates(alpha, beta, l1, J)
    target = 0.95e-8 * lnorm
    crossing = int(np.argmax(est < target))
    assert 40 < crossing < J - 10, crossing                      # (the test matrix converges well inside the record array)
    pts, jeff, e_last = _lib.host_follow_records(alpha, beta, l1, n, target, lnorm)
    assert pts == sorted(set(pts)) and pts[0] == 16 and pts[-1] == jeff
    assert max(np.diff(pts)) <= 32 and all(d <= 16 for p, d in zip(pts, np.diff(pts)) if p < 64)
    assert all(est[p] >= target for p in pts[:-1]) and est[jeff] < target
    assert abs(e_last - est[jeff]) <= 1e-6 * est[jeff]
    assert 0 <= jeff - crossing <= 2, (jeff, crossing)
    assert np.diff(pts)[-1] <= 8                                  # (the points close in on the crossing: a third of the forecast distance at a time)
    # records beyond the final point do not matter; fewer records: a prefix, no end yet
    for Jc in (jeff, jeff + 1, jeff + 7):
        assert _lib.host_follow_records(alpha, beta, l1, n, target, lnorm, J=Jc)[:2] == (pts, jeff)
    for Jc in (20, 47, jeff - 1):
        p2, j2, _ = _lib.host_follow_records(alpha, beta, l1, n, target, lnorm, J=Jc)
        assert j2 == -1 and p2 == [p for p in pts if p <= Jc]
    # a looser target ends earlier on a prefix of the same early points
    p3, j3, _ = _lib.host_follow_records(alpha, beta, l1, n, 1e-4 * lnorm, lnorm)
    assert j3 < jeff and est[j3] < 1e-4 * lnorm and p3[:2] == pts[:2]
    # basis capacity: the last point is the (even) cap
    p4, j4, _ = _lib.host_follow_records(alpha, beta, l1, n, target, lnorm, jcap=50)
    assert j4 == -1 and p4[-1] == 50
    # breakdown: on the complete graph the Krylov space of any start vector (orthogonal to 1) has dimension 1
    K = n * np.eye(8) - np.ones((8, 8))
    ak, bk, lk = _lanczos_records(K[:8, :8] * 1.0, np.arange(8.0), 20)
    pk, jk, _ = _lib.host_follow_records(ak, bk, lk, 8, 1e-8, 8.0, J=16)
    assert jk == 1 and pk == [16]
    with pytest.raises(AssertionError, match="start vector"):          # (BAD_ARG surfaces as the reference's assert does)
        _lib.host_follow_records(np.ones(20), np.zeros(21), np.ones(20), 8, 1e-8, 1.0)
