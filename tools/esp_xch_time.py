"""Timing of the exchange on the log tree count (mac_amd/csrc/esp_exchange.h): one JSON line per run.

    python tools/esp_xch_time.py [case ...]      cases: intel sphere2500 city10000 (default: all)

Per pose graph, K = m // 3: the exchange from the greedy's own selection (run to convergence) and from NaiveGreedy's (the K heaviest
candidates) with max_swaps = 200.  Each is run twice: once plain (ms = device time of the call, ms_per_round over the rounds after
the load) and once with option esp_xch_profile = 1, which puts events between the phases: load (Sigma0 copy, K forced picks, T's
build), pairs (pair pass + final argmax), t_rows (T's rank-1 updates), steps (forced steps + score updates), folds.  rows = "lds" or
"global": where the pair pass reads its row of T from (option esp_xch_lds_kb; both are timed where the row fits the default 48 KiB).  The model counts
per round 8 K ld bytes of T for the pair pass, 28 m K bytes of candidate arrays through L2, and per swap 2 x 16 K ld bytes for T's
updates; greedy_ms is the yardstick: a fresh greedy run to the same K on the same handle.

    python tools/esp_xch_time.py --edge [case ...]      cases: intel_kept50 chain100k (default: both)

The exchange in edge space (mac_amd/csrc/esp_exchange_edge.h), the same two starts and the same phases, every
run repeated (rep = 0, 1, 2).  intel_kept50: intel with its first 50 closures kept as fixed edges (M = 785, ld = 832), and on the same
graph and starts the dense exchange (route = "dense", ld = 1 728).  chain100k: the 100 000-node chain with 4 000 candidates of
tools/esp_relax_time.py; greedy_ms is a fresh matrix-free greedy run to the same K, the only alternative there.  The model counts per
round 8 K ld bytes of T and 20 m K bytes of candidate arrays through L2, and per swap 2 x 16 K ld bytes for T's updates."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd import _lib  # noqa: E402
from mac_amd.solvers import GreedyESP, NaiveGreedy  # noqa: E402
from mac_amd.utils.graphs import Edge  # noqa: E402


def pose_graph(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{name}.npz"))
    return int(g["n"]), g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"]


def timed(esp, start, cap, profile, call="exchange"):
    with _lib.default_options(esp_xch_profile=1 if profile else None):
        return getattr(esp, call)(start, max_swaps=cap)[2]


def run(case):
    n, fi, fj, fw, ci, cj, cw = pose_graph(case)
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(fi, fj, fw)]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(ci, cj, cw)]
    m = len(cw)
    K = m // 3
    esp = GreedyESP(fixed, cand, n)
    ld = esp.info()["ld"]
    esp.subset(8)                                # (first launches of the greedy's kernels)
    greedy_sel = np.flatnonzero(esp.subset(K)[0])
    greedy_ms = float(esp._dev.select([K])[2][-1])
    starts = (("greedy", greedy_sel, 10 * K), ("naive", np.flatnonzero(NaiveGreedy(cand).subset(K)), 200))
    for rows in ("lds", "global"):
        if rows == "lds" and 8 * ld > 48 * 1024:      # (beyond the default budget the call reads global rows: city10000)
            continue
        with _lib.default_options(esp_xch_lds_kb=None if rows == "lds" else 0):
            esp.exchange(greedy_sel, max_swaps=1)      # (first launches of the exchange's kernels, T allocated)
            for tag, start, cap in starts:
                plain = timed(esp, start, cap, False)
                prof = timed(esp, start, cap, True)
                assert list(plain["out"]) == list(prof["out"]) and list(plain["in"]) == list(prof["in"])
                swaps = plain["swaps"]
                rounds = swaps + (1 if plain["converged"] else 0)
                load_ms, pairs_ms, trows_ms, steps_ms, folds_ms = (float(v) * 1e3 for v in prof["phase_seconds"])
                ms = plain["seconds"] * 1e3
                pair_bytes = 8 * K * ld + 28 * m * K
                trow_bytes = 2 * 16 * K * ld
                print(json.dumps(dict(
                    case=case, start=tag, rows=rows, n=n, m=m, K=K, ld=ld, pairs_per_round=K * (m - K), swaps=swaps,
                    converged=bool(plain["converged"]), growth=round(plain["growth"], 6), ms=round(ms, 3),
                    profiled_ms=round(prof["seconds"] * 1e3, 3), load_ms=round(load_ms, 3),
                    ms_per_round=round((ms - load_ms) / max(rounds, 1), 4),
                    pairs_ms_per_round=round(pairs_ms / max(rounds, 1), 4), t_rows_ms_per_swap=round(trows_ms / max(swaps, 1), 4),
                    steps_ms_per_swap=round(steps_ms / max(swaps, 1), 4), folds_ms=round(folds_ms, 3),
                    pair_bytes_model=pair_bytes, pair_model_tb_s=round(pair_bytes * rounds / max(pairs_ms, 1e-9) / 1e9, 3),
                    t_rows_bytes_model=trow_bytes, t_rows_model_tb_s=round(trow_bytes * swaps / max(trows_ms, 1e-9) / 1e9, 3),
                    greedy_ms=round(greedy_ms, 3))), flush=True)


def edge_graph(case):
    if case == "chain100k":                      # (the generator of tools/esp_relax_time.py)
        rng = np.random.default_rng(100)
        n, cands = 100000, 4000
        fi = np.arange(n - 1)
        return (n, fi, fi + 1, rng.uniform(0.5, 2.0, n - 1), rng.integers(0, n, cands), rng.integers(0, n, cands),
                rng.uniform(0.5, 2.0, cands)), True
    assert case == "intel_kept50", case
    n, fi, fj, fw, ci, cj, cw = pose_graph("intel")
    c = 50
    return (n, np.concatenate([fi, ci[:c]]), np.concatenate([fj, cj[:c]]), np.concatenate([fw, cw[:c]]), ci[c:], cj[c:], cw[c:]), "tree"


def run_edge(case, reps=3):
    from mac_amd.solvers import ESPRelaxation
    (n, fi, fj, fw, ci, cj, cw), space = edge_graph(case)
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(fi, fj, fw)]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(ci, cj, cw)]
    m = len(cw)
    K = m // 3
    relax = ESPRelaxation(fixed, cand, n, edge_space=space)
    greedy = GreedyESP(fixed, cand, n, matrix_free=space)
    greedy.subset(8)                             # (first launches of the greedy's kernels, the seeds)
    greedy_sel = np.flatnonzero(greedy.subset(K)[0])
    greedy_ms = [round(float(greedy._dev.select([K])[2][-1]), 3) for _ in range(reps)]
    starts = (("greedy", greedy_sel, 10 * K), ("naive", np.flatnonzero(NaiveGreedy(cand).subset(K)), 200))
    routes = [("edge", relax, "exchange_edge")]
    if case == "intel_kept50":
        routes.append(("dense", GreedyESP(fixed, cand, n), "exchange"))
    for route, esp, call in routes:
        getattr(esp, call)(greedy_sel, max_swaps=1)      # (first launches of the exchange's kernels, G built, T allocated)
        ld = esp.info()["relax_ld"] if route == "edge" else esp.info()["ld"]
        for tag, start, cap in starts:
            for rep in range(reps):
                plain = timed(esp, start, cap, False, call)
                prof = timed(esp, start, cap, True, call)
                assert list(plain["out"]) == list(prof["out"]) and list(plain["in"]) == list(prof["in"])
                swaps = plain["swaps"]
                rounds = swaps + (1 if plain["converged"] else 0)
                load_ms, pairs_ms, trows_ms, steps_ms, folds_ms = (float(v) * 1e3 for v in prof["phase_seconds"])
                ms = plain["seconds"] * 1e3
                pair_bytes = 8 * K * ld + (20 if route == "edge" else 28) * m * K
                trow_bytes = 2 * 16 * K * ld
                print(json.dumps(dict(
                    case=case, route=route, start=tag, rep=rep, n=n, m=m, K=K, ld=ld, pairs_per_round=K * (m - K), swaps=swaps,
                    converged=bool(plain["converged"]), growth=round(plain["growth"], 6), ms=round(ms, 3),
                    profiled_ms=round(prof["seconds"] * 1e3, 3), load_ms=round(load_ms, 3),
                    ms_per_round=round((ms - load_ms) / max(rounds, 1), 4),
                    pairs_ms_per_round=round(pairs_ms / max(rounds, 1), 4), t_rows_ms_per_swap=round(trows_ms / max(swaps, 1), 4),
                    steps_ms_per_swap=round(steps_ms / max(swaps, 1), 4), folds_ms=round(folds_ms, 3),
                    pair_bytes_model=pair_bytes, pair_model_tb_s=round(pair_bytes * rounds / max(pairs_ms, 1e-9) / 1e9, 3),
                    t_rows_bytes_model=trow_bytes, t_rows_model_tb_s=round(trow_bytes * swaps / max(trows_ms, 1e-9) / 1e9, 3),
                    greedy_ms=greedy_ms)), flush=True)


if __name__ == "__main__":
    GreedyESP([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3).subset(1)      # (HIP context and code objects)
    args = sys.argv[1:]
    if "--edge" in args:
        for c in [a for a in args if a != "--edge"] or ["intel_kept50", "chain100k"]:
            run_edge(c)
    else:
        for c in args or ["intel", "sphere2500", "city10000"]:
            run(c)
