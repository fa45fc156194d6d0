"""GreedyEig, dense chain form against the matrix-free route (mac_amd/csrc/eig_free.h): one JSON line per route
and one per pair, both routes of a pair in this one process.

    python tools/eig_free_time.py [case ...]      cases: intel10 intel50 city20 (default: all three); intel_kept50 city_kept50

intel10 / intel50: subset(k) on the intel pose graph with k = 10 % / 50 % of the candidates.  city20: the first 20 picks of
city10000.  intel_kept50 / city_kept50 (the spanning-tree route, mac_amd/csrc/eig_free_tree.h, DESIGN section 22, against the dense
general form): the same graphs with their first 50 closures moved to the fixed list, k = 10 % of the remaining candidates / 20.
Per route: build_ms = wall time of the constructor, select_ms = wall time of subset(k), ms per pick, candidates solved
exactly and operator applications per solved candidate as GreedyEig.info() reports them.  Per pair: the speedup of the matrix-free
route, whether the picks are the same, and the largest difference of lambda_2 after a pick.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd.solvers import GreedyEig  # noqa: E402
from mac_amd.utils.graphs import Edge  # noqa: E402


def pose_graph(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{name}.npz"))
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(g["fi"], g["fj"], g["fw"])]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(g["ci"], g["cj"], g["cw"])]
    return int(g["n"]), fixed, cand


def one(case, n, fixed, cand, K, matrix_free):
    m = len(cand)
    t0 = time.perf_counter()
    ge = GreedyEig(fixed, cand, n, matrix_free=matrix_free)
    build_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sol, _ = ge.subset(K)
    select_ms = (time.perf_counter() - t0) * 1e3
    inf = ge.info()
    solved, apps = inf["solved"], inf["applications"]
    row = dict(case=case, route=inf["form"], n=n, m=m, picks=K, ld=inf["ld"], batch=inf["batch"], fold=inf["fold"],
               build_ms=round(build_ms, 2), select_ms=round(select_ms, 2), ms_per_pick=round(select_ms / K, 3),
               ms_first_pick=round(float(ge.last_times[0]) * 1e3, 3), ms_last_pick=round(float(ge.last_times[-1] - ge.last_times[-2]) * 1e3, 3),
               lambda2_last=float(ge.last_lambda2[-1]), solved_total=int(solved.sum()),
               solved_share=round(float(solved.sum() / (m * K - K * (K - 1) / 2)), 4), applications_total=int(apps.sum()),
               applications_per_solved=round(float(apps.sum() / solved.sum()), 2))
    print(json.dumps(row), flush=True)
    lam = ge.last_lambda2.copy()
    ge._dev.close()
    return row, np.nonzero(sol)[0], lam


def pair(case, name, k_of, kept=0):
    n, fixed, cand = pose_graph(name)
    fixed, cand = fixed + cand[:kept], cand[kept:]
    K = k_of(len(cand))
    d, sd, ld_ = one(case, n, fixed, cand, K, False)
    f, sf, lf = one(case, n, fixed, cand, K, "tree" if kept else True)
    print(json.dumps(dict(case=case, pair="dense / matrix_free", picks=K, history_over_ld=round((kept + K) / d["ld"], 3),
                          select_speedup=round(d["select_ms"] / f["select_ms"], 2), build_speedup=round(d["build_ms"] / f["build_ms"], 2),
                          same_picks=bool(np.array_equal(sd, sf)), max_lambda2_difference=float(np.max(np.abs(ld_ - lf))),
                          applications_per_solved=[d["applications_per_solved"], f["applications_per_solved"]])), flush=True)


if __name__ == "__main__":
    for mf in (False, True, "tree"):      # (HIP context and code objects of every route: not build_ms)
        GreedyEig([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3, matrix_free=mf).subset(1)
    for c in sys.argv[1:] or ["intel10", "intel50", "city20"]:
        if c == "intel10":
            pair(c, "intel", lambda m: int(0.1 * m))
        elif c == "intel50":
            pair(c, "intel", lambda m: int(0.5 * m))
        elif c == "city20":
            pair(c, "city10000", lambda m: 20)
        elif c == "intel_kept50":
            pair(c, "intel", lambda m: int(0.1 * m), kept=50)
        elif c == "city_kept50":
            pair(c, "city10000", lambda m: 20, kept=50)
        else:
            raise SystemExit(f"unknown case {c}")
