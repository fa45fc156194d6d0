"""GreedyEig timing (mac_amd/csrc/eig.h): one JSON line per case.

    python tools/eig_time.py [case ...]      cases: intel10 intel50 city20 python10 (default: intel10 intel50 python10)

intel10 / intel50: subset(k) on the intel pose graph with k = 10 % / 50 % of the candidates.  city20: the first 20 picks of
city10000.  python10: intel's first 10 picks by the driver a user could write without this solver -- the same greedy in Python,
every must-solve candidate of a pick evaluated through MAC.evaluate_objective_batch (independent preconditioned solves), pruned by
the same bound -- next to GreedyEig's time for the same 10 picks.  build_ms = wall time of the constructor (the inverse and the
fixed graph's Fiedler pair), select_ms = wall time of subset(k); solved / applications as GreedyEig.info() reports them.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd.solvers import MAC, GreedyEig  # noqa: E402
from mac_amd.utils.graphs import Edge  # noqa: E402


def pose_graph(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{name}.npz"))
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(g["fi"], g["fj"], g["fw"])]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(g["ci"], g["cj"], g["cw"])]
    return int(g["n"]), fixed, cand


def run(case, name, k_of):
    n, fixed, cand = pose_graph(name)
    m = len(cand)
    K = k_of(m)
    t0 = time.perf_counter()
    ge = GreedyEig(fixed, cand, n)
    build_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ge.subset(K)
    select_ms = (time.perf_counter() - t0) * 1e3
    inf = ge.info()
    solved, apps = inf["solved"], inf["applications"]
    ld = inf["ld"]
    print(json.dumps(dict(case=case, n=n, m=m, picks=K, form=inf["form"], ld=ld, batch=inf["batch"], fold=inf["fold"],
                          build_ms=round(build_ms, 2), select_ms=round(select_ms, 2), ms_per_pick=round(select_ms / K, 3),
                          ms_first_pick=round(float(ge.last_times[0]) * 1e3, 3),
                          lambda2_first=float(ge.last_lambda2[0]), lambda2_last=float(ge.last_lambda2[-1]),
                          solved_total=int(solved.sum()), solved_share=round(float(solved.sum() / (m * K - K * (K - 1) / 2)), 4),
                          applications_total=int(apps.sum()), applications_per_solved=round(float(apps.sum() / solved.sum()), 2),
                          product_flop_model=int(2.0 * ld * ld * apps.sum()))), flush=True)


def python_driver(name="intel", K=10):
    """The greedy on top of MAC.evaluate_objective_batch: what the package offered for this selection rule before GreedyEig."""
    n, fixed, cand = pose_graph(name)
    m = len(cand)
    mac = MAC(fixed, cand, n)
    t0 = time.perf_counter()
    x = np.zeros(m)
    lam, grad = mac.problem(x)                       # grad_e = w_e (v_i - v_j)^2: the bound is lam + grad_e
    order, nsolved = [], 0
    for _ in range(K):
        u = np.where(x > 0, -np.inf, lam + grad)
        idx = np.argsort(-u, kind="stable")[: m - len(order)]
        vals = np.full(m, np.nan)
        top = -np.inf
        for q in range(0, len(idx), 512):
            part = idx[q:q + 512]
            if u[part[0]] < top:
                break
            X = np.repeat(x[None, :], len(part), axis=0)
            X[np.arange(len(part)), part] = 1.0
            vals[part] = mac.evaluate_objective_batch(X)
            nsolved += len(part)
            top = max(top, float(np.nanmax(vals)))
        best, best_l2 = -1, 0.0
        for e in np.nonzero(np.isfinite(vals))[0]:
            if vals[e] > best_l2 + 1e-8:
                best, best_l2 = int(e), float(vals[e])
        x[best] = 1.0
        order.append(best)
        lam, grad = mac.problem(x)
    py_ms = (time.perf_counter() - t0) * 1e3
    ge = GreedyEig(fixed, cand, n)
    ge.subset(2)                                     # (first launches of every kernel)
    t0 = time.perf_counter()
    sol, _ = ge.subset(K)
    ge_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(case="python10", graph=name, picks=K, python_driver_ms=round(py_ms, 1), python_solved=nsolved,
                          greedy_eig_ms=round(ge_ms, 1), greedy_eig_solved=int(ge.info()["solved"].sum()),
                          speedup=round(py_ms / ge_ms, 1), same_picks=bool(np.array_equal(np.nonzero(sol)[0], np.sort(order))),
                          lambda2_python=float(lam), lambda2_greedy_eig=float(ge.last_lambda2[-1]))), flush=True)


if __name__ == "__main__":
    GreedyEig([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3).subset(1)      # (HIP context and code objects: not build_ms)
    for c in sys.argv[1:] or ["intel10", "intel50", "python10"]:
        if c == "intel10":
            run(c, "intel", lambda m: int(0.1 * m))
        elif c == "intel50":
            run(c, "intel", lambda m: int(0.5 * m))
        elif c == "city20":
            run(c, "city10000", lambda m: 20)
        elif c == "python10":
            python_driver()
        else:
            raise SystemExit(f"unknown case {c}")
