"""Timing of the best-swap local search on lambda_2 (mac_amd/csrc/eig_exchange.h): one JSON line per run.

    python tools/eig_xch_time.py [case ...]      cases: greedy rounded python (default: all)

intel pose graph, K = 10 % of the candidates.  greedy / rounded: GreedyEig.exchange from GreedyEig's own selection / from the
selection MAC.solve rounds to (x_init = the first K candidates), run to convergence, three times each after a one-swap call has
launched every kernel once.  ms = wall time of the call, device_ms = between events around the call's first and last command;
rounds = swaps + 1 when converged; solved / applications / removal_solves as the call reports them, summed over the rounds.
greedy_ms_per_pick: a fresh subset(K) on the same handle divided by K, the yardstick of DESIGN section 12.

python: one round of the same search by the driver a user could write without it -- removal pairs by MAC.problem (lambda_2 and
the supergradient), the same bounds, row order and batches of 512, every batch through MAC.evaluate_objective_batch -- from the
greedy's selection,
next to the device's first round from the same selection (a max_swaps = 1 call, load included)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd.solvers import MAC, GreedyEig  # noqa: E402
from mac_amd.utils.graphs import Edge  # noqa: E402


def pose_graph(name="intel"):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{name}.npz"))
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(g["fi"], g["fj"], g["fw"])]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(g["ci"], g["cj"], g["cw"])]
    return int(g["n"]), fixed, cand


def starts(ge, mac, m, K):
    x0 = np.zeros(m)
    x0[:K] = 1.0
    return {"greedy": np.flatnonzero(ge.subset(K)[0]), "rounded": np.flatnonzero(mac.solve(K, x0)[0])}


def run(tag, ge, start, K, m, greedy_ms_per_pick, reps=3):
    ge.exchange(start, max_swaps=1)                  # (first launches of the exchange's kernels, its state allocated)
    for rep in range(reps):
        t0 = time.perf_counter()
        _, _, info = ge.exchange(start)
        wall = (time.perf_counter() - t0) * 1e3
        rounds = len(info["swaps"]) + (1 if info["converged"] else 0)
        inf = ge.info()
        print(json.dumps(dict(
            case=tag, rep=rep, m=m, K=K, ld=inf["ld"], batch=inf["batch"], fold=inf["fold"], pairs_per_round=K * (m - K),
            swaps=len(info["swaps"]), converged=bool(info["converged"]), lambda2_start=float(info["lambda2"][0]),
            lambda2_end=float(info["lambda2"][-1]), ms=round(float(info["t_ms"][0]), 2), device_ms=round(float(info["t_ms"][1]), 2),
            python_wall_ms=round(wall, 2), ms_per_round=round(float(info["t_ms"][0]) / max(rounds, 1), 2),
            solved=int(info["solved"].sum()), solved_share=round(float(info["solved"].sum()) / max(rounds * K * (m - K), 1), 4),
            applications=int(info["applies"].sum()), removal_solves=int(info["removal_solves"].sum()),
            greedy_ms_per_pick=round(greedy_ms_per_pick, 3),
            round_in_greedy_picks=round(float(info["t_ms"][0]) / max(rounds, 1) / greedy_ms_per_pick, 1))), flush=True)


def python_round(ge, mac, fixed, cand, n, start):
    """One round driven from Python: (ms, pairs solved, (out, in), value)."""
    m = len(cand)
    t0 = time.perf_counter()
    x = np.zeros(m)
    x[start] = 1.0
    tau = mac.evaluate_objective(x)
    rows = [int(e) for e in start]
    U = np.empty((len(rows), m))
    for r, e in enumerate(rows):                     # removal pairs: problem() returns lambda_2 and w_f (v_i - v_j)^2 of every candidate
        x[e] = 0.0
        lam_r, grad = mac.problem(x)
        x[e] = 1.0
        U[r] = np.where(x > 0, -np.inf, lam_r + grad)
    rowmax = U.max(axis=1)
    top, vals, nsolved = -np.inf, {}, 0
    unsel = np.flatnonzero(x == 0)
    for r in np.argsort(-rowmax, kind="stable"):
        if not rowmax[r] > max(tau, top):
            break
        order = unsel[np.argsort(-U[r, unsel], kind="stable")]
        base = x.copy()
        base[rows[r]] = 0.0
        for q in range(0, len(order), 512):
            if U[r, order[q]] < max(tau, top):
                break
            part = order[q:q + 512]
            X = np.repeat(base[None, :], len(part), axis=0)
            X[np.arange(len(part)), part] = 1.0
            lam = mac.evaluate_objective_batch(X)
            nsolved += len(part)
            for f, v in zip(part, lam):
                vals[(rows[r], int(f))] = float(v)
            top = max(top, float(lam.max()))
    best, running = None, tau
    for key in sorted(vals):
        if vals[key] > running + 1e-8:
            best, running = key, vals[key]
    return (time.perf_counter() - t0) * 1e3, nsolved, best, running


if __name__ == "__main__":
    GreedyEig([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0), Edge(0, 1, 0.5)], 3).exchange([0], max_swaps=1)      # (HIP context and code objects)
    n, fixed, cand = pose_graph()
    m = len(cand)
    K = int(0.1 * m)
    ge, mac = GreedyEig(fixed, cand, n), MAC(fixed, cand, n)
    s = starts(ge, mac, m, K)
    t0 = time.perf_counter()
    ge.subset(K)
    per_pick = (time.perf_counter() - t0) * 1e3 / K
    for c in sys.argv[1:] or ["greedy", "rounded", "python"]:
        if c in ("greedy", "rounded"):
            run(c, ge, s[c], K, m, per_pick)
        elif c == "python":
            ge.exchange(s["greedy"], max_swaps=1)
            dev = ge.exchange(s["greedy"], max_swaps=1)[2]
            py_ms, py_solved, py_swap, py_val = python_round(ge, mac, fixed, cand, n, s["greedy"])
            print(json.dumps(dict(case="python", m=m, K=K, python_round_ms=round(py_ms, 1), python_solved=py_solved,
                                  device_round_ms=round(float(dev["t_ms"][0]), 2), device_solved=int(dev["solved"].sum()),
                                  ratio=round(py_ms / float(dev["t_ms"][0]), 1),
                                  same_swap=bool(dev["swaps"] == [py_swap] if py_swap else not dev["swaps"]),
                                  lambda2_python=float(py_val), lambda2_device=float(dev["lambda2"][-1]))), flush=True)
        else:
            raise SystemExit(f"unknown case {c}")
