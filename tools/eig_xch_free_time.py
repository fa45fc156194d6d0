"""Timing of GreedyEig.exchange_free against GreedyEig.exchange: one JSON line per run, written to
profiles/eig_exchange_free_time.txt (or the path given) as well as printed.

    python tools/eig_xch_free_time.py [--swaps N] [--out PATH]

intel pose graph (its fixed edges are the chain), K = 78 from GreedyEig.subset.  The dense ``exchange`` and ``exchange_free`` on a
``matrix_free=True`` and on a ``matrix_free="tree"`` handle run in one process, three runs each of N swaps (default 10; 0: to
convergence) after a one-swap call has launched every kernel once.  The yardstick is the dense route in the same run.
Per run: ms (wall time of the call), device_ms, ms_per_round, and whether the swaps are the dense route's.
load: a max_swaps = 0 call (reset, the selection loaded, its Fiedler pair polished), three times per route.
compaction: on the matrix-free routes a 2-swap call with option eig_xch_free_swaps = 1 (one compaction, before the second round)
next to the same call with the option unset (none); the difference is the compaction -- a fraction of a millisecond between two
calls of about 300 ms, so it resolves a compaction only where the calls' own scatter is below that (DESIGN section 23 takes the figure
from the kernels' durations, profiles/eig_exchange_free_load_kstats.txt)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from eig_xch_time import pose_graph  # noqa: E402
from mac_amd import _lib  # noqa: E402
from mac_amd.solvers import GreedyEig  # noqa: E402


def main(argv):
    swaps, out = 10, os.path.join(ROOT, "profiles", "eig_exchange_free_time.txt")
    if "--swaps" in argv:
        swaps = int(argv[argv.index("--swaps") + 1])
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    n, fixed, cand = pose_graph()
    m, K = len(cand), 78
    routes = {"dense": GreedyEig(fixed, cand, n), "chain_free": GreedyEig(fixed, cand, n, matrix_free=True),
              "tree_free": GreedyEig(fixed, cand, n, matrix_free="tree")}
    start = np.flatnonzero(routes["dense"].subset(K)[0])
    cap = swaps if swaps > 0 else None
    ref = None
    for tag, ge in routes.items():
        call = ge.exchange if tag == "dense" else ge.exchange_free
        call(start, max_swaps=1)                     # (first launches of every kernel, the call's state allocated)
        for rep in range(3):
            info = call(start, max_swaps=0)[2]
            emit(case="load", route=tag, rep=rep, n=n, m=m, K=K, ld=ge.info()["ld"], ms=round(float(info["t_ms"][0]), 3),
                 device_ms=round(float(info["t_ms"][1]), 3))
        for rep in range(3):
            info = call(start, max_swaps=cap)[2]
            rounds = len(info["swaps"]) + (1 if info["converged"] else 0)
            if ref is None:
                ref = info["swaps"]
            emit(case="rounds", route=tag, rep=rep, n=n, m=m, K=K, swaps=len(info["swaps"]), converged=bool(info["converged"]),
                 lambda2_start=float(info["lambda2"][0]), lambda2_end=float(info["lambda2"][-1]), ms=round(float(info["t_ms"][0]), 2),
                 device_ms=round(float(info["t_ms"][1]), 2), ms_per_round=round(float(info["t_ms"][0]) / max(rounds, 1), 2),
                 solved=int(info["solved"].sum()), applications=int(info["applies"].sum()), compactions=info.get("compactions"),
                 same_swaps_as_dense=bool(info["swaps"] == ref))
        if tag == "dense":
            continue
        for rep in range(3):
            plain = call(start, max_swaps=2)[2]
            with _lib.default_options(eig_xch_free_swaps=1):
                comp = call(start, max_swaps=2)[2]
            emit(case="compaction", route=tag, rep=rep, K=K, compactions=comp["compactions"], ms_with=round(float(comp["t_ms"][0]), 2),
                 ms_without=round(float(plain["t_ms"][0]), 2), compaction_ms=round(float(comp["t_ms"][0] - plain["t_ms"][0]), 2),
                 same_swaps=bool(comp["swaps"] == plain["swaps"]))
    with open(out, "w") as f:
        f.write("# python tools/eig_xch_free_time.py --swaps %d   (MI355X; intel, K = 78 from GreedyEig.subset)\n" % swaps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
