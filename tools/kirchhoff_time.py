"""GreedyKirchhoff timing (mac_amd/csrc/kirchhoff.h): one JSON line per case.

    python tools/kirchhoff_time.py [case ...]      cases: intel sphere2500 city10000 (default: all)

Pose graphs at K = 10 % of the candidates.  build_ms = wall time of the constructor (host arrays + Sigma0 on the device),
select_ms = device time of one run from its start to the last pick (events on the handle's stream), us_per_pick = their
quotient; product_tb_s_floor = 8 ld^2 bytes per pick over the WHOLE pick's time -- a floor on the rate of the product k_kir_y,
which is one of the pick's five launches.  index_ms = wall time of kirchhoff_index(selection) (Sigma0 copy, K forced picks, folds,
two trace reductions); identity = (index before - sum of gains - index after) / index before; winner_drift = the largest relative
difference, at eight prefixes k of the run, between the gain the recurrences kept for pick k and its exact re-scoring from Sigma
after k picks (a fresh run of k picks, then gains()).

The split by kernel comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o k -- python tools/kirchhoff_time.py city10000
    python tools/kirchhoff_time.py --kernel-stats <dir>/.../k_kernel_stats.csv

prints, per kernel of kirchhoff.h and esp.h, calls, total ms and mean us per launch, and for k_kir_y the rate 8 ld^2 / mean with ld
taken from --ld (default: city10000's 10 048).
"""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pose_graph(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{name}.npz"))
    return int(g["n"]), g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"]


def run(case):
    from mac_amd.solvers import GreedyKirchhoff
    from mac_amd.utils.graphs import Edge
    n, fi, fj, fw, ci, cj, cw = pose_graph(case)
    m = len(cw)
    K = max(1, m // 10)
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(fi, fj, fw)]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(ci, cj, cw)]
    t0 = time.perf_counter()
    gk = GreedyKirchhoff(fixed, cand, n)
    build_ms = (time.perf_counter() - t0) * 1e3
    info = gk.info()
    gk.subset(min(K, 8))                         # (first launches of every kernel)
    t0 = time.perf_counter()
    order, gain, t_ms = gk._dev.kirchhoff_select([K])
    wall_ms = (time.perf_counter() - t0) * 1e3
    ld, B = info["ld"], info["fold"]
    us = float(t_ms[-1]) * 1e3 / K
    drift = 0.0                                  # the kept gain of pick k against its exact re-scoring after k picks, at 8 prefixes
    for k in sorted({max(1, K * q // 8) for q in range(1, 9)} - {K}) + [K - 1]:
        gk._dev.kirchhoff_select([k])
        exact = gk.gains()[order[k]]
        drift = max(drift, abs(float(gain[k]) - exact) / exact)
    t0 = time.perf_counter()
    after = gk.kirchhoff_index(order)
    index_ms = (time.perf_counter() - t0) * 1e3
    before = gk.kirchhoff_index(None)
    print(json.dumps(dict(case=case, n=n, m=m, picks=K, form=info["form"], ld=ld, fold=B, build_ms=round(build_ms, 2),
                          select_ms=round(float(t_ms[-1]), 3), select_wall_ms=round(wall_ms, 2), us_per_pick=round(us, 2),
                          product_bytes=8 * ld * ld, product_tb_s_floor=round(8 * ld * ld / (us * 1e-6) / 1e12, 3),
                          index_ms=round(index_ms, 2), index_before=before, index_after=after, gain_sum=float(gain.sum()),
                          identity=(before - float(gain.sum()) - after) / before, winner_drift=drift)), flush=True)


def kernel_stats(path, ld):
    rows = list(csv.DictReader(open(path)))
    keep = [r for r in rows if any(k in r["Name"] for k in ("k_kir_", "k_esp_", "Memcpy", "copyBuffer"))]
    for r in sorted(keep, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].split("(")[0].replace("machip::", "")
        calls, tot, avg = int(r["Calls"]), float(r["TotalDurationNs"]), float(r["AverageNs"])
        out = dict(kernel=name, calls=calls, total_ms=round(tot / 1e6, 3), mean_us=round(avg / 1e3, 2))
        if "k_kir_y" in name:
            out["tb_s"] = round(8 * ld * ld / (avg * 1e-9) / 1e12, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--kernel-stats" in args:
        ld = int(args[args.index("--ld") + 1]) if "--ld" in args else 10048
        kernel_stats(args[args.index("--kernel-stats") + 1], ld)
    else:
        from mac_amd.solvers import GreedyKirchhoff
        from mac_amd.utils.graphs import Edge
        GreedyKirchhoff([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3).subset(1)      # (HIP context and code objects: not build_ms)
        for c in args or ["intel", "sphere2500", "city10000"]:
            run(c)
