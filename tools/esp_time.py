"""GreedyESP timing (mac_amd/csrc/esp.h): one JSON line per case.

    python tools/esp_time.py [case ...]      cases: intel sphere2500 city10000 ais2klinik er10k (default: all)

Pose graphs: a full sweep (K = all candidates).  er10k: n = 10 000, chain-fixed, ER candidates with p = 0.01, K = 10 % of them.
build_ms = wall time of the constructor (host arrays + Sigma0 on the device), select_ms = device time of one run from its start
to the last pick (events on the handle's stream).  The bytes model counts HBM traffic per step (two rows of Sigma, the pending
block, the z column, the score pass over the candidates), per fold (Sigma read + written) and for Sigma0.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd.solvers import GreedyESP  # noqa: E402
from mac_amd.utils.graphs import Edge  # noqa: E402


def pose_graph(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{name}.npz"))
    return int(g["n"]), g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"], len(g["cw"])


def er10k(n=10000, p=0.01, seed=0):
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    want = int(p * n * (n - 1) / 2)
    a = rng.integers(0, n, 2 * want); b = rng.integers(0, n, 2 * want)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n + hi)[hi - lo > 1])
    key = rng.permutation(key)[:want]
    ci, cj = key // n, key % n
    cw = rng.uniform(0.5, 2.0, len(ci))
    return n, fi, fj, fw, ci, cj, cw, int(0.1 * len(ci))


def run(case):
    n, fi, fj, fw, ci, cj, cw, K = er10k() if case == "er10k" else pose_graph(case)
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(fi, fj, fw)]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(ci, cj, cw)]
    t0 = time.perf_counter()
    esp = GreedyESP(fixed, cand, n)
    build_ms = (time.perf_counter() - t0) * 1e3
    info = esp.info()
    esp.subset(min(K, 8))                        # (first launches of every kernel)
    t0 = time.perf_counter()
    esp.subsets_lazy([K])
    wall_ms = (time.perf_counter() - t0) * 1e3
    order, gain, t_ms = esp._dev.select([K])
    ld, B, m = info["ld"], info["fold"], len(cw)
    step_bytes = 8 * ld * (2 + (B - 1) / 2 + 1) + m * (4 + 4 + 8 + 16 + 4 + 16)
    fold_bytes = 16 * ld * ld
    sigma0_bytes = 8 * ld * ld if info["form"] == "chain" else 16 * ld * ld * (ld // 32)
    folds = K // B
    model = K * step_bytes + folds * fold_bytes + 8 * ld * ld * 2      # (+ the copy of Sigma0 at the start of a run)
    print(json.dumps(dict(case=case, n=n, m=m, steps=K, form=info["form"], beta=info["beta"], ld=ld, fold=B,
                          build_ms=round(build_ms, 2), select_ms=round(float(t_ms[-1]), 3), select_wall_ms=round(wall_ms, 2),
                          us_per_step=round(float(t_ms[-1]) * 1e3 / K, 3), folds=folds,
                          bytes_per_step=int(step_bytes), bytes_per_fold=int(fold_bytes), bytes_sigma0=int(sigma0_bytes),
                          select_bytes_model=int(model), model_tb_s=round(model / (float(t_ms[-1]) * 1e-3) / 1e12, 3))), flush=True)


if __name__ == "__main__":
    GreedyESP([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3).subset(1)      # (HIP context and code objects: not build_ms)
    for c in sys.argv[1:] or ["intel", "sphere2500", "city10000", "ais2klinik", "er10k"]:
        run(c)
