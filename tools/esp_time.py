"""GreedyESP timing (mac_amd/csrc/esp.h): one JSON line per case.

    python tools/esp_time.py [case ...]      cases: intel sphere2500 city10000 ais2klinik er10k (default: all)

Pose graphs: a full sweep (K = all candidates).  er10k: n = 10 000, chain-fixed, ER candidates with p = 0.01, K = 10 % of them.
build_ms = wall time of the constructor (host arrays + Sigma0 on the device), select_ms = device time of one run from its start
to the last pick (events on the handle's stream).  The bytes model counts HBM traffic per step (two rows of Sigma, the pending
block, the z column, the score pass over the candidates), per fold (Sigma read + written) and for Sigma0.

    python tools/esp_time.py --matrix-free [case ...]      cases: city10000 er10k chain100k:2000 chain100k:10000 (default: all)

The matrix-free route (mac_amd/csrc/esp_free.h; chain-fixed graphs, no Sigma).  chain100k:K: n = 100 000, chain-fixed, 2 M random
candidate pairs, K picks -- beyond the dense limit.  One run with eight budgets: per segment of picks the mean history length j,
us per pick, and the rate in the model "pick j streams 8 ld j bytes" (the history only: the score pass is not counted);
history_bytes = 8 ld K.

    python tools/esp_time.py --matrix-free-tree [case ...]      cases: chain100k:2000 tree100k:2000 (default: both)

The spanning-tree route (mac_amd/csrc/esp_tree.h; any connected fixed graph).  chain100k:K runs the chain case above through both
routes in the same process (route = "matrix_free" is the yardstick, route = "tree_free" the new one).  tree100k:K: n = 100 000, a
random recursive tree plus r = 1 000 extra fixed edges, 2 M random candidate pairs.  Beside the fields above: seeds, seed_ms = wall
time of the first weighted_resistances() (the history for the seeds, the r seeded columns, one rescoring pass), first_select_ms =
wall time of the first select (the history regrown for K picks included).
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


def chain100k(K, n=100000, m=2000000, seed=0):
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1)
    return n, fi, fi + 1, rng.uniform(0.5, 2.0, n - 1), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m), K


def tree100k(K, n=100000, r=1000, m=2000000, seed=0):
    rng = np.random.default_rng(seed)
    ti = np.arange(1, n)
    tj = (rng.random(n - 1) * ti).astype(np.int64)              # node i below a uniformly drawn earlier node
    fi = np.concatenate([ti, rng.integers(0, n, r)]); fj = np.concatenate([tj, rng.integers(0, n, r)])
    return n, fi, fj, rng.uniform(0.5, 2.0, len(fi)), rng.integers(0, n, m), rng.integers(0, n, m), rng.uniform(0.5, 2.0, m), K


def run_free(case, matrix_free=True):
    from mac_amd import _lib
    if case.startswith("chain100k"):
        n, fi, fj, fw, ci, cj, cw, K = chain100k(int(case.split(":")[1]))
    elif case.startswith("tree100k"):
        n, fi, fj, fw, ci, cj, cw, K = tree100k(int(case.split(":")[1]))
    else:
        n, fi, fj, fw, ci, cj, cw, K = er10k() if case == "er10k" else pose_graph(case)
    t0 = time.perf_counter()
    dev = _lib.Esp(n, fi, fj, fw, ci, cj, cw, matrix_free=matrix_free)
    build_ms = (time.perf_counter() - t0) * 1e3
    info = dev.info()
    ld, m = info["ld"], len(cw)
    ks = sorted({max(1, K * q // 8) for q in range(1, 9)})
    extra = {}
    if matrix_free == "tree":
        t0 = time.perf_counter()
        dev.weighted_resistances()
        extra["seed_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    dev.select([min(K, 64)])                     # (first launches of every kernel; the history is allocated before the timed events)
    extra["first_select_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    order, gain, t_ms = dev.select(ks)
    wall_ms = (time.perf_counter() - t0) * 1e3
    segs, k0, t_prev = [], 0, 0.0
    for k1, t1 in zip(ks, t_ms):                 # picks k0 .. k1 - 1: pick j has j columns behind it
        us = (float(t1) - t_prev) * 1e3 / (k1 - k0)
        j = (k0 + k1 - 1) / 2
        segs.append([round(j, 1), round(us, 3), round(8 * ld * j / (us * 1e-6) / 1e12, 3)])
        k0, t_prev = k1, float(t1)
    stream = 4 * ld * K * (K - 1)
    print(json.dumps(dict(case=case, route=info["form"].replace("chain_free", "matrix_free"), n=n, m=m, steps=K, form=info["form"], ld=ld,
                          seeds=info["seeds"], **extra, build_ms=round(build_ms, 2),
                          select_ms=round(float(t_ms[-1]), 3), select_wall_ms=round(wall_ms, 2),
                          us_per_step=round(float(t_ms[-1]) * 1e3 / K, 3), history_bytes=8 * ld * K, stream_bytes_model=stream,
                          stream_tb_s=round(stream / (float(t_ms[-1]) * 1e-3) / 1e12, 3), j_us_tbs=segs)), flush=True)


if __name__ == "__main__":
    GreedyESP([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3).subset(1)      # (HIP context and code objects: not build_ms)
    args = [a for a in sys.argv[1:] if not a.startswith("--matrix-free")]
    if "--matrix-free-tree" in sys.argv[1:]:
        for c in args or ["chain100k:2000", "tree100k:2000"]:
            if c.startswith("chain"):
                run_free(c)
            run_free(c, matrix_free="tree")
    elif "--matrix-free" in sys.argv[1:]:
        for c in args or ["city10000", "er10k", "chain100k:2000", "chain100k:10000"]:
            run_free(c)
    else:
        for c in args or ["intel", "sphere2500", "city10000", "ais2klinik", "er10k"]:
            run(c)
