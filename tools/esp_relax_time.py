"""ESPRelaxation timing (mac_amd/csrc/esp_relax.h, esp_relax_edge.h, esp_relax_edge_tree.h): one JSON line per case.

    python tools/esp_relax_time.py [--no-check] [--edge-space | --edge-space-tree] [--no-python] [case ...]
    cases: intel sphere2500 ais2klinik city10000 (default: intel sphere2500 city10000), and chain100k (a chain of 100 000 nodes,
    weights U(0.5, 2), 4 000 seeded random candidates: --edge-space or --edge-space-tree only, never checked on the CPU);
    intel_kept50 ("chain plus kept closures": intel with its first 50 closures moved to the fixed list) and tree100k ("random tree":
    a random recursive tree of 100 000 nodes plus 1 000 random fixed links, 3 000 seeded random candidates, weights U(0.5, 2);
    never checked on the CPU): not the chain, so --edge-space refuses them, and tree100k is beyond the node form

--edge-space-tree: ESPRelaxation(edge_space="tree") -- N(x) = I + G D over the candidates and the seeds of a spanning tree, G stored
(DESIGN section 17); any connected fixed graph.  The line then carries seeds (r), and gram_ms = first_ms - eval_ms: what the first
relaxation call costs beyond one evaluation (three ld x ld allocations, the Gram build, log det N(0) is one evaluation itself); the
Gram kernel alone is k_edge_tree_gram in a rocprofv3 kernel trace.

--edge-space: ESPRelaxation(edge_space=True) -- N(x) = I + G D in the candidates' space; a fixed graph the
route refuses (not the connected chain) gives a line with "refused", and so does chain100k without --edge-space.  --no-python:
skip the Python-driven loop and leave its keys out of the line.

K = 20 % of the candidates, naive start, 20 Frank-Wolfe iterations with the stop tests off.  run_ms = wall time of
machip_esp_relax_run (the loop on the C side); python_ms = the same 20 iterations driven from Python: frank_wolfe over
ESPRelaxation.problem (machip_esp_relax_eval per iteration, gradient to the host, LP vertex and update in NumPy).  first_ms =
the first relaxation call on the handle (third buffer, incidence list, log det M(0)).  Unless --no-check: F of the final iterate
against two CPU routes (dense LAPACK LU, sparse SuperLU), d = their disagreement.  The bytes model is DESIGN section 13's.
Per kernel group: `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/esp_relax_time.py --no-check <case>`
(k_relax_assemble, k_gj_step, k_esp_scores, k_sel_small, k_fw_final + k_relax_scalars: one launch each per iteration, ld / 32 of
k_gj_step).
"""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd.optimization.frankwolfe import frank_wolfe  # noqa: E402
from mac_amd.solvers import ESPRelaxation, NaiveGreedy  # noqa: E402
from mac_amd.utils.graphs import Edge  # noqa: E402

ITERS = 20


def reduced(n, i, j, w):
    keep = i != j
    i, j, w = i[keep], j[keep], w[keep]
    L = sp.coo_matrix((np.concatenate([w, w, -w, -w]), (np.concatenate([i, j, i, j]), np.concatenate([i, j, j, i]))), shape=(n, n))
    return L.tocsc()[1:, 1:]


def cpu_logdets(n, fi, fj, fw, ci, cj, cw, x, beta):
    out = []
    for xv in (x, np.zeros(len(x))):
        M = (reduced(n, fi, fj, fw) + reduced(n, ci, cj, cw * xv) + beta * sp.identity(n - 1)).tocsc()
        lu = splu(M, permc_spec="COLAMD", diag_pivot_thresh=0.0)
        out.append((float(np.linalg.slogdet(M.toarray())[1]), float(np.sum(np.log(np.abs(lu.U.diagonal()))))))
    return out


def lp_vertex(g, k):
    s = np.zeros(len(g))
    s[np.lexsort((np.arange(len(g)), -g))[:k]] = 1.0
    return s


def chain100k(n=100000, cands=4000, seed=100):
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1)
    return n, fi, fi + 1, rng.uniform(0.5, 2.0, n - 1), rng.integers(0, n, cands), rng.integers(0, n, cands), rng.uniform(0.5, 2.0, cands)


def tree100k(n=100000, extra=1000, cands=3000, seed=101):
    rng = np.random.default_rng(seed)
    v = np.arange(1, n)
    par = (rng.random(n - 1) * v).astype(np.int64)          # a random recursive tree: the parent of v is uniform in [0, v)
    fi = np.concatenate([v, rng.integers(0, n, extra)]); fj = np.concatenate([par, rng.integers(0, n, extra)])
    return n, fi, fj, rng.uniform(0.5, 2.0, len(fi)), rng.integers(0, n, cands), rng.integers(0, n, cands), rng.uniform(0.5, 2.0, cands)


def run(case, check, edge_space=False, python_loop=True):
    if case == "tree100k":
        n, fi, fj, fw, ci, cj, cw = tree100k()
        check = False
    elif case == "intel_kept50":
        g = np.load(os.path.join(ROOT, "tests", "golden", "g2o_intel.npz"))
        n, c = int(g["n"]), 50
        fi, fj, fw = np.concatenate([g["fi"], g["ci"][:c]]), np.concatenate([g["fj"], g["cj"][:c]]), np.concatenate([g["fw"], g["cw"][:c]]).astype(np.float64)
        ci, cj, cw = g["ci"][c:], g["cj"][c:], g["cw"][c:].astype(np.float64)
    elif case == "chain100k":
        n, fi, fj, fw, ci, cj, cw = chain100k()
        check = False
        if not edge_space:                      # (n is beyond the node form's 16 384: there is nothing to time)
            print(json.dumps(dict(case=case, n=n, m=len(cw), form="node", refused="chain100k is --edge-space only")), flush=True)
            return
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", f"g2o_{case}.npz"))
        n, fi, fj, fw, ci, cj, cw = int(g["n"]), g["fi"], g["fj"], g["fw"].astype(np.float64), g["ci"], g["cj"], g["cw"].astype(np.float64)
    fixed = [Edge(int(a), int(b), float(c)) for a, b, c in zip(fi, fj, fw)]
    cand = [Edge(int(a), int(b), float(c)) for a, b, c in zip(ci, cj, cw)]
    m = len(cw)
    k = int(0.2 * m)
    x0 = NaiveGreedy(cand).subset(k)
    try:
        relax = ESPRelaxation(fixed, cand, n, edge_space=edge_space)
    except AssertionError as e:
        print(json.dumps(dict(case=case, n=n, m=m, form="edge_tree" if edge_space == "tree" else "edge" if edge_space else "node", refused=str(e))), flush=True)
        return
    dev = relax._dev
    t0 = time.perf_counter()
    try:
        dev.relax_eval(np.zeros(m), want_grad=False)
    except AssertionError as e:                     # (a size limit: decided at the first relaxation call)
        print(json.dumps(dict(case=case, n=n, m=m, form=dev.relax_info()["form"], refused=str(e))), flush=True)
        return
    first_ms = (time.perf_counter() - t0) * 1e3
    dev.relax_run(k, x0, max_iters=2, gap_tol=0.0, grad_tol=0.0)          # (first launches of every kernel)
    t0 = time.perf_counter()
    r = dev.relax_run(k, x0, max_iters=ITERS, gap_tol=0.0, grad_tol=0.0)
    run_ms = (time.perf_counter() - t0) * 1e3
    py = {}
    if python_loop:
        t0 = time.perf_counter()
        xp, up = frank_wolfe(x0, relax.problem, lambda gr: lp_vertex(gr, k), maxiter=ITERS, relative_duality_gap_tol=0.0, grad_norm_tol=0.0)
        python_ms = (time.perf_counter() - t0) * 1e3
        py = dict(python_ms=round(python_ms, 2), python_ms_per_iteration=round(python_ms / ITERS, 3), upper_python=float(up),
                  python_x_equal=bool(np.array_equal(xp, r["x"])))
    t0 = time.perf_counter()
    F = relax.evaluate_objective(r["x"])
    eval_ms = (time.perf_counter() - t0) * 1e3
    info = relax.info()
    ld = info["relax_ld"]                       # node space: n - 1 rounded up to 64; edge space: m (tree: m + r) rounded up to 64
    # (edge space: the assembly writes 8 ld^2 bytes as well, and the gradient reads 8 ld m instead of the scores' 52 m; over a tree
    # the stored G is read once more by each of the two: 8 ld^2 and 8 ld m)
    tree = info["relax_form"] == "edge_tree"
    out = dict(case=case, form=info["relax_form"], n=n, m=m, k=k, ld=ld, beta=info["beta"], iterations=int(r["iters"]), first_ms=round(first_ms, 2),
               run_ms=round(run_ms, 2), ms_per_iteration=round(run_ms / ITERS, 3), eval_ms=round(eval_ms, 3),
               bytes_assembly=(16 if tree else 8) * ld * ld, bytes_inverse=16 * ld * ld * (ld // 32),
               bytes_scores=(16 if tree else 8) * ld * m if edge_space else 52 * m,
               model_tb_s=round(((16 if tree else 8) * ld * ld + 16 * ld * ld * (ld // 32) + ((16 if tree else 8) * ld * m if edge_space else 52 * m)) / (run_ms / ITERS * 1e-3) / 1e12, 3),
               F_last=float(r["f"][-1]), upper=float(r["upper"]), **py)
    if tree:
        out.update(seeds=info["seeds"], gram_ms=round(first_ms - eval_ms, 2))
    if check:
        (dx, sx), (d0, s0) = cpu_logdets(n, fi, fj, fw, ci, cj, cw, r["x"], info["beta"])
        out.update(F_final_iterate=F, F_cpu_dense=dx - d0, F_cpu_sparse=sx - s0, logdet_Mx=dx, d=abs(dx - sx),
                   device_error=abs(F - (dx - d0)), tolerance=10 * max(abs(dx - sx), 1e-13 * abs(dx)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    check = "--no-check" not in args
    ESPRelaxation([Edge(0, 1, 1.0), Edge(1, 2, 1.0)], [Edge(0, 2, 1.0)], 3).evaluate_objective([0.5])     # (HIP context and code objects)
    for c in [a for a in args if not a.startswith("--")] or ["intel", "sphere2500", "city10000"]:
        run(c, check, edge_space="tree" if "--edge-space-tree" in args else "--edge-space" in args, python_loop="--no-python" not in args)
