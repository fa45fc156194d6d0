"""Timing of machip_lowest_pairs' deflated Lanczos step against the Fiedler solve's own step: one JSON line per
measurement, written to profiles/lowest_pairs_time.txt (or the path given) as well as printed.

    python tools/pairs_time.py [--q Q] [--reps R] [--out PATH] [--only er2000,intel,...]

One process, on er2000_x0 (golden), intel and city10000 at the benchmark's x0, and configs[3] (er100k) at its x0.  Per graph:
  parent   the yardstick: a plain Fiedler solve forced onto the Lanczos path (fiedler_method "hip_lanczos"), R times after one warm-up
           call; us per step = machip_solve_stats.step_ms / steps_timed (hipEvents around the Krylov chunks), the median over the calls
  pairs    lowest_pairs(q) R times after one warm-up call; per column c >= 1 the median over the calls of (device ms of the column
           / its steps): hipEvents on the handle's stream around the whole column -- its two launches per step, the host's look at the
           records every 16 steps, Ritz vectors and explicit checks -- so this is the step as a solve pays for it, not a kernel's duration
ratio = pairs us per step / parent us per step, per column.

--method lanczos (default) | lobpcg | both: with lobpcg the columns run the preconditioned route in the same
process, after the Lanczos route's figures ("both") or instead of them; per column one `pairs_lob` line -- iterations, device ms, the
mode that produced it (6 / 7; 1 or 9: Lanczos ran or finished it) and, under "both", ms_lanczos / ms_lobpcg against the Lanczos
route's column of the same rank --, and per graph one `pairs_lob_build` line: the closures and the one-off preconditioner build in
ms (0: column 0's was reused).  The default output is then profiles/lowest_pairs_lob_time.txt, and the graphs are intel,
sphere2500 and city10000 at the benchmark's x0 (the greedy initial selection, the goldens' x_init) unless --only says otherwise."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mac_amd import _lib  # noqa: E402
from mac_amd.utils.fiedler import reference_start_block_q  # noqa: E402


def workloads(only):
    import bench
    if not only or "er2000" in only:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "er2000_x0.npz")))
        yield "er2000_x0", dict(n=int(g["n"]), fi=g["fi"], fj=g["fj"], fw=g["fw"], ci=g["ci"], cj=g["cj"], cw=g["cw"], x0=g["x"])
    for tag, cfg in (("intel", "c3"), ("sphere2500", "c5a"), ("city10000", "c5b"), ("er100k_x0", "c4")):
        if (not only and tag != "sphere2500") or (only and tag.split("_")[0] in only):
            yield tag, bench.make_workload(cfg)


def main(argv):
    q, reps, out, only, method = 4, 5, None, None, "lanczos"
    if "--method" in argv:
        method = argv[argv.index("--method") + 1]
        assert method in ("lanczos", "lobpcg", "both")
        if "--only" not in argv:
            only = ["intel", "sphere2500", "city10000"]
    if "--q" in argv:
        q = int(argv[argv.index("--q") + 1])
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    if "--only" in argv:
        only = argv[argv.index("--only") + 1].split(",")
    if out is None:
        out = os.path.join(ROOT, "profiles", "lowest_pairs_time.txt" if method == "lanczos" else "lowest_pairs_lob_time.txt")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for tag, w in workloads(only):
        n = int(w["n"])
        P = _lib.Problem(n, w["fi"], w["fj"], w["fw"], w["ci"], w["cj"], w["cw"])
        P.set_x(w["x0"])
        nnz = P.assemble()
        X = reference_start_block_q(n, q)
        x0 = np.ascontiguousarray(X[:, 0])
        P.set_solver(1)                                   # "hip_lanczos": the scalar step is what the new step is compared with
        P.fiedler(tol=1e-8, x0=x0)
        us, steps, mode = [], [], None
        for _ in range(reps):
            P.fiedler(tol=1e-8, x0=x0)
            st = P.stats
            us.append(1e3 * st.step_ms / max(1, st.steps_timed)); steps.append(int(st.lanczos_steps)); mode = P.solve_mode()[0]
        parent = float(np.median(us))
        emit(graph=tag, n=n, nnz=nnz, case="parent", mode=mode, steps=int(np.median(steps)), us_per_step=round(parent, 3), reps=reps)
        ms_lan = None
        if method != "lobpcg":
            P.lowest_pairs(q=q, tol=1e-8, X0=X, max_steps=20000)
            per, ms_col, st_col = [], [], []
            for _ in range(reps):
                lams, V, info = P.lowest_pairs(q=q, tol=1e-8, X0=X, max_steps=20000)
                ms = P.lowest_pairs_time(q)
                per.append(1e3 * ms / np.maximum(info["steps"], 1)); ms_col.append(ms); st_col.append(info["steps"])
            per, ms_col = np.median(np.array(per), axis=0), np.median(np.array(ms_col), axis=0)
            ms_lan = ms_col
            for c in range(1, q):
                emit(graph=tag, n=n, nnz=nnz, case="pairs", column=c, locked=c + 1, steps=int(st_col[-1][c]), ms=round(float(ms_col[c]), 3),
                     us_per_step=round(float(per[c]), 3), ratio=round(float(per[c]) / parent, 2), status=int(info["status"][c]),
                     residual=float(info["residual"][c]), reps=reps)
        if method != "lanczos":
            P.set_solver(0)                               # column 0 as a caller gets it: the automatic mode
            P.lowest_pairs(q=q, tol=1e-8, X0=X, max_steps=20000, method="lobpcg")
            ms_col, build = [], []
            for _ in range(reps):
                lams, V, info = P.lowest_pairs(q=q, tol=1e-8, X0=X, max_steps=20000, method="lobpcg")
                ms_col.append(P.lowest_pairs_time(q)); build.append(info["build_ms"])
            ms_col = np.median(np.array(ms_col), axis=0)
            emit(graph=tag, n=n, nnz=nnz, case="pairs_lob_build", closures=info["closures"], build_ms=round(float(np.median(build)), 3), reps=reps)
            for c in range(q):
                row = dict(graph=tag, n=n, nnz=nnz, case="pairs_lob", column=c, iterations=int(info["steps"][c]), ms=round(float(ms_col[c]), 3),
                           mode=int(info["method"][c]), restarts=int(info["restarts"][c]), status=int(info["status"][c]),
                           residual=float(info["residual"][c]), reps=reps)
                if ms_lan is not None and c >= 1:
                    row["ms_lanczos_over_ms_lobpcg"] = round(float(ms_lan[c]) / max(float(ms_col[c]), 1e-9), 2)
                emit(**row)
        P.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
