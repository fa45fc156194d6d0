"""Same-box A/B of two builds of the library on the eigen-solver DRIVER's outputs, bit for bit: the harness of tools/esp_ab_bits.py (one
fresh child process per library, one after the other; the parent opens no device; exit 1 at the first array that differs, with the
case and the array named) on one case per route through mac_amd/csrc/solver*.h.

    python tools/solver_ab_bits.py LIB_A LIB_B      (two builds, MACHIP_BUILD_OUT=; SOLVER_AB_BITS_OUT=DIR keeps A.npz and B.npz there)

Every case is one eigen-solve on a fresh handle under set_solver(1) (unless the case names another mode), from the reference's start
vector (set_start), and records lambda_2, the vector, stats.lanczos_steps / restarts / steps_lowp / drift and solve_mode(); never a
time.  Cases, on the smallest graphs the suite uses for each route: golden er300_x0 and er2000_xfrac with the default options, the
chunk feeder (stream = 2), the chunk-granular loop (stream = 0), chunks with tail kernels, eager launches, captured chunks, short
chunks; the two-kernel form (classic_n: from the first step on er2000 only -- er300 is chain-like and keeps the single-workgroup
form) and the restarts a small basis forces (vcap = 80); a 300-node chain with a tenth of its closures active under solver modes
1 (single-workgroup form), 2 (with and without the exact preconditioner) and 0; the padded fixed-width step and the gather step on a
6 001-node chain; the column-panel step in five shapes, one of them ended by the drift monitor; both mixed-precision forms; a cold
start without a stored vector, then two warm starts after x has moved; the Lanczos -> exact hand-over and the exact mode's own
start on 9 000 nodes; two Frank-Wolfe iterations with the eigen-solve row-partitioned over two in-process ranks on one device.
The solves between processes are not covered here: tests/test_gpu_parity.py and tests/test_distributed.py run them."""
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from esp_ab_bits import main  # noqa: E402


def cases():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_golden
    from esp_relax_restatement import chain_er
    from mac_amd import _lib
    from mac_amd.utils.fiedler import reference_start_block
    from test_gpu_parity import _stream_cases

    out = {}

    def put_solve(case, P, lam, v):
        st = P.stats
        for k, val in dict(lambda2=lam, v=v, lanczos_steps=st.lanczos_steps, restarts=st.restarts, steps_lowp=st.steps_lowp,
                           drift=st.drift, solve_mode=P.solve_mode()).items():
            out[f"{case}/{k}"] = np.asarray(val)

    def handle(args, x, opts, solver=1, precision=0, start=True):
        with _lib.default_options(**opts):
            P = _lib.Problem(*args)
        P.set_solver(solver); P.set_precision(precision)
        if start:
            P.set_start(reference_start_block(args[0])[:, 0].copy())
        P.set_x(x)
        return P

    def solve(case, args, x, opts=None, **kw):
        P = handle(args, x, opts or {}, **kw)
        lam, v, _ = P.fiedler()
        put_solve(case, P, lam, v)
        P.close()

    def tag(opts):
        return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"

    gold = {}
    for nm in ("er300_x0", "er2000_xfrac"):
        g = load_golden(nm)
        gold[nm] = ((int(g["n"]), g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"]), g["x"])
    er300, er2000 = gold["er300_x0"], gold["er2000_xfrac"]

    for nm, (args, x) in gold.items():
        for opts in ({}, {"stream": 2}, {"stream": 0}, {"tailless": 0}, {"graph": 0}, {"graph": 1, "chunk": 8}, {"chunk": 6, "chunk_near": 2}):
            solve(f"{nm}/{tag(opts)}", args, x, opts)
    solve("er300_x0/classic_n=100000", *er300, {"classic_n": 100000})
    # (er300_x0 is chain-like and takes the single-workgroup form whatever classic_n says: the two-kernel form from the first step on er2000)
    solve("er2000_xfrac/classic_n=100000", *er2000, {"classic_n": 100000})
    solve("er2000_xfrac/vcap=80", *er2000, {"vcap": 80})
    assert out["er2000_xfrac/classic_n=100000/solve_mode"][0] == 5 and out["er2000_xfrac/vcap=80/restarts"] >= 1

    # (a tenth of the closures active: at most two per node, or solve() keeps the preconditioned modes out)
    chain = chain_er(300, 0.03, 1)
    rng = np.random.default_rng(11)
    xc = np.where(rng.random(len(chain[6])) < 0.1, rng.random(len(chain[6])), 0.0)
    solve("chain300/solver1", chain, xc)
    solve("chain300/solver2", chain, xc, solver=2)
    solve("chain300/solver2,woodbury=0", chain, xc, {"woodbury": 0}, solver=2)
    solve("chain300/solver0", chain, xc, solver=0)
    modes = [int(out[f"chain300/{c}/solve_mode"][0]) for c in ("solver1", "solver2", "solver2,woodbury=0")]
    assert modes == [4, 7, 6], modes

    (_, args6001, x6001, _), = [c for c in _stream_cases() if c[0] == "chain6001"]
    for opts in ({"ell": 1}, {"ell": 0}):
        solve(f"chain6001/{tag(opts)}", args6001, x6001, opts)

    for opts in ({"panel": 1, "panel_np": 3}, {"panel": 1, "panel_u": 0}, {"panel": 1, "stream": 0},
                 {"panel": 1, "panel_np": 3, "panel_nb": 6, "panel_cells": 2}, {"panel": 1, "panel_u_amp": 2}):
        solve(f"er2000_xfrac/{tag(opts)}", *er2000, opts)

    solve("er2000_xfrac/precision1", *er2000, precision=1)
    solve("er2000_xfrac/precision1,panel=1", *er2000, {"panel": 1}, precision=1)

    P = handle(*er2000, {}, start=False)
    lam, v, _ = P.fiedler()
    put_solve("er2000_xfrac/cold", P, lam, v)
    x = er2000[1]
    for i in (1, 2):
        x = np.clip(x + 0.05 * np.random.default_rng(i).standard_normal(len(x)), 0.0, 1.0)
        P.set_x(x)
        lam, v, _ = P.fiedler(warm_start=True)
        put_solve(f"er2000_xfrac/warm{i}", P, lam, v)
    P.close()

    # (the graph of test_lanczos_hands_over_to_the_exact_mode_on_its_own_forecast)
    n, s_ = 9000, 1800
    rng = np.random.default_rng(21)
    fi = np.arange(n - 1, dtype=np.int32)
    ci = rng.choice(n - 60, s_, replace=False).astype(np.int32); cj = (ci + rng.integers(2, 50, s_)).astype(np.int32)
    P = handle((n, fi, fi + 1, np.full(n - 1, 40.0), ci, cj, np.full(s_, 15.0)), np.ones(s_), {}, solver=0)
    for call in ("handover", "exact_start"):
        lam, v, _ = P.fiedler()
        put_solve(f"chain9000/solver0_{call}", P, lam, v)
    assert out["chain9000/solver0_handover/solve_mode"][0] == 7 and out["chain9000/solver0_handover/lanczos_steps"] > 128
    P.close()

    # in-process ranks on one device (as tests/test_gpu_parity.py test_in_process_ranks_match_single_rank enables them): every
    # eigen-solve of the two Frank-Wolfe iterations is row-partitioned
    g = load_golden("er2000_solve")
    R, k = 2, int(g["k"])
    Ps = [_lib.Problem(int(g["n"]), g["fi"], g["fj"], g["fw"], g["ci"], g["cj"], g["cw"]) for _ in range(R)]
    _lib.comm_init_local(Ps)
    assert _lib.load().machip_comm_mode(Ps[0]._h) == 3
    got = [None] * R

    def drive(r):
        try:
            P = Ps[r]
            P.set_start(reference_start_block(int(g["n"]))[:, 0].copy())
            P.set_x(g["x_init"])
            fs, steps = [], []
            for it in range(2):
                fs.append(P.fw_step(k, it))
                steps.append([P.stats.lanczos_steps, P.stats.restarts])
                P.fw_commit()
            got[r] = dict(f_dual_gnorm=np.array(fs), steps=np.array(steps), x=P.get_x(), gradient=P.gradient())
        except Exception as exc:       # a failing rank must not leave its peer in the barrier
            got[r] = exc
            Ps[r].close()
    th = [threading.Thread(target=drive, args=(r,)) for r in range(R)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for r in range(R):
        if isinstance(got[r], Exception):
            raise got[r]
        for name, val in got[r].items():
            out[f"in_process_ranks/rank{r}/{name}"] = val
    for P in Ps:
        P.close()
    return out


if __name__ == "__main__":
    sys.exit(main(sys.argv, cases, __file__))
