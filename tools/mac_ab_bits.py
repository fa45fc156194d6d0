"""Same-box A/B of two builds of the library on MAC's OUTPUTS, bit for bit: the harness of tools/esp_ab_bits.py (one fresh child process
per library, one after the other; the parent opens no device; exit 1 at the first array that differs, with the case and the array
named) on the MAC case set below.

    python tools/mac_ab_bits.py LIB_A LIB_B      (two builds, MACHIP_BUILD_OUT=; MAC_AB_BITS_OUT=DIR keeps A.npz and B.npz there)

Two graphs: `chain`, a chain-fixed graph of 300 nodes (the single-workgroup and the preconditioned solver modes are reachable; 16
lanes), and `er`, 400 nodes on a fixed path through shuffled labels with more than kSelSmallMax = 32 768 ER candidates (the fused
gradient + select pass runs; 4 lanes).  On each: laplacian_csr; fiedler (lambda_2 and vector) under solver mode 1, under solver
mode 2 (chain only: the mode is the chain preconditioner's) and under precision 1, each on a fresh handle; gradient, lp_topk and
round_nearest at one decimal, where more candidates tie at the k-th rounded value than fit; fw_run with a warm start: f, dual,
gnorm, the solver modes, iters, upper and the final x; eval_batch with more entries than lanes; fw_sweep over more budgets than
lanes with a gap tolerance that stops some problems early (the child asserts that): X, R, upper, iters, status and f_traj;
fiedler_csr twice on the chain's Laplacian, so that the second call takes the cached handle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from esp_ab_bits import main  # noqa: E402


def shuffled_path_er(n, p, seed):
    """Fixed: the path through a random order of the nodes (connected, not chain-like); candidates: ER(n, p); weights in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    iu, ju = np.triu_indices(n, 1)
    pick = rng.random(len(iu)) < p
    return n, perm[:-1], perm[1:], rng.uniform(0.5, 2.0, n - 1), iu[pick], ju[pick], rng.uniform(0.5, 2.0, int(pick.sum()))


def cases():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from esp_relax_restatement import chain_er
    from mac_amd import _lib

    out = {}

    def put(case, **arrays):
        for k, v in arrays.items():
            out[f"{case}/{k}"] = np.asarray(v)

    rng = np.random.default_rng(11)
    for tag, g, lanes in (("chain", chain_er(300, 0.03, 1), 16), ("er", shuffled_path_er(400, 0.45, 2), 4)):
        m = len(g[6])
        k = m // 5
        assert tag == "chain" or m > 32768, m
        x = rng.random(m) * (2.0 * k / m)

        P = _lib.Problem(*g)
        P.set_x(x)
        indptr, indices, data = P.laplacian_csr()
        put(f"{tag}/laplacian_csr", indptr=indptr, indices=indices, data=data)

        for name, mode, prec in (("mode1", 1, 0), ("mode2", 2, 0), ("prec1", 0, 1)):
            if mode == 2 and tag != "chain":
                continue
            Q = _lib.Problem(*g)
            Q.set_solver(mode); Q.set_precision(prec)
            Q.set_x(x)
            lam, v, _ = Q.fiedler()
            put(f"{tag}/fiedler_{name}", lambda2=lam, v=v, solve_mode=Q.solve_mode())

        P.fiedler()
        put(f"{tag}/gradient", g=P.gradient())
        put(f"{tag}/lp_topk", s=P.lp_topk(k))
        P.set_x(np.round(rng.random(m), 2))
        kr = m // 2
        keys = np.sort(np.round(P.get_x(), 1))[::-1]
        assert (keys == keys[kr - 1]).sum() > 1 + (kr - 1 - np.argmax(keys == keys[kr - 1])), "no tie at the k-th rounded value"
        put(f"{tag}/round_nearest", tie=P.round_nearest(kr, decimals=1), top_k=P.round_nearest(kr, decimals=None))

        Q = _lib.Problem(*g)
        Q.set_x(np.full(m, k / m))
        r = Q.fw_run(k, 6, warm_start=True)
        put(f"{tag}/fw_run", f=r["f"], dual=r["dual"], gnorm=r["gnorm"], modes=r["modes"], iters=r["iters"], upper=r["upper"], x=Q.get_x())

        B = lanes + 3
        X = rng.random((B, m)) * (2.0 * k / m)
        lam, st = P.eval_batch(X)
        put(f"{tag}/eval_batch", lambda2=lam, status=st)

        ks = np.linspace(m // 20, m // 2, B).astype(np.int64)
        max_iters = 10
        r = P.fw_sweep(ks, np.outer(ks / m, np.ones(m)), max_iters=max_iters, gap_tol=1.8, grad_tol=0.0, warm_start=True, round_decimals=1)
        # (relative gap (upper - f) / |f| over ten iterations from x = k/m, on both graphs: above 9 at k = m/20, below 1 at k = m/2)
        assert (r["iters"] < max_iters).any() and (r["iters"] == max_iters).any(), f"{tag}: the sweep's stops are not mixed: {r['iters']}"
        put(f"{tag}/fw_sweep", X=r["x"], R=r["rounded"], upper=r["upper"], iters=r["iters"], status=r["status"], f_traj=r["f_traj"])

        if tag == "chain":
            for call in ("first", "cached"):
                lam, v, _, _ = _lib.fiedler_csr(indptr, indices, data, g[0])
                put(f"{tag}/fiedler_csr_{call}", lambda2=lam, v=v)
    return out


if __name__ == "__main__":
    sys.exit(main(sys.argv, cases, __file__))
