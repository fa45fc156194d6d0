"""Same-box A/B of two builds of the library on GreedyEig's OUTPUTS, bit for bit: the harness of tools/esp_ab_bits.py (one fresh child
process per library, one after the other; the parent opens no device; times left out; exit 1 at the first array that differs, with
the case and the array named) on the GreedyEig case set below.

    python tools/eig_ab_bits.py LIB_A LIB_B      (two builds, MACHIP_BUILD_OUT=; EIG_AB_BITS_OUT=DIR keeps A.npz and B.npz there)

Per case: select's order and lambda_2; info()'s solved, applications, pending and lambda2; candidate_lambda2 and candidate_bounds;
the exchange's selection, out, in, lambda2, converged, solved, applications and removal_solves.  Equal application counts are the
evidence that the launch sequence is the same (tests/test_eig_precond_gpu.py pins them in absolute terms).  The cases are the
smallest shapes at which each shared host piece can go wrong: the dense chain form at ld = 192 with fold 4 and batch 8 (picks that
take several batches, picks that stop early, winners outside the last batch; a restart), the dense general form at ld = 128, the
chain without Sigma (default options, eig_free_split = 2, eig_free_rows = 8; a grown history), the spanning tree without Sigma (5
seeds, bounds before any pick, seeds carried over when the history grows) and the dense exchange from the K heaviest candidates
(fold 4, batch 8 < K = 28: removal pairs in several batches, folds inside rounds; to convergence and with max_swaps = 0).  The child
asserts from info() that the scan stopped early in some pick, took more than one batch in some pick, and that the exchange swapped."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from esp_ab_bits import main  # noqa: E402


def cases():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from esp_edge_tree_restatement import random_tree
    from esp_exchange_restatement import naive_start
    from esp_relax_restatement import chain_er
    from mac_amd import _lib

    out = {}

    def put(case, **arrays):
        for k, v in arrays.items():
            out[f"{case}/{k}"] = np.asarray(v)

    def put_select(case, h, k):
        order, lam, _ = h.select(k)
        i = h.info()
        put(case, order=order, lambda2=lam, solved=i["solved"], applications=i["applications"], pending=i["pending"], info_lambda2=i["lambda2"])
        return i

    chain, tree, chain60 = chain_er(130, 0.05, 1), random_tree(70, 5, 123, 7), chain_er(60, 0.05, 1)

    h = _lib.Eig(*chain, fold=4, batch=8)
    assert h.info()["form"] == "chain" and h.info()["ld"] == 192
    i = put_select("dense_chain/select_11", h, 11)
    unselected = h.m - np.arange(11)
    assert (i["solved"] < unselected).any(), "no pick of the dense chain case stopped its scan early"
    assert (i["solved"] > 8).any(), "no pick of the dense chain case took more than one batch"
    assert i["pending"] == 3
    put("dense_chain", candidate_lambda2_after_11=h.candidate_lambda2(), candidate_bounds_after_11=h.candidate_bounds())
    put_select("dense_chain/select_5", h, 5)

    h = _lib.Eig(*tree)
    assert h.info()["form"] == "dense" and h.info()["ld"] == 128
    put_select("dense_general/select_11", h, 11)

    for tag, opts in (("default", {}), ("split2", dict(eig_free_split=2)), ("rows8", dict(eig_free_rows=8))):
        with _lib.default_options(**opts):
            h = _lib.Eig(*chain, matrix_free=True)
        assert h.info()["form"] == "chain_free"
        put_select(f"chain_free_{tag}/select_10", h, 10)
        put(f"chain_free_{tag}", candidate_bounds_after_10=h.candidate_bounds())
        put_select(f"chain_free_{tag}/select_20", h, 20)

    h = _lib.Eig(*tree, matrix_free="tree")
    assert h.info()["form"] == "tree_free" and h.info()["seeds"] == 5
    put("tree_free", candidate_bounds_before=h.candidate_bounds())
    put_select("tree_free/select_10", h, 10)
    put_select("tree_free/select_20", h, 20)
    put("tree_free", candidate_lambda2_after_20=h.candidate_lambda2())

    K = 28
    start = naive_start(chain60, K)
    h = _lib.Eig(*chain60, fold=4, batch=8)
    assert h.info()["ld"] == 64
    keys = ("selection", "out", "in", "lambda2", "converged", "solved", "applications", "removal_solves")
    r = h.exchange(start, 10 * K)
    assert r["swaps"] >= 1, "the exchange case made no swap"
    put("dense_exchange/converge", **{k: r[k] for k in keys}, pending=h.info()["pending"])
    put("dense_exchange", candidate_lambda2_after=h.candidate_lambda2())
    r = h.exchange(start, 0)
    put("dense_exchange/max_swaps_0", **{k: r[k] for k in keys})
    return out


if __name__ == "__main__":
    sys.exit(main(sys.argv, cases, __file__))
