"""Same-box A/B of two builds of the library on the GreedyESP family's OUTPUTS (tools/ab_lib.sh compares rates): every array the
cases below return, bit for bit.

    python tools/esp_ab_bits.py LIB_A LIB_B      (two builds, MACHIP_BUILD_OUT=; ESP_AB_BITS_OUT=DIR keeps A.npz and B.npz there)

Each library runs the cases once in a fresh child process of its own (MACHIP_LIB is read at import), one child after the other,
and saves what it got; the parent opens no device, compares shape, type and bytes, and exits 1 at the first difference with the
case and the array named.  Times (t_ms) are left out.  The cases are the smallest shapes at which each shared host driver can go
wrong: the dense greedy (chain form at ld = 192 with 63 padding rows, fold 4, budgets [3, 11] and a restart; Gauss-Jordan form at
ld = 128), the chain-free greedy (K = 40: one slice up to pick 31, two from 32 on; esp_free_split = 2; a grown history at K = 60),
the tree greedy (5 seeds, carried over when the history grows), the dense exchange (folds inside rounds, LDS and global rows,
max_swaps = 0), the edge-space exchange (chain; tree with the seeds as forced picks; as a handle's first call with relax_run after
it) and the relaxation in the three spaces: five Frank-Wolfe iterations, relax_inner as a handle's first call, relax_eval with
and without the gradient (in edge space at x = 0 too), relax_info before and after the first call, relax_gram as a handle's
first call, one iteration through the multi-launch select (m = 40 000), and the refusals with their messages as byte arrays
(where a call breaks two rules, the message says which check comes first).

The child / save / compare harness is `main(argv, cases, script)`: another family's tool (tools/eig_ab_bits.py) passes its own case
set and file, and gets the same rules -- NAME_OUT=DIR for a tool NAME.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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

    def put_select(case, r):
        put(case, order=r[0], gain=r[1])

    def relax_info(h):      # (space, ld) as integers
        i = h.relax_info()
        return [("node", "edge", "edge_tree").index(i["form"]), i["ld"]]

    def put_xch(case, r):
        put(case, **{k: r[k] for k in ("selection", "out", "in", "ratios", "swaps", "converged")})

    chain, tree, chain60 = chain_er(130, 0.05, 1), random_tree(70, 5, 123, 7), chain_er(60, 0.05, 1)

    h = _lib.Esp(*chain, fold=4)
    assert h.info()["form"] == "chain" and h.info()["ld"] == 192
    put_select("dense_chain/select_3_11", h.select([3, 11]))
    assert h.info()["pending"] == 3
    put("dense_chain", resist_after_11=h.weighted_resistances())
    put_select("dense_chain/select_5", h.select([5]))

    h = _lib.Esp(*tree, fold=4)
    assert h.info()["form"] == "dense" and h.info()["ld"] == 128
    put_select("dense_general/select_11", h.select([11]))

    for tag, split in (("default", None), ("split2", 2)):
        with _lib.default_options(esp_free_split=split):
            h = _lib.Esp(*chain, matrix_free=True)
        put_select(f"chain_free_{tag}/select_40", h.select([40]))
        put(f"chain_free_{tag}", resist_after_40=h.weighted_resistances())
        put_select(f"chain_free_{tag}/select_60", h.select([60]))

    h = _lib.Esp(*tree, matrix_free="tree")
    assert h.info()["seeds"] == 5
    put("tree", resist_before=h.weighted_resistances())
    put_select("tree/select_40", h.select([40]))
    put("tree", resist_after_40=h.weighted_resistances())
    put_select("tree/select_60", h.select([60]))

    K = 28
    start = naive_start(chain60, K)
    h = _lib.Esp(*chain60, fold=4)
    assert h.info()["ld"] == 64
    put_xch("dense_exchange/lds", h.exchange(start, 10 * K))
    with _lib.default_options(esp_xch_lds_kb=0):
        put_xch("dense_exchange/global", h.exchange(start, 10 * K))
    put_xch("dense_exchange/max_swaps_0", h.exchange(start, 0))
    put("dense_exchange", resist_after=h.weighted_resistances())

    h = _lib.Esp(*chain60, matrix_free=True, edge_relax=True)
    put_xch("edge_exchange/chain", h.exchange_edge(start, 10 * K))
    h = _lib.Esp(*tree, matrix_free="tree", edge_relax="tree")
    Kt = len(tree[6]) // 3
    put_xch("edge_exchange/tree", h.exchange_edge(naive_start(tree, Kt), 10 * Kt))

    rng = np.random.default_rng(5)
    for tag, g, kw in (("node", chain, {}), ("edge", chain, dict(matrix_free=True, edge_relax=True)),
                       ("edge_tree", tree, dict(matrix_free="tree", edge_relax="tree"))):
        m = len(g[6])
        k = m // 3
        a, b = rng.random(m), rng.random(m)
        put(f"relax_{tag}", inner_first_call=_lib.Esp(*g, **kw).relax_inner(a, b))
        h = _lib.Esp(*g, **kw)
        r = h.relax_run(k, np.full(m, k / m), max_iters=5, gap_tol=0.0, grad_tol=0.0)
        put(f"relax_{tag}/run", **r)
        put(f"relax_{tag}", inner_after_run=h.relax_inner(a, b))

        h = _lib.Esp(*g, **kw)
        put(f"relax_{tag}/info", before=relax_info(h))
        x = rng.random(m) * (k / m)
        put(f"relax_{tag}/eval", F_only=h.relax_eval(x, want_grad=False)[0])
        put(f"relax_{tag}/info", after=relax_info(h))
        F, grad = h.relax_eval(x)
        put(f"relax_{tag}/eval", F=F, grad=grad)
        if kw:
            F0, grad0 = h.relax_eval(np.zeros(m))
            assert F0 == 0.0
            put(f"relax_{tag}/eval", F_at_0=F0, grad_at_0=grad0)

    put("relax_edge_tree", gram_first_call=_lib.Esp(*tree, matrix_free="tree", edge_relax="tree").relax_gram())

    for tag, g, kw, kx in (("chain", chain60, dict(matrix_free=True, edge_relax=True), K),
                           ("tree", tree, dict(matrix_free="tree", edge_relax="tree"), Kt)):
        h = _lib.Esp(*g, **kw)
        m = len(g[6])
        put_xch(f"edge_exchange_first_call/{tag}", h.exchange_edge(naive_start(g, kx), 10 * kx))
        put(f"edge_exchange_first_call/{tag}/relax_run", **h.relax_run(kx, np.full(m, kx / m), max_iters=3, gap_tol=0.0, grad_tol=0.0))

    from test_esp_relax_gpu import many_parallel_candidates
    g = many_parallel_candidates()
    m, k = len(g[6]), 4001
    assert m > 32768
    put("relax_node_multi_launch_select", **_lib.Esp(*g).relax_run(k, np.random.default_rng(3).random(m) * (k / m), max_iters=1, gap_tol=0.0, grad_tol=0.0))

    def refusal(case, call):
        try:
            call()
        except (AssertionError, _lib.MachipError) as e:
            put("refusals", **{case: np.frombuffer(str(e).encode(), dtype=np.uint8)})
        else:
            raise SystemExit(f"{case}: the call was not refused")

    m = len(chain[6])
    for tag, kw in (("chain", dict(matrix_free=True)), ("tree", dict(matrix_free="tree"))):
        g = chain if tag == "chain" else tree
        refusal(f"relax_eval_on_matrix_free_{tag}", lambda: _lib.Esp(*g, **kw).relax_eval(np.zeros(len(g[6]))))
        # (k outside [1, m] as well: the run's k check comes first on a handle that is not oversize)
        refusal(f"relax_run_on_matrix_free_{tag}_bad_k", lambda: _lib.Esp(*g, **kw).relax_run(0, np.zeros(len(g[6]))))
        refusal(f"relax_run_on_matrix_free_{tag}", lambda: _lib.Esp(*g, **kw).relax_run(3, np.zeros(len(g[6]))))
    refusal("exchange_edge_on_node_handle", lambda: _lib.Esp(*chain60, fold=4).exchange_edge(start, 10 * K))
    refusal("exchange_edge_on_matrix_free_handle", lambda: _lib.Esp(*chain60, matrix_free=True).exchange_edge(start, 10 * K))
    refusal("relax_gram_on_chain_edge_handle", lambda: _lib.Esp(*chain, matrix_free=True, edge_relax=True).relax_gram())
    refusal("relax_gram_on_node_handle", lambda: _lib.Esp(*chain).relax_gram())
    h = _lib.Esp(*tree, matrix_free="tree", edge_relax="tree")
    Mt = len(tree[6]) + h.info()["seeds"]
    for wrong in (Mt + 1, Mt - 1, 0):
        refusal(f"relax_gram_wrong_M_{wrong - Mt:+d}", lambda: _lib.check(h._lib.machip_esp_relax_gram(h._h, _lib.p_f64(np.empty((Mt + 1, Mt + 1))), wrong)))
    return out


def main(argv, cases=cases, script=__file__):
    """cases: () -> {"case/array": values}, run in the child; script: the file that calls this with them (what the child runs)."""
    tool = os.path.splitext(os.path.basename(script))[0]
    if len(argv) == 3 and argv[1] == "--child":
        np.savez(argv[2], **cases())
        return 0
    if len(argv) != 3:
        print(sys.modules[cases.__module__].__doc__)
        return 2
    got = []
    keep = os.environ.get(f"{tool.upper()}_OUT") or tempfile.mkdtemp(prefix=f"{tool}_")      # (the saved arrays: A.npz, B.npz)
    os.makedirs(keep, exist_ok=True)
    for i, lib in enumerate(argv[1:]):
        path = os.path.join(keep, f"{'AB'[i]}.npz")
        env = dict(os.environ, MACHIP_LIB=os.path.abspath(lib))
        subprocess.run([sys.executable, os.path.abspath(script), "--child", path], env=env, check=True)      # (one child at a time)
        got.append(np.load(path))
    A, B = got
    if sorted(A.files) != sorted(B.files):
        print("DIFFERENT: the two runs did not return the same arrays", sorted(set(A.files) ^ set(B.files)))
        return 1
    for name in A.files:
        if A[name].shape != B[name].shape or A[name].dtype != B[name].dtype or A[name].tobytes() != B[name].tobytes():      # (NaN is a value like any other)
            print(f"DIFFERENT: case {name.rsplit('/', 1)[0]}, array {name.rsplit('/', 1)[1]}\n A = {A[name]}\n B = {B[name]}")
            return 1
        print(f"same  {name}  {A[name].dtype}{list(A[name].shape)}")
    print(f"{tool}: {len(A.files)} arrays bit-identical between {argv[1]} and {argv[2]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
