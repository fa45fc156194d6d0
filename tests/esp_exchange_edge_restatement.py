"""NumPy restatement of the exchange on the log tree count in edge space (mac_amd/csrc/esp_exchange_edge.h), written from the
formulas, for the tests.  Graphs are the tuples (n, fi, fj, fw, ci, cj, cw) of tests/esp_relax_restatement.py.

G is the Gram matrix of the M = m + r columns (the candidates, then the r seeds of the spanning-tree form; r = 0 on a chain)
under the fixed graph's Sigma0: esp_edge_restatement.G_of on a chain, esp_edge_tree_restatement.G_of over a spanning tree.  With
S' the selection plus the seeds,  R = A^T Sigma(S') A  is M x M and
    s_f = w_f R[f][f],   r_ef = R[e][f],   Delta(e, f) = (1 - s_e)(1 + s_f) + w_e w_f R[e][f]^2.
Column e enters by  R -= c R[:, e] R[e, :]  with c = w_e / (1 + s_e)  and leaves with  c = -w_e / (1 - s_e).
The loop: R <- G; the seeds, then the selection ascending, enter; rounds take the largest Delta over e selected, f an unselected
candidate (esp_exchange_restatement.top_two: ties to the lowest e, then the lowest f) and stop when Delta - 1 <= min_gain.
Nothing of size n is formed here: the loop runs at any number of nodes.
"""
import numpy as np

import esp_edge_restatement as EC
import esp_edge_tree_restatement as ET
import esp_exchange_restatement as E


def gram(g, tree):
    """(G, w of the M columns, m): the chain's closed form (tree False) or the spanning tree's with the seeds' columns."""
    m = len(g[6])
    w = np.asarray(g[6], dtype=np.float64)
    if not tree:
        return EC.G_of(g), w, m
    plan = ET.plan_of(g)
    return ET.G_of(g, plan), np.concatenate([w, plan["seeds"][2]]), m


def exchange(G, w, m, sel0, max_swaps, min_gain=1e-9):
    """dict(out, in, ratios = (1 - s_e)(1 + s_f'), deltas (the winners' Delta), separations (one per round, the stopping round
    included), selection, converged)."""
    R = np.array(G, dtype=np.float64)
    M = len(w)
    in_sel = np.zeros(M, dtype=bool)

    def update(e, c):
        R[:] -= c * np.outer(R[:, e], R[e, :].copy())

    def enter(e):
        update(e, w[e] / (1.0 + w[e] * R[e, e]))
        in_sel[e] = True

    for e in range(m, M):
        enter(e)
    for e in np.sort(np.asarray(sel0, dtype=np.int64)):
        enter(int(e))
    out = dict(out=[], ratios=[], deltas=[], separations=[], converged=0)
    out["in"] = []
    for _ in range(max_swaps):
        s = w * np.diag(R)
        sel = np.flatnonzero(in_sel[:m])
        unsel = np.flatnonzero(~in_sel[:m])
        r = R[np.ix_(sel, unsel)]
        D = (1.0 - s[sel])[:, None] * (1.0 + s[unsel])[None, :] + (w[sel][:, None] * w[unsel][None, :]) * r * r
        first, second = E.top_two(D, sel, unsel)
        out["separations"].append(E.separation(first, second))
        if first[0] - 1.0 <= min_gain:
            out["converged"] = 1
            break
        _, e, f = first
        ratio = 1.0 - s[e]
        update(e, -w[e] / (1.0 - s[e]))
        in_sel[e] = False
        ratio *= 1.0 + w[f] * R[f, f]
        enter(f)
        out["out"].append(e); out["in"].append(f); out["ratios"].append(ratio); out["deltas"].append(first[0])
    out["selection"] = np.flatnonzero(in_sel[:m])
    return out


def run(g, tree, sel0, max_swaps, min_gain=1e-9):
    G, w, m = gram(g, tree)
    return exchange(G, w, m, sel0, max_swaps, min_gain)


def near_best(G, w, m, sel, rel):
    """Every pair (e, f) whose Delta lies within `rel` (relative) of the best one at the selection `sel`, the winner included."""
    R = np.array(G, dtype=np.float64)
    picked = list(range(m, len(w))) + [int(e) for e in np.sort(np.asarray(sel, dtype=np.int64))]
    for e in picked:
        R -= (w[e] / (1.0 + w[e] * R[e, e])) * np.outer(R[:, e], R[e, :].copy())
    s = w * np.diag(R)
    sel = np.sort(np.asarray(sel, dtype=np.int64))
    unsel = np.setdiff1d(np.arange(m), sel)
    r = R[np.ix_(sel, unsel)]
    D = (1.0 - s[sel])[:, None] * (1.0 + s[unsel])[None, :] + (w[sel][:, None] * w[unsel][None, :]) * r * r
    i, j = np.nonzero(D >= D.max() * (1.0 - rel))
    return [(int(sel[a]), int(unsel[b])) for a, b in zip(i, j)]


# ---- the large inputs of the device tests: beyond every dense limit ----
def long_chain(n=100_000, cands=300, seed=41):
    """The generator of tests/test_esp_edge_gpu.py (restated): a chain of n nodes, `cands` random candidates, one at node 0 and one
    spanning the whole chain (given hi first)."""
    rng = np.random.default_rng(seed)
    fi = np.arange(n - 1); fj = fi + 1; fw = rng.uniform(0.5, 2.0, n - 1)
    a = rng.integers(0, n, cands); b = rng.integers(0, n, cands)
    a[0], b[0] = 0, 7000
    a[1], b[1] = n - 1, 0
    return n, fi, fj, fw, a, b, rng.uniform(0.5, 2.0, cands)


def large_tree(deep):
    """40 000 nodes, 20 fixed links beyond the tree, 300 candidates: a random recursive tree (deep False) or a spine of 3 000 nodes."""
    return ET.random_tree(40_000, 20, 300, 17, deep=3000 if deep else 0)
