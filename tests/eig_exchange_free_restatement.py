"""NumPy restatement of what GreedyEig.exchange_free adds to the exchange (tests/eig_exchange_restatement.py has the rounds), written
from the rules (for the tests; not a port of any implementation).

The history.  Sigma = Sigma0 - Z diag(c) Z^T, Sigma0 the inverse of the reduced Laplacian (node 0 pinned) of the chain or the
spanning tree, column q of Z the Sherman-Morrison column z_q = Sigma_{q-1} a_q of edge q with c_q = w_q / (1 + w_q a_q^T z_q).  A
removal is the edge with weight -w.

  * ``sequential``: one edge after the other.
  * ``blocked``: ``block`` edges at a time against the inverse as it stands:  Z0 = Sigma A;  G = A^T Z0;  for b in order
    c_b = w_b / (1 + w_b G[b, b]), N[b, b'] = c_b G[b, b'] (b' > b), G -= c_b g g^T with g column b of G before the update;
    Z = Z0 (I + N)^-1 by forward substitution along every row (N is strictly upper triangular).
  * ``compaction_rule``: the history has room for seeds + K + 2 C + 1 columns; the load leaves seeds + K; a round that starts with
    pending + 3 above the room compacts first (pending back to seeds + K); a swap appends two columns.
"""
import numpy as np

import eig_restatement as R


def incidence(n, ci, cj):
    """Reduced incidence columns (n - 1 rows; node 0 has no row) of the edges (ci[q], cj[q])."""
    A = np.zeros((n - 1, len(ci)))
    for q, (i, j) in enumerate(zip(ci, cj)):
        if i > 0:
            A[i - 1, q] += 1.0
        if j > 0:
            A[j - 1, q] -= 1.0
    return A


def sigma0_of(n, fi, fj, fw):
    """inv of the reduced Laplacian of the edges given (the chain, a spanning tree)."""
    return np.linalg.inv(R.laplacian(n, fi, fj, fw)[1:, 1:])


def tree_edges(parent, Rt):
    """The spanning tree of _lib.host_esp_tree as edges: node v > 0 hangs under parent[v] by a link of resistance Rt[v] - Rt[parent[v]]."""
    v = np.arange(1, len(parent))
    return v, np.asarray(parent)[v], 1.0 / (np.asarray(Rt)[v] - np.asarray(Rt)[np.asarray(parent)[v]])


def sequential(Sigma, A, w):
    """(Z, c) of the edges with incidence columns A and weights w, loaded one at a time onto the inverse Sigma."""
    S = np.array(Sigma, dtype=np.float64)
    Z, c = np.zeros(A.shape), np.zeros(len(w))
    for q in range(len(w)):
        z = S @ A[:, q]
        c[q] = w[q] / (1.0 + w[q] * (A[:, q] @ z))
        Z[:, q] = z
        S -= c[q] * np.outer(z, z)
    return Z, c


def blocked_block(Sigma, A, w):
    """One block: (Z, c, N)."""
    B = len(w)
    Z0 = Sigma @ A
    G = A.T @ Z0
    c, N = np.zeros(B), np.zeros((B, B))
    for b in range(B):
        c[b] = w[b] / (1.0 + w[b] * G[b, b])
        N[b, b + 1:] = c[b] * G[b, b + 1:]
        g = G[:, b].copy()
        G -= c[b] * np.outer(g, g)
    Z = Z0.copy()
    for b in range(1, B):                                   # z_b = Z0[:, b] - sum_{b' < b} z_b' N[b', b]
        Z[:, b] -= Z[:, :b] @ N[:b, b]
    return Z, c, N


def blocked(Sigma, A, w, block=64):
    """(Z, c) of the same edges, ``block`` at a time."""
    S = np.array(Sigma, dtype=np.float64)
    Z, c = np.zeros(A.shape), np.zeros(len(w))
    for q in range(0, len(w), block):
        zb, cb, _ = blocked_block(S, A[:, q:q + block], np.asarray(w[q:q + block], dtype=np.float64))
        Z[:, q:q + block], c[q:q + block] = zb, cb
        S -= (zb * cb) @ zb.T
    return Z, c


def implied_inverse(Sigma0, Z, c):
    return Sigma0 - (Z * c) @ Z.T


def compaction_rule(K, seeds, C, swaps, converged=True):
    """(compactions, pending) after a call that made ``swaps`` swaps with room for C of them between compactions (C = min(max_swaps,
    option eig_xch_free_swaps)); ``converged``: a last round found no swap (it starts, so it too may compact)."""
    room = seeds + K + 2 * C + 1
    pending, comp = seeds + K, 0
    for r in range(swaps + (1 if converged else 0)):
        if pending + 3 > room:
            pending, comp = seeds + K, comp + 1
        if r < swaps:
            pending += 2
    return comp, pending


def history_after(g, Sigma0, seeds, start, swaps=(), C=32, converged=True, block=64):
    """(Z, c) as a call leaves them: the seeds (su, sv, sw; one at a time), the selection ``start`` ascending in blocks, then per swap
    (e, f) the downdate of e and the column of f, with the compactions of ``compaction_rule`` (back to the seeds, the current
    selection ascending in blocks) where they fall."""
    n, fi, fj, fw, ci, cj, cw = g
    ci, cj, cw = np.asarray(ci), np.asarray(cj), np.asarray(cw, dtype=np.float64)
    su, sv, sw = seeds
    Zs, cs = sequential(Sigma0, incidence(n, su, sv), np.asarray(sw, dtype=np.float64))
    Sseed = implied_inverse(Sigma0, Zs, cs)
    r, K = len(sw), len(start)

    def load(rows):
        rows = np.array(sorted(rows), dtype=np.int64)
        Z, c = blocked(Sseed, incidence(n, ci[rows], cj[rows]), cw[rows], block=block)
        return [Z], [c]
    rows = sorted(int(e) for e in start)
    Zl, cl = load(rows)
    pending, room = r + K, r + K + 2 * C + 1
    for t in range(len(swaps) + (1 if converged else 0)):
        if pending + 3 > room:
            Zl, cl = load(rows)
            pending = r + K
        if t < len(swaps):
            e, f = swaps[t]
            S = implied_inverse(Sseed, np.hstack(Zl), np.concatenate(cl))
            Z, c = sequential(S, incidence(n, ci[[e, f]], cj[[e, f]]), np.array([-cw[e], cw[f]]))
            Zl.append(Z); cl.append(c)
            rows[rows.index(e)] = f
            pending += 2
    return np.hstack([Zs] + Zl), np.concatenate([cs] + cl)


def with_closures(g, r):
    """The graph with its first r candidates moved to the fixed edges (a chain plus r closures: r seeds on the tree route)."""
    n, fi, fj, fw, ci, cj, cw = g
    return (n, np.concatenate([fi, ci[:r]]), np.concatenate([fj, cj[:r]]), np.concatenate([fw, cw[:r]]), ci[r:], cj[r:], cw[r:])
