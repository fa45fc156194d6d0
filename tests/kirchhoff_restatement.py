"""NumPy restatement of GreedyKirchhoff's selection rule, written from the maths (for the tests; not a port of any implementation).

A-optimal selection minimises tr L^+ (total effective resistance; Kirchhoff index / n).  Node 0 pinned, Sigma = L_red^-1 of the
connected fixed graph, Sigma~ = Sigma padded with a zero row / column for node 0:  tr L^+ = tr Sigma - (1^T Sigma 1) / n.
Candidate e = (u, v, w) keeps q_e = |z_e|^2, t_e = 1^T z_e (z_e = Sigma~ a_e) and s_e = w a_e^T Sigma~ a_e; adding it lowers tr L^+ by
    gain_e = w_e (q_e - t_e^2 / n) / (1 + s_e).
A step picks argmax gain over the unselected (ties: lowest index), then with z = Sigma~ a_f, c = w_f / (1 + s_f), y = Sigma z (Sigma
before this pick's update: the folded one minus the pending columns) and d_e = z_u - z_v:
    q_e <- q_e - 2 c d_e (y_u - y_v) + c^2 d_e^2 |z|^2,   t_e <- t_e - c d_e 1^T z,   s_e <- s_e - w_e c d_e^2,   Sigma <- Sigma - c z z^T,
the rank-1 updates kept as a low-rank block and folded into Sigma every `fold` steps, as esp_restatement.greedy keeps them.
"""
import numpy as np

import esp_restatement as R


def full_laplacian(n, edges):
    L = np.zeros((n, n))
    for i, j, w in edges:
        i, j = int(i), int(j)
        if i == j:
            continue
        L[i, i] += w; L[j, j] += w; L[i, j] -= w; L[j, i] -= w
    return L


def exact_trace(n, edges):
    """tr L^+ of the graph with the given (i, j, w) edges, by the pseudo-inverse."""
    return float(np.trace(np.linalg.pinv(full_laplacian(n, edges), hermitian=True)))


def trace_of(Sig, n):
    """tr L^+ from Sigma = L_red^-1."""
    return float(np.trace(Sig) - Sig.sum() / n)


def exact_scores(Sig, n, ci, cj, cw):
    """(q, t, s, gain) of every candidate from Sigma itself."""
    u, v = np.asarray(ci) - 1, np.asarray(cj) - 1
    Sp = np.zeros((Sig.shape[0] + 1, Sig.shape[1]))        # row -1: node 0
    Sp[:-1] = Sig
    Z = Sp[u] - Sp[v]
    q = np.einsum("ij,ij->i", Z, Z)
    t = Z.sum(axis=1)
    s = R.scores(Sig, ci, cj, cw)
    return q, t, s, np.asarray(cw) * (q - t * t / n) / (1.0 + s)


def greedy(n, fi, fj, fw, ci, cj, cw, K, fold=64):
    """(order, gains, margins, drift): margins[k] = relative gap between the best and the second-best unselected gain at step k
    (inf when only one is left); drift = the largest relative difference, over the unselected candidates at the end, between the
    gains the recurrences kept and an exact re-scoring from the final Sigma."""
    Sig, beta = R.initial_sigma(n, fi, fj, fw)
    assert beta == 0.0, "a disconnected fixed graph has infinite Kirchhoff index"
    npr = n - 1
    cw = np.asarray(cw, dtype=np.float64)
    u, v = np.asarray(ci) - 1, np.asarray(cj) - 1
    m = len(cw)
    q, t, s, g = exact_scores(Sig, n, ci, cj, cw)
    sel = np.zeros(m, dtype=bool)
    Zb = np.zeros((npr + 1, fold))          # row npr stays 0: node 0
    cb = np.zeros(fold)
    Sp = np.zeros((npr + 1, npr))
    Sp[:npr] = Sig
    order, gains, margins = [], [], []
    for k in range(K):
        masked = np.where(sel, -np.inf, g)
        e = int(np.argmax(masked))
        best = masked[e]
        masked[e] = -np.inf
        second = masked.max() if m - k > 1 else -np.inf
        margins.append((best - second) / abs(best) if np.isfinite(second) and best != 0 else np.inf)
        j = k % fold
        alpha = cb[:j] * (Zb[u[e], :j] - Zb[v[e], :j])
        z = Sp[u[e]] - Sp[v[e]] - Zb[:npr, :j] @ alpha
        c = cw[e] / (1.0 + s[e])
        y = Sp[:npr] @ z - Zb[:npr, :j] @ (cb[:j] * (Zb[:npr, :j].T @ z))      # Sigma before this pick, times z
        zz, zt = float(z @ z), float(z.sum())
        Zb[:npr, j] = z
        cb[j] = c
        zp, yp = np.append(z, 0.0), np.append(y, 0.0)
        d = zp[u] - zp[v]
        q = q - 2.0 * c * d * (yp[u] - yp[v]) + (c * d) ** 2 * zz
        t = t - c * d * zt
        s = s - cw * c * d * d
        g = cw * (q - t * t / n) / (1.0 + s)
        sel[e] = True
        order.append(e)
        gains.append(best)
        if j == fold - 1:
            Sp[:npr] -= (Zb[:npr] * cb) @ Zb[:npr].T
            Zb[:] = 0.0
            cb[:] = 0.0
    Sf = Sp[:npr] - (Zb[:npr] * cb) @ Zb[:npr].T
    ge = exact_scores(Sf, n, ci, cj, cw)[3]
    rest = ~sel
    drift = float(np.max(np.abs(g[rest] - ge[rest]) / np.maximum(np.abs(ge[rest]), 1e-300))) if rest.any() else 0.0
    return np.array(order), np.array(gains), np.array(margins), drift


def gains_after(n, fi, fj, fw, ci, cj, cw, order):
    """The exact gains of every candidate (selected ones included) in the fixed graph plus the candidates `order`."""
    fi2 = np.concatenate([np.asarray(fi), np.asarray(ci)[order]]); fj2 = np.concatenate([np.asarray(fj), np.asarray(cj)[order]])
    fw2 = np.concatenate([np.asarray(fw, dtype=np.float64), np.asarray(cw, dtype=np.float64)[order]])
    Sig, _ = R.initial_sigma(n, fi2, fj2, fw2)
    return exact_scores(Sig, n, ci, cj, cw)[3]
