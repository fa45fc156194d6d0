"""NumPy restatement of GreedyESP's selection rule, written from the maths (for the tests; not a port of any implementation).

Node 0 pinned; L_red = the fixed graph's Laplacian without row / column 0; Sigma = (L_red + beta I)^-1 with beta = 0 when the
fixed graph is connected, 1e-4 otherwise (an error when a node other than 0 has no fixed edge).  Candidate e = (u, v, w) scores
s_e = w (Sigma_uu + Sigma_vv - 2 Sigma_uv) (node-0 terms 0).  A step picks argmax s over the unselected (ties: lowest index),
then with z = Sigma a_e*, c = w* / (1 + s*):  Sigma <- Sigma - c z z^T,  s <- s - w c (z_u - z_v)^2.  The rank-1 updates are
kept as a low-rank block and folded into Sigma every `fold` steps (a dense update per step would not fit a test's time).
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components


def reduced_laplacian(n, fi, fj, fw, sparse=False):
    fi, fj, fw = np.asarray(fi), np.asarray(fj), np.asarray(fw, dtype=np.float64)
    keep = fi != fj
    fi, fj, fw = fi[keep], fj[keep], fw[keep]
    rows = np.concatenate([fi, fj, fi, fj])
    cols = np.concatenate([fi, fj, fj, fi])
    data = np.concatenate([fw, fw, -fw, -fw])
    L = sp.coo_matrix((data, (rows, cols)), shape=(n, n)).tocsr()[1:, 1:]
    return L.tocsc() if sparse else L.toarray()


def beta_of(n, fi, fj, fw):
    fi, fj, fw = np.asarray(fi), np.asarray(fj), np.asarray(fw, dtype=np.float64)
    keep = (fi != fj) & (fw != 0)
    A = sp.coo_matrix((np.ones(int(keep.sum())), (fi[keep], fj[keep])), shape=(n, n))
    ncomp, _ = connected_components(A, directed=False)
    if ncomp == 1:
        return 0.0
    touched = np.zeros(n, dtype=bool)
    touched[fi[keep]] = True
    touched[fj[keep]] = True
    if not touched[1:].all():
        raise ValueError("a node other than 0 has no fixed edge")
    return 1e-4


def initial_sigma(n, fi, fj, fw):
    beta = beta_of(n, fi, fj, fw)
    L = reduced_laplacian(n, fi, fj, fw)
    return np.linalg.inv(L + beta * np.eye(n - 1)), beta


def scores(Sig, ci, cj, cw):
    u, v = np.asarray(ci) - 1, np.asarray(cj) - 1
    d = np.concatenate([np.diag(Sig), [0.0]])             # index -1 -> the appended 0
    S = np.pad(Sig, ((0, 1), (0, 1)))
    a, b = np.minimum(u, v), np.maximum(u, v)              # upper triangle: a pair and its reverse score alike
    return np.asarray(cw) * (d[u] + d[v] - 2.0 * S[a, b])


def greedy(n, fi, fj, fw, ci, cj, cw, K, fold=64):
    """(order, gains, margins): margins[k] = relative gap between the best and the second-best unselected score at step k
    (inf when only one is left)."""
    Sig, _ = initial_sigma(n, fi, fj, fw)
    npr = n - 1
    cw = np.asarray(cw, dtype=np.float64)
    u, v = np.asarray(ci) - 1, np.asarray(cj) - 1
    m = len(cw)
    s = scores(Sig, ci, cj, cw)
    sel = np.zeros(m, dtype=bool)
    Zb = np.zeros((npr + 1, fold))          # row npr stays 0: node 0
    cb = np.zeros(fold)
    Sp = np.zeros((npr + 1, npr))
    Sp[:npr] = Sig
    order, gains, margins = [], [], []
    for k in range(K):
        masked = np.where(sel, -np.inf, s)
        e = int(np.argmax(masked))
        best = masked[e]
        masked[e] = -np.inf
        second = masked.max() if m - k > 1 else -np.inf
        margins.append((best - second) / abs(best) if np.isfinite(second) and best != 0 else np.inf)
        j = k % fold
        alpha = cb[:j] * (Zb[u[e], :j] - Zb[v[e], :j])
        z = Sp[u[e]] - Sp[v[e]] - Zb[:npr, :j] @ alpha
        c = cw[e] / (1.0 + best)
        Zb[:npr, j] = z
        cb[j] = c
        zz = np.append(z, 0.0)
        s = s - cw * c * (zz[u] - zz[v]) ** 2
        sel[e] = True
        order.append(e)
        gains.append(best)
        if j == fold - 1:
            Sp[:npr] -= (Zb[:npr] * cb) @ Zb[:npr].T
            Zb[:] = 0.0
            cb[:] = 0.0
    return np.array(order), np.array(gains), np.array(margins)


def logdet_sparse(L):
    """log det of a sparse SPD matrix by SuperLU (det > 0: the sum of log |U_ii|)."""
    from scipy.sparse.linalg import splu
    lu = splu(sp.csc_matrix(L), permc_spec="COLAMD", diag_pivot_thresh=0.0)
    return float(np.sum(np.log(np.abs(lu.U.diagonal()))))
