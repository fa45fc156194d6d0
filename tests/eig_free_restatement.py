"""NumPy restatement of GreedyEig's matrix-free preconditioner (mac_amd/csrc/eig_free.h), written from its header comment for the
tests -- a model for tests/eig_lobpcg_restatement.py (``Q.select(g, K, batch, M=ChainFree(...))``), not a port of any kernel.

``ChainFree`` is the route's algebra.  Sigma0 of the chain is never formed: with R the prefix sums of 1 / w_link and
d_t = R[t] - R[t-1],
    (Sigma0 q)_a = sum_{t <= a} d_t s_t,      s_t = sum_{b >= t} q_b,
in chunks of ``rows`` rows over [0, ld): a chunk's suffix carry is the later chunks' sums of q, its prefix carry the earlier chunks'
sums of u_t = d_t s_t.  The picks stay in a history Zb (n' x j), cb that is never folded:
    T = Sigma0 Q - Zb (diag(cb) Zb^T Q),      z_e = Sigma0 a_e - Zb (diag(cb) Zb^T a_e),      c_e = w_e / (1 + w_e a_e^T z_e),
the projection Zb^T Q summed over ``split`` row slices of per = ceil(ld / 32 / split) * 32 rows.  ``damage=`` breaks one term:
    scan_carry     one chunk's prefix carry is dropped (the middle chunk's)
    history_tail   the last j mod 4 history columns are missing from the projection and the back-substitution (the k-loop's tail)
    history_block  the history columns 64.. are missing (the second 64-column tile)
    slice_lost     one row slice (the second) is missing from the projection
    no_cand        the column's own c_e z_e z_e^T term is dropped
    no_pending     the history is ignored by the application
    pad_rows       every operand is carried with ld rows: Sigma0 = identity on the rows n'..ld, where r, a_e, z_e and Zb are 0 -- the
                   same numbers unless something leaks into or out of the padding

A damaged variant that runs into the 500-iteration cap counts as infinite at every pick it is active at (``Q.excess``).  Such a run
costs up to 500 iterations of a whole batch, so ``reference`` first asks ``hits_cap_alone``: the 16 columns with the largest bounds at
the variant's first active pick -- part of that pick's first batch whatever the batch size (>= 16) -- solved alone from the Fiedler
vector of the graph after the exact run's earlier picks (the variant is inactive before, so they are its picks too).  Columns of a
batch are independent, so if they hit the cap alone the whole run does, and it is not made; if they converge, the whole run decides
(scan_carry and slice_lost fail in every column and are caught; no_pending and history_tail fail in a few columns at a later pick).
"""
import functools

import numpy as np

import eig_lobpcg_restatement as Q
import eig_restatement as R

DAMAGES = ("scan_carry", "history_tail", "history_block", "slice_lost", "no_cand", "no_pending", "pad_rows")
ROWS, SPLIT = 32, 3          # the options the device test forces beside the automatic ones
PANEL = 32


def chain_resistances(L0):
    """R[i] = resistance from node 0 to node i + 1 along the chain L0 is the Laplacian of (asserted)."""
    n = L0.shape[0]
    link = -np.diag(L0, 1)
    assert np.all(link > 0.0) and np.allclose(L0, R.laplacian(n, np.arange(n - 1), np.arange(1, n), link), rtol=0, atol=0)
    return np.cumsum(1.0 / link)


def scan_apply(Rp, A, rows, ld=None, lost=None):
    """Sigma0 A by the two chunked scans; ``lost``: the chunk whose prefix carry is dropped."""
    npn, B = A.shape
    ld = (npn + 63) // 64 * 64 if ld is None else ld
    Qp = np.zeros((ld, B))
    Qp[:npn] = A
    d = np.zeros(ld)
    d[:npn] = np.diff(np.concatenate([[0.0], Rp]))
    if ld % rows == 0:                               # whole chunks: the same sums, all chunks at once
        nch = ld // rows
        Qc, dc = Qp.reshape(nch, rows, B), d.reshape(nch, rows, 1)
        cs = Qc.sum(axis=1)
        carry = np.cumsum(cs[::-1], axis=0)[::-1] - cs                      # the later chunks' sums
        U = dc * (carry[:, None, :] + np.cumsum(Qc[:, ::-1], axis=1)[:, ::-1])
        cu = U.sum(axis=1)
        top = np.cumsum(cu, axis=0) - cu                                   # the earlier chunks' sums
        if lost is not None and lost < nch:
            top[lost] = 0.0
        return (top[:, None, :] + np.cumsum(U, axis=1)).reshape(ld, B)[:npn]
    cuts = [(a, min(ld, a + rows)) for a in range(0, ld, rows)]
    cs = [Qp[a:b].sum(axis=0) for a, b in cuts]
    U = np.zeros((ld, B))
    for c, (a, b) in enumerate(cuts):
        carry = np.sum(cs[c + 1:], axis=0) if c + 1 < len(cuts) else np.zeros(B)
        U[a:b] = d[a:b, None] * (carry + np.cumsum(Qp[a:b][::-1], axis=0)[::-1])
    cu = [U[a:b].sum(axis=0) for a, b in cuts]
    out = np.zeros((ld, B))
    for c, (a, b) in enumerate(cuts):
        top = np.sum(cu[:c], axis=0) if c and c != lost else np.zeros(B)
        out[a:b] = top + np.cumsum(U[a:b], axis=0)
    return out[:npn]


class ChainFree:
    """The matrix-free route's algebra, one term of which ``damage`` breaks."""
    fold = None

    def __init__(self, damage=None, rows=ROWS, split=SPLIT, ld=None):
        assert damage is None or damage in DAMAGES
        self.damage, self.rows, self.split, self.ld = damage, rows, split, ld

    @property
    def pending(self):
        return len(self.cb)

    def reset(self, L0):
        self.Rp = chain_resistances(L0)
        self.np = len(self.Rp)
        if self.ld is None:
            self.ld = (self.np + 63) // 64 * 64
        self.Zb, self.cb, self._kept = [], [], None

    def _pad(self, A):
        """pad_rows: node-space columns with the rows n'..ld as explicit entries."""
        if self.damage != "pad_rows" or A.shape[0] == self.ld:
            return A
        return np.vstack([A, np.zeros((self.ld - A.shape[0], A.shape[1]))])

    def _sig0(self, A):
        nch = (self.ld + self.rows - 1) // self.rows
        T = scan_apply(self.Rp, A[:self.np], self.rows, self.ld, lost=nch // 2 if self.damage == "scan_carry" else None)
        return np.vstack([T, A[self.np:]])           # (pad_rows: identity on the padding; otherwise nothing to stack)

    def _cols(self):
        """The history columns the two matrix products see."""
        j = len(self.cb)
        if self.damage == "history_tail":
            j -= j % 4
        if self.damage == "history_block":
            j = min(j, 64)
        return j

    def _arrays(self, j):
        """Zb (rows x j) and cb of the first j history columns (kept until the next push)."""
        if self._kept is None or self._kept[0] != (j, len(self.cb)):
            self._kept = ((j, len(self.cb)), np.array(self.Zb[:j]).T, np.array(self.cb[:j]))
        return self._kept[1], self._kept[2]

    def _history(self, A, project_rows=None):
        j = self._cols()
        if j == 0:
            return 0.0
        Zb, cb = self._arrays(j)
        Zp = Zb
        if project_rows is not None:                 # slice_lost: the rows of one slice are missing from Zb^T Q
            Zp = Zb.copy()
            Zp[project_rows[0]:project_rows[1]] = 0.0
        return Zb @ (cb[:, None] * (Zp.T @ A))

    def _z(self, A):
        """alpha is a gather, not the projection kernel: only the back-substitution's damages reach z."""
        j = self._cols()
        Z = self._sig0(A)
        if j:
            Zb, cb = self._arrays(j)
            Z = Z - Zb @ (cb[:, None] * (Zb.T @ A))
        return Z

    def push(self, n, u, v, w):
        A = self._pad(Q.incidence(n, [u], [v]))
        z = self._z(A)[:, 0]
        self.Zb.append(z)
        self.cb.append(float(w / (1.0 + w * float(A[:, 0] @ z))))

    def fold_now(self): pass

    def columns(self, L, U, V, w):
        n = L.shape[0]
        A = self._pad(Q.incidence(n, U, V))
        Z = self._z(A)
        w = np.asarray(w, dtype=np.float64)
        cc = w / (1.0 + w * np.sum(A * Z, axis=0))
        if self.damage == "no_cand":
            cc = np.zeros_like(cc)
        lost = None
        if self.damage == "slice_lost":
            per = (self.ld // PANEL + self.split - 1) // self.split * PANEL
            lost = (per, 2 * per)

        def apply(act, Rr):
            Rr = self._pad(Rr)
            T = self._sig0(Rr)
            if self.damage != "no_pending":
                T = T - self._history(Rr, lost)
            T = T - Z[:, act] * (cc[act] * np.sum(Z[:, act] * Rr, axis=0))[None, :]
            return T[:n - 1]
        return apply


# ---- the inputs the host and the device module share ----
K_LONG = 68
LONG_SEED = 0


@functools.lru_cache(maxsize=None)
def graph(name):
    """chain150 / chain129 of eig_lobpcg_restatement; long66: 66 nodes (n' = 65, ld = 128: padding rows), about 200 candidates, for a
    history that passes every remainder mod 4 and crosses 64 columns."""
    if name == "long66":
        return Q.chain_er(66, 0.1, LONG_SEED)
    return Q.graph(name)


CASES = [("chain150", Q.K_PICKS, 512), ("chain150", Q.K_PICKS, 64), ("chain129", Q.K_PICKS, 512), ("chain129", Q.K_PICKS, 64),
         ("long66", K_LONG, 512)]
PROBE = 16


def variants(K, ld, rows=ROWS, split=SPLIT):
    """{damage: the picks it can differ at}: pick k sees a history of k columns."""
    k = np.arange(K)
    per = (ld // PANEL + split - 1) // split * PANEL
    act = {"no_cand": k >= 0, "no_pending": k > 0, "scan_carry": (k >= 0) & (ld > rows), "history_tail": k % 4 > 0,
           "history_block": k > 64, "slice_lost": (k > 0) & (per < ld)}
    return {d: a for d, a in act.items() if a.any()}


def ld_of(name):
    return (graph(name)[0] - 1 + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def exact(name, K, batch):
    return Q.select(graph(name), K, batch=batch)


def state_at(name, K, batch, damage, k0):
    """What ``Q.select`` holds when a variant that is inactive before pick k0 arrives there: the graph after the exact run's first k0
    picks, the model with those picks pushed, and the Fiedler pair (numpy.linalg.eigh's: the run's own polished pair to rounding)."""
    import eig_exchange_restatement as E
    n, fi, fj, fw, ci, cj, cw = graph(name)
    ci, cj, cw = np.asarray(ci, dtype=np.int64), np.asarray(cj, dtype=np.int64), np.asarray(cw, dtype=np.float64)
    before = exact(name, K, batch)["order"][:k0]
    L = R.laplacian(n, fi, fj, fw)
    M = ChainFree(damage)
    M.reset(L)
    for e in before:
        M.push(n, ci[e], cj[e], cw[e])
        L = L + E.edge_lap(n, ci[e], cj[e], cw[e])
    lam, v = R.fiedler(L)
    sel = np.zeros(len(cw), dtype=bool)
    sel[before] = True
    return n, ci, cj, cw, L, M, lam, v, sel


def hits_cap_alone(name, K, batch, damage, k0):
    """True if the PROBE columns with the largest bounds at pick k0, solved alone with the damaged model, hit the iteration cap."""
    n, ci, cj, cw, L, M, lam, v, sel = state_at(name, K, batch, damage, k0)
    u = lam + cw * (v[ci] - v[cj]) ** 2
    unsel = np.flatnonzero(~sel)
    es = unsel[np.argsort(-u[unsel], kind="stable")][:PROBE]
    try:
        Q.solve_columns(L, ci[es], cj[es], cw[es], v, M.columns(L, ci[es], cj[es], cw[es]))
    except Q.NotConverged:
        return True
    return False


def applications_from(name, K, batch, damage, k0):
    """The applications per pick of ``Q.select(graph, K, batch, M=ChainFree(damage))`` for the picks k0.. (nan before), for a variant
    that is inactive before k0: the loop of ``Q.select``, entered at pick k0 from ``state_at`` instead of replaying k0 picks that are
    the undamaged run's.  The start vector differs from the replay's by rounding (start noise of 1e-9 moves a count by 3 at most)."""
    import eig_exchange_restatement as E
    n, ci, cj, cw, L, M, lam, v, sel = state_at(name, K, batch, damage, k0)
    apps = np.full(K, np.nan)
    for k in range(k0, K):
        u = lam + cw * (v[ci] - v[cj]) ** 2
        unsel = np.flatnonzero(~sel)
        order = unsel[np.argsort(-u[unsel], kind="stable")]
        top, napp = -np.inf, 0
        l2 = np.full(len(cw), np.nan)
        last, lastX = np.zeros(0, dtype=np.int64), None
        for q in range(0, len(order), batch):
            if u[order[q]] < top:
                break
            es = order[q:q + batch]
            r = Q.solve_columns(L, ci[es], cj[es], cw[es], v, M.columns(L, ci[es], cj[es], cw[es]))
            l2[es] = r["lam"]
            top = max(top, float(r["lam"].max()))
            napp += r["napp"]
            last, lastX = es, r["X"]
        best = R.scan(l2)[0]
        assert best >= 0
        at = np.flatnonzero(last == best)
        one = ([ci[best]], [cj[best]], [cw[best]])
        r = Q.solve_columns(L, *one, lastX[:, at[0]] if len(at) else v, M.columns(L, *one), polish=True)
        apps[k] = napp + r["napp"]
        lam, v = float(r["lam"][0]), r["X"][:, 0]
        M.push(n, ci[best], cj[best], cw[best])
        sel[best] = True
        L = L + E.edge_lap(n, ci[best], cj[best], cw[best])
    return apps


@functools.lru_cache(maxsize=None)
def reference(name, K, batch):
    """dict(run: the exact replay, A: its applications per pick, excess: {damage: A_damaged - A on the picks it is active at}, D:
    the smallest excess of any active variant per pick)."""
    run = exact(name, K, batch)
    A = run["applications"].astype(np.float64)
    ex = {}
    for d, act in variants(K, ld_of(name)).items():
        k0 = int(np.flatnonzero(act)[0])
        if hits_cap_alone(name, K, batch, d, k0):
            ex[d] = np.where(act, np.inf, np.nan)
        elif k0 >= 8:            # (a long inactive prefix: enter the loop at pick k0 instead of replaying the undamaged picks)
            ex[d] = Q.excess(A, lambda: applications_from(name, K, batch, d, k0), act)
        else:
            ex[d] = Q.excess(A, lambda: Q.select(graph(name), K, batch=batch, M=ChainFree(d))["applications"], act)
    return dict(run=run, A=A, excess=ex, D=np.nanmin(np.array(list(ex.values())), axis=0))
