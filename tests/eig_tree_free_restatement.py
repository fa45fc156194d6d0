"""NumPy restatement of GreedyEig's matrix-free preconditioner over a spanning tree (mac_amd/csrc/eig_free_tree.h), written from
its header comment for the tests -- a model for tests/eig_lobpcg_restatement.py (``Q.select(g, K, batch, M=TreeFree(g, ...))``), not a
port of any kernel.

``TreeFree`` is the route's algebra.  The plan (the BFS tree T from node 0, preorder numbers, subtree ends, the seeds) is
tests/esp_tree_restatement.py's.  Sigma0(T) is never formed: in preorder, with d_p = 1 / w(link above p),
    s_p = S(p) - S(end_p + 1),   S(p) = sum_{p' >= p} q_p',      u_p = d_p s_p,
    T_p = the prefix over the Euler tour of (+u_a on entering a, -u_a on leaving a), read at p's entry,
the rows in chunks of ``rows`` over [0, ld) and the tour in chunks of 2 ``rows`` events: a row chunk's suffix carry is the later
chunks' sums of q, a tour chunk's prefix carry the earlier chunks' sums of +-u, each added in ascending chunk order.  The r seeds are
pushed in ``reset`` as history columns [0, r), the picks follow; history, projection and back-substitution as
tests/eig_free_restatement.py's ``ChainFree`` with j = r + picks.  ``damage=`` breaks one term:
    sub_end        the - S(end_p + 1) term is dropped
    no_close       the tour's -u events are dropped: the chain formula on a tree
    down_carry     one tour chunk's prefix carry is dropped (the middle chunk's)
    up_carry       one row chunk's suffix carry is dropped (the middle chunk's)
    no_seeds       the seeds are not in the history
    history_tail, history_block, slice_lost, no_cand, no_pending, pad_rows      as in eig_free_restatement, j counted from r

A damaged variant that runs into the 500-iteration cap counts as infinite at every pick it is active at; ``reference`` asks
``hits_cap_alone`` first (eig_free_restatement explains the probe), so that a capped variant is not replayed in full.  A case's
reference still costs 10 to 20 s of CPU time, so what the device module needs of it -- the exact run's picks, solved counts and
applications A, and D -- is recorded in tests/golden/eig_tree_free_reference.json (``recorded``; written by ``python
tests/eig_tree_free_restatement.py``); tests/test_eig_tree_free_host.py recomputes every case and compares.
"""
import functools
import json
import os

import numpy as np

import eig_exchange_restatement as E
import eig_free_restatement as F
import eig_lobpcg_restatement as Q
import eig_restatement as R
import esp_tree_restatement as TR

DAMAGES = ("sub_end", "no_close", "down_carry", "up_carry", "no_seeds", "history_tail", "history_block", "slice_lost", "no_cand",
           "no_pending", "pad_rows")
ROWS, SPLIT, PANEL = F.ROWS, F.SPLIT, F.PANEL


def tables(n, P):
    """dict(node_of, end (by preorder number), d (by preorder number), tour: (preorder number, sign) per event) of a plan."""
    pre, end = np.asarray(P["pre"]), np.asarray(P["end"])
    node_of = np.zeros(n, dtype=np.int64)
    node_of[pre] = np.arange(n)
    d = np.zeros(n)
    d[1:] = (P["R"] - P["R"][np.maximum(P["parent"], 0)])[node_of[1:]]
    endp = end[node_of]
    ev, stack = [], []
    for p in range(1, n):
        while stack and endp[stack[-1]] < p:
            ev.append((stack.pop(), -1.0))
        ev.append((p, 1.0))
        stack.append(p)
    while stack:
        ev.append((stack.pop(), -1.0))
    return dict(node_of=node_of, end=endp, d=d, tour_p=np.array([e[0] for e in ev], dtype=np.int64).reshape(-1),
                tour_s=np.array([e[1] for e in ev]).reshape(-1))


def _running(carry, X):
    """carry, carry + X[0], (carry + X[0]) + X[1], ...: a chunk walked row after row from its carry."""
    return np.cumsum(np.vstack([carry[None, :], X]), axis=0)[1:]


def sweep_apply(n, Tb, A, rows, ld=None, damage=None):
    """Sigma0(T) A (A: n' x B in reduced node order) by the four chunked sweeps."""
    npn, B = A.shape
    assert npn == n - 1
    ld = (npn + 63) // 64 * 64 if ld is None else ld
    rowof = Tb["node_of"][1:] - 1                            # batch row of the preorder row k = p - 1
    Ap = A[rowof]
    cuts = [(a, min(npn, a + rows)) for a in range(0, ld, rows)]
    cs = [Ap[a:b].sum(axis=0) if a < b else np.zeros(B) for a, b in cuts]
    lost_up = len(cuts) // 2 if damage == "up_carry" else None
    S = np.zeros((npn + 1, B))                               # S[k] = S(k + 1); S[n'] = 0: past the last row
    for c, (a, b) in enumerate(cuts):
        if a >= b:
            continue
        carry = np.zeros(B)
        if c != lost_up:
            for c2 in range(c + 1, len(cuts)):
                carry = carry + cs[c2]
        S[a:b] = _running(carry, Ap[a:b][::-1])[::-1]
    p, sg = Tb["tour_p"], Tb["tour_s"]
    s = S[p - 1]
    if damage != "sub_end":
        s = s - S[np.minimum(Tb["end"][p], npn)]
    ev = sg[:, None] * (Tb["d"][p][:, None] * s)
    if damage == "no_close":
        ev = np.where(sg[:, None] > 0, ev, 0.0)
    nev = len(p)
    tcuts = [(a, min(nev, a + 2 * rows)) for a in range(0, nev, 2 * rows)]
    ct = [ev[a:b].sum(axis=0) for a, b in tcuts]
    lost_down = len(tcuts) // 2 if damage == "down_carry" else None
    run = np.zeros((nev, B))
    for c, (a, b) in enumerate(tcuts):
        carry = np.zeros(B)
        if c != lost_down:
            for c2 in range(c):
                carry = carry + ct[c2]
        run[a:b] = _running(carry, ev[a:b])
    out = np.zeros((npn, B))
    enter = sg > 0
    out[rowof[p[enter] - 1]] = run[enter]
    return out


class TreeFree:
    """The spanning-tree route's algebra, one term of which ``damage`` breaks."""
    fold = None

    def __init__(self, g, damage=None, rows=ROWS, split=SPLIT, ld=None):
        assert damage is None or damage in DAMAGES
        self.n, self.fixed = g[0], tuple(g[1:4])
        self.damage, self.rows, self.split, self.ld = damage, rows, split, ld
        self.P = TR.plan(self.n, *self.fixed)
        self.Tb = tables(self.n, self.P)
        self.seeds = len(self.P["seeds"][2])

    @property
    def pending(self):
        return len(self.cb)

    def reset(self, L0):
        assert L0.shape[0] == self.n and np.allclose(L0, R.laplacian(self.n, *self.fixed), rtol=1e-13, atol=0)
        self.np = self.n - 1
        if self.ld is None:
            self.ld = (self.np + 63) // 64 * 64
        self.Zb, self.cb, self._kept = [], [], None
        if self.damage != "no_seeds":
            for u, v, w in zip(*self.P["seeds"]):
                self.push(self.n, int(u), int(v), float(w))

    def _pad(self, A):
        if self.damage != "pad_rows" or A.shape[0] == self.ld:
            return A
        return np.vstack([A, np.zeros((self.ld - A.shape[0], A.shape[1]))])

    def _sig0(self, A):
        T = sweep_apply(self.n, self.Tb, A[:self.np], self.rows, self.ld, self.damage)
        return np.vstack([T, A[self.np:]])           # (pad_rows: identity on the padding; otherwise nothing to stack)

    def _cols(self):
        j = len(self.cb)
        if self.damage == "history_tail":
            j -= j % 4
        if self.damage == "history_block":
            j = min(j, 64)
        return j

    def _arrays(self, j):
        if self._kept is None or self._kept[0] != (j, len(self.cb)):
            self._kept = ((j, len(self.cb)), np.array(self.Zb[:j]).T, np.array(self.cb[:j]))
        return self._kept[1], self._kept[2]

    def _history(self, A, project_rows=None):
        j = self._cols()
        if j == 0:
            return 0.0
        Zb, cb = self._arrays(j)
        Zp = Zb
        if project_rows is not None:
            Zp = Zb.copy()
            Zp[project_rows[0]:project_rows[1]] = 0.0
        return Zb @ (cb[:, None] * (Zp.T @ A))

    def _z(self, A):
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
def _deep(n):
    """A permuted chain with chords: relabelled, and its first 5 candidates moved to the end of the fixed list (5 seeds)."""
    n, fi, fj, fw, ci, cj, cw = Q.chain_er(n, 0.02, 3)
    perm = np.random.default_rng(103).permutation(n)
    fi, fj, ci, cj = perm[fi], perm[fj], perm[ci], perm[cj]
    return (n, np.concatenate([fi, ci[:5]]), np.concatenate([fj, cj[:5]]), np.concatenate([fw, cw[:5]]), ci[5:], cj[5:], cw[5:])


@functools.lru_cache(maxsize=None)
def graph(name):
    """general150: eig_lobpcg_restatement's (74 seeds, depth 8, ld 192: six row chunks of 32, padding rows, a history that starts
    beyond one 64-column tile).  deep150 / deep129: 5 seeds, depths 38 / 44; deep129 has n' = ld = 128, no padding."""
    if name in ("deep150", "deep129"):
        return _deep(int(name[4:]))
    return Q.graph(name)


NAMES = ("general150", "deep150", "deep129")
CASES = [(name, Q.K_PICKS, batch) for name in NAMES for batch in (512, 64)]
PROBE = F.PROBE


def ld_of(name):
    return (graph(name)[0] - 1 + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def model_facts(name):
    """(r, depth, tour events) of an input."""
    g = graph(name)
    M = TreeFree(g)
    depth = np.zeros(g[0], dtype=np.int64)
    for x in M.P["order"][1:]:
        depth[x] = depth[M.P["parent"][x]] + 1
    return M.seeds, int(depth.max()), len(M.Tb["tour_p"])


def variants(name, K, rows=ROWS, split=SPLIT):
    """{damage: the picks it can differ at}: pick k sees a history of r + k columns."""
    r, _, nev = model_facts(name)
    ld = ld_of(name)
    k = np.arange(K)
    j = r + k
    per = (ld // PANEL + split - 1) // split * PANEL
    always = k >= 0
    act = {"sub_end": always, "no_close": always, "down_carry": always & (nev > 2 * rows), "up_carry": always & (ld > rows),
           "no_seeds": always & (r > 0), "no_cand": always, "no_pending": j > 0, "history_tail": j % 4 > 0, "history_block": j > 64,
           "slice_lost": (j > 0) & (per < ld)}
    return {d: a for d, a in act.items() if a.any()}


@functools.lru_cache(maxsize=None)
def exact(name, K, batch):
    return Q.select(graph(name), K, batch=batch)


def state_at(name, K, batch, damage, k0):
    """What ``Q.select`` holds when a variant that is inactive before pick k0 arrives there (eig_free_restatement.state_at)."""
    g = graph(name)
    n, fi, fj, fw, ci, cj, cw = g
    ci, cj, cw = np.asarray(ci, dtype=np.int64), np.asarray(cj, dtype=np.int64), np.asarray(cw, dtype=np.float64)
    before = exact(name, K, batch)["order"][:k0] if k0 else np.zeros(0, dtype=np.int64)
    L = R.laplacian(n, fi, fj, fw)
    M = TreeFree(g, damage)
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


@functools.lru_cache(maxsize=None)
def reference(name, K, batch):
    """dict(run: the exact replay, A: its applications per pick, excess: {damage: A_damaged - A on the picks it is active at}, D:
    the smallest excess of any active variant per pick)."""
    run = exact(name, K, batch)
    A = run["applications"].astype(np.float64)
    ex = {}
    for d, act in variants(name, K).items():
        k0 = int(np.flatnonzero(act)[0])
        if hits_cap_alone(name, K, batch, d, k0):
            ex[d] = np.where(act, np.inf, np.nan)
        else:
            ex[d] = Q.excess(A, lambda: Q.select(graph(name), K, batch=batch, M=TreeFree(graph(name), d))["applications"], act)
    return dict(run=run, A=A, excess=ex, D=np.nanmin(np.array(list(ex.values())), axis=0))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eig_tree_free_reference.json")


@functools.lru_cache(maxsize=None)
def recorded(name, K, batch):
    """dict(order, solved, A, D) of ``reference(name, K, batch)`` as recorded in tests/golden/eig_tree_free_reference.json."""
    with open(GOLDEN) as f:
        rec = json.load(f)[f"{name}:{K}:{batch}"]
    return dict(order=np.array(rec["order"]), solved=np.array(rec["solved"]), A=np.array(rec["A"], dtype=np.float64),
                D=np.array(rec["D"], dtype=np.float64))


if __name__ == "__main__":
    out = {}
    for name, K, batch in CASES:
        ref = reference(name, K, batch)
        out[f"{name}:{K}:{batch}"] = dict(order=ref["run"]["order"].tolist(), solved=ref["run"]["solved"].tolist(), A=ref["A"].tolist(),
                                          D=ref["D"].tolist())
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
