"""GreedyEig: greedy k-edge selection by algebraic connectivity, the third baseline MAC is compared against -- same public
surface as the reference class (mac/solvers/greedy_eig.py), hot path on the MI355X (mac_amd/csrc/eig.h).

Each of the k picks adds the candidate e that maximises lambda_2(L_cur + w_e a_e a_e^T).  A candidate whose supergradient bound
u_e = lambda_2 + w_e (v_i - v_j)^2 (v the current unit Fiedler vector) is below a value already established in the pick cannot
win and is not solved; the others are solved exactly (stop rule ||L_e v - lambda v||_1 / ||L_e||_inf < 1e-8), and the pick is the
reference's scan over them: candidate-index order, a candidate replaces the running best only if it exceeds it by more than
1e-8.  The reference re-factors by Cholesky up- and down-dates, one candidate after the other; here the dense inverse of the
reduced Laplacian is resident on the GPU (the state GreedyESP keeps) and a batch of candidates is one dense fp64 matrix product
per solver iteration.

The fixed (odometry) graph must be connected: the reference factors L_odom with one diagonal entry pinned and no
regularisation, which only means anything for a connected odometry graph; a disconnected one raises ``Disconnected`` here.
Size limits as GreedyESP: 32 768 poses when the fixed edges are exactly the chain (i, i+1), 16 384 otherwise.

``matrix_free=True`` (chain-fixed graphs only) keeps no inverse at all: the chain's inverse applied to a batch is two scans, the
picks are a low-rank correction kept as a history of n x k doubles, and one solver iteration costs 4 n j B flop plus three passes
over the batch instead of 2 n^2 B (mac_amd/csrc/eig_free.h).  No limit on the number of poses but memory; the
picks obey the same rule and stop rule, decided by the sparse Laplacian.  The polish on that route (and on "tree") is
``exchange_free``; ``exchange`` itself stays the dense routes' and refuses a matrix-free handle.

``matrix_free="tree"`` is that route for ANY connected fixed graph -- a chain plus kept closures, odometry whose indices are not
consecutive, a landmark spur, merged sessions: a spanning tree T of the fixed graph takes the chain's place (its inverse applied to
a batch is four sweeps over T in preorder, a fixed number of launches whatever its depth), and the r fixed links outside T enter the
history as its first r columns before the first pick (mac_amd/csrc/eig_free_tree.h).  Nothing of size n x n
exists, so the 16 384-pose limit of the dense route is gone; ``info()`` reports ``form="tree_free"``, ``seeds=r`` and
``pending = r + picks``.  Worth it while r + picks stays well below n.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from mac_amd import _lib
from mac_amd.utils import fiedler as _fiedler
from mac_amd.utils.graphs import Edge, edges_to_arrays, weight_graph_lap_from_edge_list, weight_graph_lap_from_edges


def selection_indices(selection, m):
    """The candidate indices ``selection`` names: a 0/1 array of length m, or a sequence of indices (``GreedyESP.exchange``'s rule
    and its errors; decided before any device is asked for)."""
    sel = np.asarray(selection)
    if sel.ndim != 1:
        raise ValueError("selection must be a 0/1 array of length m or a sequence of candidate indices")
    if len(sel) == m and set(np.unique(sel).tolist()) <= {0, 1}:
        return np.flatnonzero(sel)
    if sel.dtype.kind not in "iu":
        raise ValueError("selection must be a 0/1 array of length m or a sequence of candidate indices")
    return sel


class GreedyEig:
    def __init__(self, odom_measurements: List[Edge], lc_measurements: List[Edge], num_poses: int, *, device: int = 0,
                 batch: int = 512, fold: Optional[int] = None, dense_inverse: bool = False, matrix_free=False):
        """Arguments as mac/solvers/greedy_eig.py of the reference, plus keyword-only ``device`` (GPU ordinal), ``batch``
        (candidates solved together, 1..4096), ``fold`` (picks kept as a low-rank block before they are folded into the
        inverse, 1..256; None: 16), ``dense_inverse`` (build the inverse by dense Gauss-Jordan even for a chain: cross-checks) and
        ``matrix_free`` (no inverse: the fixed edges must be exactly the chain (i, i+1); nothing is folded, so ``fold`` must be
        left at None -- any value is a ValueError: an argument without a meaning is refused, not ignored -- as is ``dense_inverse``;
        ``matrix_free="tree"``: the same for any connected fixed graph, over a spanning tree and its seeds; any other value that is
        not a bool is a ValueError).
        Raises Disconnected when the fixed graph is not connected (``matrix_free="tree"``: the spanning-tree plan's own refusal)."""
        if not isinstance(matrix_free, (bool, np.bool_)) and not (isinstance(matrix_free, str) and matrix_free == "tree"):
            raise ValueError(f'matrix_free must be False, True or "tree", not {matrix_free!r}')
        if matrix_free and fold is not None:
            raise ValueError(f"matrix_free={matrix_free!r} never folds: fold has no meaning on this route (got fold={fold!r}); leave it at None")
        if matrix_free and dense_inverse:
            raise ValueError(f"matrix_free={matrix_free!r} keeps no inverse: it cannot be combined with dense_inverse=True")
        self.L_odom = weight_graph_lap_from_edge_list(odom_measurements, num_poses)
        self.num_poses = num_poses
        self.odom_measurements = odom_measurements
        self.lc_measurements = lc_measurements
        ci, cj, cw = edges_to_arrays(lc_measurements)
        self.weights = cw
        self.edge_list = np.stack([ci, cj], axis=1).astype(np.int64).reshape(-1, 2)
        fi, fj, fw = edges_to_arrays(odom_measurements)
        self._dev = _lib.Eig(num_poses, fi, fj, fw, ci, cj, cw, fold=fold, batch=batch, dense_inverse=dense_inverse, device=device,
                             matrix_free=matrix_free if isinstance(matrix_free, str) else bool(matrix_free))
        self._matrix_free = matrix_free if isinstance(matrix_free, str) else bool(matrix_free)
        self.last_lambda2: Optional[np.ndarray] = None      # lambda_2 after every pick of the last run
        self.last_times: Optional[np.ndarray] = None        # seconds from the start of the last run until each pick

    # ---- the reference's helpers ----
    def find_fiedler_pair(self, L, method="tracemin_lu", tol=1e-8):
        """(lambda_2(L), v_2(L)) by mac_amd.utils.fiedler.find_fiedler_pair."""
        lam, v, _ = _fiedler.find_fiedler_pair(L, method=method, tol=tol)
        return lam, v

    def combined_laplacian(self, w, tol=1e-10):
        """L(w): the fixed edges plus the candidates weighted by w (entries of w not above ``tol`` are dropped)."""
        w = np.asarray(w, dtype=np.float64)
        idx = np.nonzero(w > tol)[0]
        return self.L_odom + weight_graph_lap_from_edges(self.edge_list[idx], w[idx] * self.weights[idx], self.num_poses)

    def grad_from_fiedler(self, fiedler_vec):
        """Supergradient of lambda_2 with respect to w: w_e (v_i - v_j)^2 per candidate."""
        v = np.asarray(fiedler_vec, dtype=np.float64)
        d = v[self.edge_list[:, 0]] - v[self.edge_list[:, 1]]
        return self.weights * d * d

    # ---- selection ----
    def subset(self, k: int, save_intermediate: bool = False) -> Tuple[np.ndarray, List[Edge]]:
        """(solution 0/1 array of length m, the picked edges in pick order).  ``save_intermediate`` is accepted for the
        reference's signature (the reference ignores it as well)."""
        m = len(self.weights)
        solution = np.zeros(m)
        if k == 0:
            self.last_lambda2 = np.zeros(0)
            self.last_times = np.zeros(0)
            return solution, []
        assert 0 < k <= m, "not enough candidate edges to satisfy the budget"
        order, lam, t_ms = self._dev.select(k)
        self.last_lambda2 = lam
        self.last_times = t_ms / 1e3
        solution[order] = 1.0
        return solution, [Edge(int(self.edge_list[e, 0]), int(self.edge_list[e, 1]), float(self.weights[e])) for e in order]

    def exchange(self, selection, max_swaps: Optional[int] = None, min_gain: float = 0.0):
        """Best-swap local search on lambda_2 from ``selection``: a 0/1 array of length m or a sequence of candidate indices.
        Every round takes the (selected, unselected) pair whose swap raises lambda_2 most -- found among the pairs whose
        concavity bound lambda_2(S - e) + w_f (v_i - v_j)^2 (v the Fiedler vector without e) can still win, by the scan ``subset``
        uses: (out, in) index order, a pair replaces the running value, initially lambda_2 + ``min_gain``, only if it exceeds it
        by more than 1e-8 -- and stops when no pair does, or after ``max_swaps`` swaps (None: 10 K, a cap, not a tuning).
        Returns ``(result, selected_edges, info)``: the 0/1 array, the edges in index order, and ``info = dict(swaps: list of
        (out, in), lambda2: swaps + 1 values starting with the given selection's, converged, solved, applies, removal_solves:
        per round the pairs solved exactly, the operator applications and the removal pairs solved, t_ms: wall and device
        milliseconds of the call)``.  Afterwards ``candidate_lambda2``, ``candidate_bounds`` and ``info`` refer to the result
        (DESIGN section 20)."""
        m = len(self.weights)
        sel = selection_indices(selection, m)
        if max_swaps is None:
            max_swaps = 10 * len(sel)
        r = self._dev.exchange(sel, max_swaps, min_gain)
        result = np.zeros(m)
        result[r["selection"]] = 1.0
        info = {"swaps": [(int(a), int(b)) for a, b in zip(r["out"], r["in"])], "lambda2": r["lambda2"], "converged": bool(r["converged"]),
                "solved": r["solved"], "applies": r["applications"], "removal_solves": r["removal_solves"], "t_ms": r["t_ms"]}
        return result, [Edge(int(self.edge_list[e, 0]), int(self.edge_list[e, 1]), float(self.weights[e])) for e in r["selection"]], info

    def exchange_free(self, selection, max_swaps: Optional[int] = None, min_gain: float = 0.0):
        """``exchange`` on a handle made with ``matrix_free=True`` or ``"tree"``: the same rule, scan, tie tolerance, stop rule and
        return triple, on the route's history instead of an inverse -- so it runs past the dense limits.  The selection is loaded
        into the history in blocks of 64 columns; a swap appends two columns; the history has room for ``min(max_swaps, 32)`` swaps
        (process option "eig_xch_free_swaps") and is compacted -- rebuilt from the current selection, nothing solved again -- when
        the next round would not fit.  ``info`` has one more key, ``compactions``.  A handle with the dense inverse is a
        ValueError: ``exchange`` is the entry there."""
        m = len(self.weights)
        sel = selection_indices(selection, m)
        if not getattr(self, "_matrix_free", False):
            raise ValueError("exchange_free works on the history of a matrix_free=True or \"tree\" GreedyEig: "
                             "on this one, which keeps the dense inverse, use exchange")
        if max_swaps is None:
            max_swaps = 10 * len(sel)
        r = self._dev.exchange_free(sel, max_swaps, min_gain)
        result = np.zeros(m)
        result[r["selection"]] = 1.0
        info = {"swaps": [(int(a), int(b)) for a, b in zip(r["out"], r["in"])], "lambda2": r["lambda2"], "converged": bool(r["converged"]),
                "solved": r["solved"], "applies": r["applications"], "removal_solves": r["removal_solves"], "t_ms": r["t_ms"],
                "compactions": r["compactions"]}
        return result, [Edge(int(self.edge_list[e, 0]), int(self.edge_list[e, 1]), float(self.weights[e])) for e in r["selection"]], info

    def candidate_lambda2(self) -> np.ndarray:
        """lambda_2(L_cur + e) of every candidate (NaN for the selected), L_cur = the fixed graph plus the last run's picks."""
        return self._dev.candidate_lambda2()

    def candidate_bounds(self) -> np.ndarray:
        """u_e = lambda_2 + w_e (v_i - v_j)^2 from the current Fiedler pair (NaN for the selected)."""
        return self._dev.candidate_bounds()

    def info(self) -> dict:
        """form ("chain" / "dense" / "chain_free" / "tree_free"), ld, fold, batch, pending, seeds, beta, lambda2 (current), and per pick of the last run:
        ``solved`` (candidates solved exactly) and ``applications`` (operator applications summed over the columns)."""
        return self._dev.info()
