"""GreedyESP: greedy k-edge selection by weighted effective resistance (Khosoussi et al., arXiv:1604.01116, Algorithm 1), the
baseline MAC is compared against -- same public surface as the reference class (mac/solvers/greedy_esp.py), hot path on the
MI355X (mac_amd/csrc/esp.h).

The reference keeps a CHOLMOD factor of the reduced Laplacian and updates it per pick; here (L_red + beta I)^-1 is resident
on the GPU (dense fp64) and every pick is a device-side argmax plus a rank-1 update: one call runs all budgets.  The reference's
lazy path (a heap kept exact by submodularity) selects the same sequence as its plain path up to the order inside exact ties,
so ``lazy`` only changes the shape of the return values, as in the reference.  Ties go to the lowest candidate index.

(This module is deliberately not called ``greedy_esp``: the import-compatibility package aliases ``mac.solvers`` to
``mac_amd.solvers``, so the reference's ``from mac.solvers.greedy_esp import GreedyESP`` would resolve to this file; the
supported line is ``from mac.solvers import GreedyESP``.)
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from mac_amd import _lib
from mac_amd.utils.graphs import Edge, edges_to_arrays, weight_reduced_graph_lap_from_edge_list


def exchange_on(dev, candidate_edges, selection, max_swaps=None, min_gain=1e-9, *, edge=False):
    """``GreedyESP.exchange`` on the handle ``dev`` (a ``_lib.Esp``): shared with ``ESPRelaxation.exchange`` and, with
    ``edge=True`` (the handle's ``exchange_edge`` instead of its ``exchange``), with ``ESPRelaxation.exchange_edge``."""
    if not edge and dev.matrix_free:
        raise ValueError("exchange works on the dense inverse: not available with matrix_free=" + repr(dev.matrix_free))
    m = len(candidate_edges)
    sel = np.asarray(selection)
    if sel.ndim != 1:
        raise ValueError("selection must be a 0/1 array of length m or a sequence of candidate indices")
    if len(sel) == m and set(np.unique(sel).tolist()) <= {0, 1}:
        sel = np.flatnonzero(sel)
    elif sel.dtype.kind not in "iu":
        raise ValueError("selection must be a 0/1 array of length m or a sequence of candidate indices")
    if max_swaps is None:
        max_swaps = 10 * len(sel)
    r = (dev.exchange_edge if edge else dev.exchange)(sel, max_swaps, min_gain)
    result = np.zeros(m)
    result[r["selection"]] = 1.0
    info = {"swaps": r["swaps"], "out": r["out"], "in": r["in"], "ratios": r["ratios"],
            "growth": float(np.sum(np.log(r["ratios"]))), "converged": bool(r["converged"]), "seconds": float(r["t_ms"][0]) / 1e3,
            "phase_seconds": r["t_ms"][1:] / 1e3}
    return result, [candidate_edges[i] for i in r["selection"]], info


class GreedyESP:
    def __init__(self, fixed_edges: List[Edge], candidate_edges: List[Edge], num_nodes: int, lazy: bool = False, *,
                 device: int = 0, fold: int = 64, dense_inverse: bool = False, matrix_free=False):
        """Arguments as mac/solvers/greedy_esp.py of the reference, plus keyword-only ``device`` (GPU ordinal), ``fold``
        (pending rank-1 updates folded into the inverse every ``fold`` picks, 1..256) and ``dense_inverse`` (build the
        inverse by dense Gauss-Jordan even when the fixed edges are a chain: cross-checks) and ``matrix_free`` (chain-fixed
        graphs only: no dense inverse, no folds (``fold`` is not used) and no limit on num_nodes; the picks' updates are kept as a history of num_nodes x k
        doubles, so the route is for k << num_nodes -- DESIGN section 14; ``matrix_free="tree"``: the same route for any
        connected fixed graph, from a spanning tree of it plus one history column per fixed link outside the tree -- DESIGN
        section 15).  Raises Disconnected when the fixed graph is
        disconnected and a node other than 0 has no fixed edge (the reference re-raises CHOLMOD's error)."""
        if num_nodes == 0:
            assert len(fixed_edges) == len(candidate_edges) == 0
        self.L_fixed = weight_reduced_graph_lap_from_edge_list(fixed_edges, num_nodes)
        self.fixed_edges = fixed_edges
        self.all_candidate_edges = candidate_edges
        self.num_nodes = num_nodes
        self.edge_weights = np.array([edge.weight for edge in candidate_edges])
        self.lazy = lazy
        fi, fj, fw = edges_to_arrays(fixed_edges)
        ci, cj, cw = edges_to_arrays(candidate_edges)
        self._dev = _lib.Esp(num_nodes, fi, fj, fw, ci, cj, cw, fold=fold, dense_inverse=dense_inverse, device=device,
                             matrix_free=matrix_free)
        self.last_gains: Optional[np.ndarray] = None      # s* of every pick of the last run (sum log(1 + gain) = logdet growth)

    def _run(self, ks):
        order, gain, t_ms = self._dev.select(ks)
        self.last_gains = gain
        return order, t_ms / 1e3

    def subset(self, k: int):
        """(result 0/1 array, selected edges); with ``lazy``: (result, selected edges, seconds) like the reference."""
        if self.lazy:
            return self.subset_lazy(k)
        assert k > 0
        assert len(self.all_candidate_edges) >= k
        order, _ = self._run([k])
        result = np.zeros(len(self.all_candidate_edges))
        result[order] = 1.0
        return result, [self.all_candidate_edges[i] for i in order]

    def subsets_lazy(self, ks: List[int], verbose=False) -> Tuple[List[np.ndarray], List[Edge], List[float]]:
        """One greedy run for all budgets (increasing): (0/1 arrays per budget, the selected edges of the largest budget in
        selection order, device seconds from the start until each budget was reached)."""
        ks = [int(k) for k in ks]
        assert all(ks[i] <= ks[i + 1] for i in range(len(ks) - 1)), "budgets must be monotonically increasing"
        assert len(self.all_candidate_edges) >= ks[-1], "Not enough candidate edges to satisfy the largest budget"
        assert ks[0] > 0, "budgets must be positive"
        if verbose:
            print(f"Running GreedyESP for budgets={ks}")
        order, times = self._run(ks)
        results = []
        for k in ks:
            r = np.zeros(len(self.all_candidate_edges))
            r[order[:k]] = 1.0
            results.append(r)
        return results, [self.all_candidate_edges[i] for i in order], [float(t) for t in times]

    def subset_lazy(self, k: int, verbose: bool = False):
        results, selected_edges, times = self.subsets_lazy([k], verbose=verbose)
        return results[0], selected_edges, times[0]

    def exchange(self, selection, max_swaps: Optional[int] = None, min_gain: float = 1e-9):
        """Best-swap local search (the Fedorov exchange of D-optimal design) on the log tree count, from ``selection``: a 0/1
        array of length m or a sequence of candidate indices.  Every round takes the (selected, unselected) pair whose swap
        raises the tree count most and stops when no swap raises it by more than a factor 1 + ``min_gain``, or after
        ``max_swaps`` swaps (None: 10 K, a cap, not a tuning).  Returns ``(result, selected_edges, info)``: the 0/1 array, the edges in
        index order, and ``info = dict(swaps, out, in, ratios, growth, converged, seconds)`` -- ``growth`` = sum(log(ratios)), the
        gain of the log tree count in nats; ``seconds`` the device time of the call (``phase_seconds``, beside it: load, pair
        passes, T updates, forced steps, folds -- zeros unless the process option esp_xch_profile is 1; tools/esp_xch_time.py).
        Dense handles with a connected fixed graph only; ValueError on a matrix-free handle."""
        return exchange_on(self._dev, self.all_candidate_edges, selection, max_swaps, min_gain)

    def weighted_resistances(self) -> np.ndarray:
        """w_e r_e of every candidate in the fixed graph plus the last run's selections."""
        return self._dev.weighted_resistances()

    def info(self) -> dict:
        """How the inverse was built: form ("chain" / "dense" / "chain_free" / "tree_free"), leading dimension, fold, pending updates, beta, seeds."""
        return self._dev.info()
