"""GreedyKirchhoff: greedy k-edge selection under the A-optimal criterion -- minimise tr L^+, the total effective resistance of
the graph (Kirchhoff index / n), for a pose graph the quantity proportional to the mean estimation covariance.  The third of
the classical design criteria beside MAC / GreedyEig (E-optimal, lambda_2) and GreedyESP (D-optimal, the spanning-tree count);
no counterpart in the reference.  Hot path on the MI355X (mac_amd/csrc/kirchhoff.h), on GreedyESP's resident dense inverse.

With node 0 pinned and Sigma = L_red^-1, tr L^+ = tr Sigma - (1^T Sigma 1) / n, and adding candidate e = (u, v, w) lowers it by
gain_e = w (|z_e|^2 - (1^T z_e)^2 / n) / (1 + w r_e), z_e = Sigma a_e.  Every step takes the unselected candidate of largest gain
(ties: lowest index) and updates all gains by a rank-1 recurrence that costs one dense product with Sigma.
A-optimality is not submodular: there is no lazy variant.  ``kirchhoff_index`` scores the selection of any solver.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from mac_amd import _lib
from mac_amd.utils.graphs import Edge, edges_to_arrays


class GreedyKirchhoff:
    def __init__(self, fixed_edges: List[Edge], candidate_edges: List[Edge], num_nodes: int, *, device: int = 0, fold: int = 64,
                 dense_inverse: bool = False):
        """``device``, ``fold`` and ``dense_inverse`` as GreedyESP's.  The criterion needs the dense inverse (num_nodes <= 32768 on
        a chain-fixed graph, <= 16384 otherwise) and a connected fixed graph: raises Disconnected when the fixed edges leave more
        than one component (the index is infinite)."""
        self.fixed_edges = fixed_edges
        self.all_candidate_edges = candidate_edges
        self.num_nodes = num_nodes
        self.edge_weights = np.array([edge.weight for edge in candidate_edges])
        fi, fj, fw = edges_to_arrays(fixed_edges)
        ci, cj, cw = edges_to_arrays(candidate_edges)
        self._dev = _lib.Esp(num_nodes, fi, fj, fw, ci, cj, cw, fold=fold, dense_inverse=dense_inverse, device=device)
        if self._dev.info()["beta"] != 0.0:
            self._dev.close()
            raise _lib.Disconnected(_lib.DISCONNECTED, "the fixed graph is disconnected: its Kirchhoff index is infinite")
        self.last_gains: Optional[np.ndarray] = None      # the drop of tr L^+ at every pick of the last run

    def _run(self, ks):
        order, gain, t_ms = self._dev.kirchhoff_select(ks)
        self.last_gains = gain
        return order, t_ms / 1e3

    def subset(self, k: int):
        """(result 0/1 array, selected edges in selection order)."""
        assert k > 0
        assert len(self.all_candidate_edges) >= k
        order, _ = self._run([k])
        result = np.zeros(len(self.all_candidate_edges))
        result[order] = 1.0
        return result, [self.all_candidate_edges[i] for i in order]

    def subsets(self, ks: List[int]) -> Tuple[List[np.ndarray], List[Edge], List[float]]:
        """One greedy run for all budgets (increasing): (0/1 arrays per budget, the selected edges of the largest budget in
        selection order, device seconds from the start until each budget was reached) -- as GreedyESP.subsets_lazy returns."""
        ks = [int(k) for k in ks]
        assert all(ks[i] <= ks[i + 1] for i in range(len(ks) - 1)), "budgets must be monotonically increasing"
        assert len(self.all_candidate_edges) >= ks[-1], "Not enough candidate edges to satisfy the largest budget"
        assert ks[0] > 0, "budgets must be positive"
        order, times = self._run(ks)
        results = []
        for k in ks:
            r = np.zeros(len(self.all_candidate_edges))
            r[order[:k]] = 1.0
            results.append(r)
        return results, [self.all_candidate_edges[i] for i in order], [float(t) for t in times]

    def gains(self) -> np.ndarray:
        """The drop of tr L^+ each candidate (selected ones included) would bring to the fixed graph plus the last run's
        selections, re-scored exactly from the inverse; after construction: to the fixed graph."""
        return self._dev.kirchhoff_gains()

    def kirchhoff_index(self, selection=None) -> float:
        """tr L^+ of the fixed graph plus ``selection``: a 0/1 array of length m or a sequence of candidate indices (each at most
        once, any order); None: the fixed graph alone.  Computed from the inverse itself, not from summed gains.  Afterwards
        ``gains()`` refers to the fixed graph plus this selection."""
        m = len(self.all_candidate_edges)
        if selection is None:
            return self._dev.kirchhoff_eval([])[0]
        sel = np.asarray(selection)
        if sel.ndim != 1:
            raise ValueError("selection must be a 0/1 array of length m or a sequence of candidate indices")
        if len(sel) == m and set(np.unique(sel).tolist()) <= {0, 1}:
            sel = np.flatnonzero(sel)
        elif len(sel) and sel.dtype.kind not in "iu":
            raise ValueError("selection must be a 0/1 array of length m or a sequence of candidate indices")
        return self._dev.kirchhoff_eval(sel)[1]

    def info(self) -> dict:
        """How the inverse was built: form ("chain" / "dense"), leading dimension, fold, pending updates, beta, seeds."""
        return self._dev.info()
