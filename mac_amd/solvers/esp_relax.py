"""ESPRelaxation: the convex relaxation of the k-edge tree-count problem GreedyESP is the greedy for (Khosoussi et al.,
arXiv:1604.01116), solved by Frank-Wolfe on the MI355X (mac_amd/csrc/esp_relax.h).

With node 0 pinned and x in [0, 1]^m, sum x <= k:

    M(x) = L_red(fixed) + beta I + sum_e x_e w_e a_e a_e^T,     F(x) = logdet M(x) - logdet M(0)     (growth in nats)

F is concave and dF/dx_e is the weighted effective resistance of e in the graph weighted by x, so the dual value
F(x) + <dF(x), s - x> (s the top-k vertex of the gradient) bounds the growth of EVERY k-edge selection from above: what
``MAC.solve`` returns for lambda_2, for the tree count.  ``evaluate_objective`` scores any solver's 0/1 selection under this
objective (for a greedy selection it equals ``sum(log1p(GreedyESP.last_gains))``).  The reference has no such solver; the
surface follows ``MAC``: ``solve`` returns the same triple and takes the same shortcut at k >= m.
"""
from __future__ import annotations

from typing import List

import numpy as np

from mac_amd import _lib
from mac_amd.solvers.esp import exchange_on
from mac_amd.utils.graphs import Edge, edges_to_arrays
from mac_amd.utils.rounding import round_madow, round_nearest


class ESPRelaxation:
    def __init__(self, fixed_edges: List[Edge], candidate_edges: List[Edge], num_nodes: int, *, device: int = 0,
                 edge_space=False):
        """Arguments as GreedyESP.  The fixed graph may be disconnected as long as every node other than 0 has a fixed edge
        (beta = 1e-4 then, as in GreedyESP); num_nodes <= 16384 (the dense M(x) is inverted per evaluation).

        edge_space=True: the same relaxation carried out in the space of the candidates (mac_amd/csrc/esp_relax_edge.h).  With G
        the candidates' Gram matrix under the chain's resistances and D = diag(w x), F(x) = logdet(I + G D) and the gradient is
        w_e [(I + G D)^-1 G]_ee: an m x m inverse per evaluation instead of an (n - 1) x (n - 1) one.  Regime: the fixed edges are
        exactly the connected chain (i, i+1) (parallel links summed), at most 16384 candidates, any num_nodes.  Same results to
        rounding, not the same bits: the default stays node space.

        edge_space="tree": edge space for any connected fixed graph (mac_amd/csrc/esp_relax_edge_tree.h).  The Gram matrix comes
        from the spanning tree GreedyESP(matrix_free="tree") works from, and the r fixed links outside that tree (``info()["seeds"]``)
        are r more columns of it: an (m + r) x (m + r) inverse per evaluation, the matrix itself built once and kept (three buffers,
        24 ld^2 bytes, ld = m + r rounded up to 64).  Regime: a connected fixed graph with positive link weights, m + r <= 16384,
        r << num_nodes, any num_nodes."""
        if not isinstance(edge_space, (bool, np.bool_)) and edge_space != "tree":
            raise ValueError(f'edge_space must be False, True or "tree", not {edge_space!r}')
        self.fixed_edges = fixed_edges
        self.all_candidate_edges = candidate_edges
        self.num_nodes = num_nodes
        fi, fj, fw = edges_to_arrays(fixed_edges)
        ci, cj, cw = edges_to_arrays(candidate_edges)
        self.weights = cw
        if isinstance(edge_space, str):
            self._dev = _lib.Esp(num_nodes, fi, fj, fw, ci, cj, cw, device=device, matrix_free="tree", edge_relax="tree")
        elif edge_space:
            self._dev = _lib.Esp(num_nodes, fi, fj, fw, ci, cj, cw, device=device, matrix_free=True, edge_relax=True)
        else:
            self._dev = _lib.Esp(num_nodes, fi, fj, fw, ci, cj, cw, device=device)
        self.edge_space = edge_space
        self.trace = []          # [(F, running upper bound, ||g||_2)] per iteration of the last solve

    def evaluate_objective(self, x) -> float:
        """F(x): the growth of the log tree count over the fixed graph, in nats (F(0) = 0)."""
        return self._dev.relax_eval(np.asarray(x, dtype=np.float64), want_grad=False)[0]

    def problem(self, x):
        """(F(x), gradient): the callable ``mac_amd.optimization.frankwolfe.frank_wolfe`` takes."""
        return self._dev.relax_eval(np.asarray(x, dtype=np.float64), want_grad=True)

    def inner(self, a, b) -> float:
        """<a, b> summed on the device in the order ``solve`` sums <gradient, s - x>: passed to ``frank_wolfe`` as ``inner``,
        the driver's dual values -- and its upper bound -- are those of ``solve`` bit for bit."""
        return self._dev.relax_inner(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))

    def solve(self, k, x_init, rounding="nearest", max_iters=20, relative_duality_gap_tol=1e-4, grad_norm_tol=1e-8,
              random_rounding_max_iters=1, verbose=False, *, exchange=False):
        """Frank-Wolfe (open-loop step 2 / (2 + t)) from ``x_init``, then rounding: ``(rounded, unrounded, upper)`` with
        ``upper`` >= F of every k-edge selection.  The loop runs on the C side (machip_esp_relax_run).  ``exchange=True``: the
        rounded selection is polished by best-swap local search on the same handle (``exchange``) before it is returned; node
        space and connected fixed graphs only (ValueError on an ``edge_space`` handle, which keeps no dense inverse, and on a
        handle with beta != 0, both before any iteration).  ``exchange="edge"``: the same polish by ``exchange_edge``, on an
        ``edge_space`` handle only (ValueError on a node-space handle, and for any other string, before any iteration)."""
        if isinstance(exchange, str):
            if exchange != "edge":
                raise ValueError(f'exchange must be False, True or "edge", not {exchange!r}')
            if not self.edge_space:
                raise ValueError('exchange="edge" works on the Gram matrix of an edge_space handle: this one has edge_space=False '
                                 "(use exchange=True)")
        elif exchange and self.edge_space:
            raise ValueError(f"exchange=True needs the dense inverse: not available with edge_space={self.edge_space!r} "
                             '(use exchange="edge")')
        if exchange and not isinstance(exchange, str) and k < len(self.weights) and self._dev.info()["beta"] != 0.0:      # (refused before the Frank-Wolfe run, not after it)
            raise ValueError("exchange=True needs a connected fixed graph: this handle has beta = %g" % self._dev.info()["beta"])
        m = len(self.weights)
        if k >= m:
            result = np.ones(m)
            return result, result, self.evaluate_objective(result)
        assert len(x_init) == m
        r = self._dev.relax_run(k, x_init, max_iters=max_iters, gap_tol=relative_duality_gap_tol, grad_tol=grad_norm_tol)
        self.trace, ub = [], float("inf")
        for i in range(r["iters"]):
            ub = min(ub, float(r["dual"][i]))
            self.trace.append((float(r["f"][i]), ub, float(r["gnorm"][i])))
            if verbose:
                print(f"[mac_amd] it {i}: F={r['f'][i]:.12g} u={ub:.12g} |g|={r['gnorm'][i]:.3g}")
        w = r["x"]
        if rounding == "madow":
            rounded = round_madow(w, k, value_fn=self.evaluate_objective, max_iters=random_rounding_max_iters)
        else:
            rounded = round_nearest(w, k, self.weights, 10)
        if exchange:
            rounded = (self.exchange_edge if isinstance(exchange, str) else self.exchange)(rounded)[0]
        return rounded, w, float(r["upper"])

    def exchange(self, selection, max_swaps=None, min_gain=1e-9):
        """``GreedyESP.exchange`` on this handle: ``(result, selected_edges, info)``."""
        if self.edge_space:
            raise ValueError(f"exchange needs the dense inverse: not available with edge_space={self.edge_space!r} (use exchange_edge)")
        return exchange_on(self._dev, self.all_candidate_edges, selection, max_swaps, min_gain)

    def exchange_edge(self, selection, max_swaps=None, min_gain=1e-9):
        """``exchange`` for an ``edge_space`` handle: the same best-swap local search carried out on the (m + r) x (m + r) Gram
        matrix the relaxation works with (mac_amd/csrc/esp_exchange_edge.h), so it runs at any num_nodes.
        ``selection`` and the returned ``(result, selected_edges, info)`` are those of ``GreedyESP.exchange``.  ValueError on a
        node-space handle (``edge_space=False``), before any device work.  (This second spelling exists only because ``exchange``
        and ``solve(exchange=True)`` are pinned to refuse ``edge_space`` handles; folding the two into one is left for later.)"""
        if not self.edge_space:
            raise ValueError("exchange_edge works on the Gram matrix of an edge_space handle: this one has edge_space=False (use exchange)")
        return exchange_on(self._dev, self.all_candidate_edges, selection, max_swaps, min_gain, edge=True)

    def info(self) -> dict:
        """The handle's description (GreedyESP.info), the space the relaxation works in (relax_form = "node" | "edge" | "edge_tree") with the
        leading dimension it inverts (relax_ld), and the iterations of the last solve."""
        d = self._dev.info()
        ri = self._dev.relax_info()
        d["relax_form"], d["relax_ld"] = ri["form"], ri["ld"]
        d["iterations"] = len(self.trace)
        return d
