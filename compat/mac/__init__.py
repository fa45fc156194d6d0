"""Import-compatibility package: put ``<repo>/compat`` on ``PYTHONPATH`` (next to the repo root) and code written against
the reference keeps its import lines --

    from mac.solvers import MAC, NaiveGreedy            # mac/solvers/__init__.py:1-2 of the reference
    from mac.utils.graphs import Edge
    from mac.utils.fiedler import find_fiedler_pair
    from mac.utils.rounding import round_madow, round_nearest
    from mac.optimization.frankwolfe import frank_wolfe

-- and runs the MI355X implementation (``mac_amd``): this package holds no code of its own, it registers the ``mac_amd``
modules under the reference's module names.

GreedyESP is provided as ``from mac.solvers import GreedyESP`` (``mac_amd/solvers/esp.py``, on the GPU).  The reference's
module path ``mac.solvers.greedy_esp`` is not: ``mac.solvers`` is the ``mac_amd.solvers`` package object, so a module of that
name there would answer the reference's import line, which stays an ImportError -- a script written against the reference
changes that one line (examples/g2o_experiment.py: ``from mac.solvers.greedy_esp import GreedyESP`` ->
``from mac.solvers import GreedyESP``).  GreedyEig is provided both ways, ``from mac.solvers import GreedyEig`` and the
reference's own ``from mac.solvers.greedy_eig import GreedyEig`` (``mac_amd/solvers/greedy_eig.py``, on the GPU).
ESPRelaxation (no counterpart in the reference: the convex relaxation GreedyESP's paper pairs the greedy with) is
``from mac.solvers import ESPRelaxation`` (``mac_amd/solvers/esp_relax.py``); ``ESPRelaxation(..., edge_space=True)`` is its
candidate-space form for chain-fixed graphs of any length.
GreedyKirchhoff (no counterpart in the reference either: the greedy under the A-optimal criterion, tr L^+) is
``from mac.solvers import GreedyKirchhoff`` (``mac_amd/solvers/kirchhoff.py``).
``mac.utils.cholesky`` (the reference's CHOLMOD wrapper) is not provided: importing it raises ImportError, as it does in the
reference without its optional SuiteSparse dependency.
"""
import importlib
import sys

_ALIASES = {
    "mac.solvers": "mac_amd.solvers",
    "mac.solvers.mac": "mac_amd.solvers.mac",
    "mac.solvers.baseline": "mac_amd.solvers.baseline",
    "mac.solvers.greedy_eig": "mac_amd.solvers.greedy_eig",
    "mac.solvers.esp_relax": "mac_amd.solvers.esp_relax",
    "mac.solvers.kirchhoff": "mac_amd.solvers.kirchhoff",
    "mac.utils": "mac_amd.utils",
    "mac.utils.graphs": "mac_amd.utils.graphs",
    "mac.utils.fiedler": "mac_amd.utils.fiedler",
    "mac.utils.rounding": "mac_amd.utils.rounding",
    "mac.utils.conversions": "mac_amd.utils.graphs",       # nx_to_mac lives with the graph helpers here
    "mac.optimization": "mac_amd.optimization",
    "mac.optimization.frankwolfe": "mac_amd.optimization.frankwolfe",
    "mac.optimization.constraints": "mac_amd.optimization.constraints",
}
for _alias, _real in _ALIASES.items():
    sys.modules[_alias] = importlib.import_module(_real)
solvers = sys.modules["mac.solvers"]
utils = sys.modules["mac.utils"]
optimization = sys.modules["mac.optimization"]
