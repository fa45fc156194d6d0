"""Public solver surface of the drop-in (the names mac/solvers/__init__.py exports, plus GreedyESP, GreedyEig and ESPRelaxation)."""
from mac_amd.solvers.baseline import NaiveGreedy  # noqa: F401
from mac_amd.solvers.esp import GreedyESP  # noqa: F401
from mac_amd.solvers.esp_relax import ESPRelaxation  # noqa: F401
from mac_amd.solvers.greedy_eig import GreedyEig  # noqa: F401
from mac_amd.solvers.kirchhoff import GreedyKirchhoff  # noqa: F401
from mac_amd.solvers.mac import MAC  # noqa: F401

__all__ = ["MAC", "NaiveGreedy", "GreedyESP", "GreedyEig", "ESPRelaxation", "GreedyKirchhoff"]
