"""Scenario generation: the reference layout (seed-reproducible), the grid-swap family for large N, and its
grid-swap-device form generated in batches on the GPU; goal assignment for interchangeable vehicles."""
from .assignment import assign_goals, assign_goals_batch  # noqa: F401
from .grid_swap_device import generate_grid_swap_batch, generate_grid_swap_device  # noqa: F401
from .position_generator import generate_grid_swap, generate_positions, straight_line_min_distance  # noqa: F401

__all__ = ("generate_positions", "generate_grid_swap", "straight_line_min_distance", "generate_grid_swap_batch",
           "generate_grid_swap_device", "assign_goals", "assign_goals_batch")
