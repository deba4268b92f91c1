"""The Pareto set, its hypervolume indicator and the default reference point (reference
acquisition/multi_objective/pareto.py:29-80, 270-287)."""
from __future__ import annotations

import numpy as np

from .dominance import non_dominated
from .partition import prepare_default_non_dominated_partition_bounds


class Pareto:
    """The non-dominated subset ``front`` of a set of observations [N, D] (D >= 2), minimisation."""

    def __init__(self, observations, already_non_dominated: bool = False):
        obs = np.asarray(observations, dtype=np.float64)
        if obs.ndim != 2:
            raise ValueError(f"observations must have rank 2, got shape {obs.shape}")
        if obs.shape[-1] < 2:
            raise ValueError(f"a Pareto set needs at least 2 objectives, got {obs.shape[-1]}")
        self.front = obs if already_non_dominated else non_dominated(obs)[0]

    def hypervolume_indicator(self, reference):
        """The volume dominated by the front and bounded by ``reference`` [D]: the box [min front - 1, reference] minus the
        cells of the non-dominated region inside it.  A front point beyond the reference point is a ValueError, as is an
        empty front."""
        if self.front.size == 0:
            raise ValueError("empty front cannot be used to calculate hypervolume indicator")
        reference = np.asarray(reference, dtype=np.float64)
        helper_anti_reference = np.min(self.front, axis=0) - 1.0
        lower, upper = prepare_default_non_dominated_partition_bounds(reference, self.front, helper_anti_reference)
        non_dominated_hypervolume = np.sum(np.prod(upper - lower, axis=1))
        return float(np.prod(reference - helper_anti_reference) - non_dominated_hypervolume)


def get_reference_point(observations):
    """The default (dynamic) reference point of the front of ``observations`` [..., N, D]: max + 2 (max - min) / |front| per
    objective."""
    obs = np.asarray(observations, dtype=np.float64)
    if obs.size == 0:
        raise ValueError("empty observations cannot be used to calculate reference point")
    front = Pareto(obs).front
    spread = np.max(front, axis=-2) - np.min(front, axis=-2)
    return np.max(front, axis=-2) + 2.0 * spread / front.shape[-2]
