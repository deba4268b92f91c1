"""The non-dominated filter (reference acquisition/multi_objective/dominance.py:23-70), minimisation."""
from __future__ import annotations

import numpy as np


def non_dominated(observations):
    """observations [N, D] -> (the non-dominated points [P, D] in their original order, mask [N]).  A point is dominated when
    another one is no worse in every objective and better in at least one; duplicates of a non-dominated point are all kept
    (as the reference keeps them)."""
    obs = np.asarray(observations, dtype=np.float64)
    if obs.ndim != 2:
        raise ValueError(f"observations must be [N, D], got shape {obs.shape}")
    n = obs.shape[0]
    mask = np.ones(n, dtype=bool)
    for i in range(n):
        if not mask[i]:
            continue
        # what point i dominates can never be on the front
        dominated = np.all(obs[i] <= obs, axis=1) & np.any(obs[i] < obs, axis=1)
        mask &= ~dominated
    return obs[mask], mask
