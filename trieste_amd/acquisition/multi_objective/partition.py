"""Partitions of the non-dominated region into axis-aligned cells (reference acquisition/multi_objective/partition.py): the
exact staircase for two objectives and the divide-and-conquer procedure of Couckuyt et al. (2012) for more.  Both store
cells as indices into the pseudo front (anti-reference point, front points, reference point), so every bound of every cell
is one of F + 2 values per objective -- which is what the device kernel's bound tables rest on."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .dominance import non_dominated

JITTER = 1e-6  # the reference's DEFAULTS.JITTER (utils/misc.py)


def prepare_default_non_dominated_partition_bounds(reference, observations=None, anti_reference=None):
    """(lower, upper) [K, D] of the cells covering the region no observation dominates inside [anti_reference, reference]:
    the exact partition for D = 2, divide and conquer above, and the single cell [anti_reference, reference] when there are
    no observations.  ``anti_reference`` defaults to -1e10 per objective (standing in for -inf), which reference point and
    observations must then not lie below."""
    reference = np.asarray(reference, dtype=np.float64)
    if reference.ndim != 1:
        raise ValueError(f"reference must have shape [D], got {reference.shape}")
    empty = observations is None or np.size(observations) == 0
    if not empty:
        observations = np.asarray(observations, dtype=np.float64)
    if anti_reference is None:
        anti_reference = np.full(reference.shape, -1e10)
        if np.any(reference < anti_reference):
            raise ValueError(f"reference point: {reference} containing at least one value below default anti-reference "
                             "point ([-1e10, ..., -1e10]), try specify a lower anti-reference point.")
        if not empty and np.any(observations < anti_reference):
            raise ValueError(f"observations: {observations} containing at least one value below default anti-reference "
                             "point ([-1e10, ..., -1e10]), try specify a lower anti-reference point.")
    else:
        anti_reference = np.asarray(anti_reference, dtype=np.float64)
        if anti_reference.ndim != 1:
            raise ValueError(f"anti_reference must have shape [D], got {anti_reference.shape}")
    if empty:
        if anti_reference.shape != reference.shape or np.any(anti_reference > reference):
            raise ValueError(f"anti_reference point: {anti_reference} contains at least one value larger than reference "
                             f"point: {reference}")
        return anti_reference[None].copy(), reference[None].copy()
    if observations.shape[-1] > 2:
        return DividedAndConquerNonDominated(observations).partition_bounds(anti_reference, reference)
    return ExactPartition2dNonDominated(observations).partition_bounds(anti_reference, reference)


def _checked_front(front) -> np.ndarray:
    front = np.asarray(front, dtype=np.float64)
    if front.ndim != 2 or front.shape[0] == 0:
        raise ValueError(f"front must be a non-empty [F, D] array, got shape {front.shape}")
    if not np.all(non_dominated(front)[1]):
        raise ValueError(f"\ninput {front} contains dominated points")
    return front


class _BoundIndexPartition:
    """Partitions stored as indices into the pseudo front: ``lower_idx`` / ``upper_idx`` [K, D] with 0 = anti-reference
    point, 1 .. F = front points, F + 1 = reference point."""

    front: np.ndarray
    lower_idx: np.ndarray
    upper_idx: np.ndarray

    def __new__(cls, *args, **kwargs):
        if cls is _BoundIndexPartition:
            raise TypeError("BoundIndexPartition may not be instantiated directly")
        return object.__new__(cls)

    def partition_bounds(self, anti_reference, reference):
        """-> (lower, upper) [K, D]; the front must lie inside [anti_reference, reference]."""
        reference = np.asarray(reference, dtype=np.float64)
        anti_reference = np.asarray(anti_reference, dtype=np.float64)
        D = self.front.shape[1]
        if reference.shape != (D,) or anti_reference.shape != (D,):
            raise ValueError(f"reference and anti_reference must have shape [{D}], got {reference.shape} and "
                             f"{anti_reference.shape}")
        if np.any(reference < self.front):
            raise ValueError(f"reference point {reference} lies below a point of the front")
        if np.any(self.front < anti_reference):
            raise ValueError(f"anti-reference point {anti_reference} lies above a point of the front")
        pseudo_front = np.concatenate([anti_reference[None], self.front, reference[None]], axis=0)
        cols = np.arange(D)[None, :]
        return pseudo_front[self.lower_idx, cols], pseudo_front[self.upper_idx, cols]


def _pseudo_front_idx(front: np.ndarray) -> np.ndarray:
    """[F + 2, D]: per objective the pseudo-front rows in ascending order of that objective."""
    F, D = front.shape
    return np.concatenate([np.zeros((1, D), np.int64), np.argsort(front, axis=0, kind="stable") + 1,
                           np.full((1, D), F + 1, np.int64)], axis=0)


class ExactPartition2dNonDominated(_BoundIndexPartition):
    """The F + 1 cells of the staircase above a two-objective front."""

    def __init__(self, front):
        front = _checked_front(front)
        if front.shape[1] != 2:
            raise ValueError(f"the exact partition takes two objectives, got {front.shape[1]}")
        self.front = front[np.argsort(front[:, 0], kind="stable")]  # ascending in the first, so descending in the second
        F = self.front.shape[0]
        order = _pseudo_front_idx(self.front)
        steps = np.arange(F + 1)
        self.lower_idx = np.stack([steps, np.zeros_like(steps)], axis=-1)
        self.upper_idx = np.stack([steps + 1, order[::-1, 1][: F + 1]], axis=-1)


class DividedAndConquerNonDominated(_BoundIndexPartition):
    """Branch and bound over index boxes of the sorted pseudo front: a box none of whose interior a front point dominates is
    accepted as a cell, a box entirely dominated is dropped, anything else is halved along its longest edge.  ``threshold``
    (a fraction of the front's bounding box) drops undecided boxes below that volume, which makes the partition
    approximate."""

    def __init__(self, front, threshold: float = 0):
        self.front = _checked_front(front)
        self.lower_idx, self.upper_idx = self._bound_index(float(threshold))

    def _bound_index(self, threshold: float):
        front = self.front
        F, D = front.shape
        min_front = np.min(front, axis=0, keepdims=True) - 1
        max_front = np.max(front, axis=0, keepdims=True) + 1
        pseudo_front = np.concatenate([min_front, front, max_front], axis=0)
        order = _pseudo_front_idx(front)
        total_size = np.prod(max_front - min_front)
        cols = np.arange(D)
        lower_result, upper_result = [], []
        stack = [(np.zeros(D, np.int64), np.full(D, F + 1, np.int64))]
        while stack:
            c0, c1 = stack.pop()
            lower_idx, upper_idx = order[c0, cols], order[c1, cols]
            lower, upper = pseudo_front[lower_idx, cols], pseudo_front[upper_idx, cols]
            # every front point is outside the box's interior in some objective: nothing in the box is dominated
            if np.all(np.any((upper - JITTER) < front, axis=1)):
                lower_result.append(lower_idx)
                upper_result.append(upper_idx)
                continue
            # some front point dominates the box's lower corner: the whole box is dominated
            if not np.all(np.any((lower + JITTER) < front, axis=1)):
                continue
            dist = c1 - c0
            if not (np.any(dist > 1) and np.prod(upper - lower) / total_size > threshold):
                continue
            edge, axis = int(np.max(dist)), int(np.argmax(dist))
            first = int(round(edge / 2.0))  # (half to even, as the reference's rounding)
            second = edge - first
            upper_cut, lower_cut = c1.copy(), c0.copy()
            upper_cut[axis] -= first
            lower_cut[axis] += second
            stack.append((c0, upper_cut))
            stack.append((lower_cut, c1))
        if not lower_result:
            return np.zeros((0, D), np.int64), np.zeros((0, D), np.int64)
        return np.stack(lower_result), np.stack(upper_result)
