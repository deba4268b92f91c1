"""Batch Monte-Carlo expected hypervolume improvement (reference acquisition/function/multi_objective.py:253-412) over a
stack of engine-backed exact GPRs, one per objective: builder and function object.  The joint posteriors, the
reparametrised samples and the inclusion-exclusion over the subsets of the batch run on the device (tgp_qehvi_values);
the sampler's base draws, the Pareto front and its partition are host arithmetic.  ``differentiable=True`` builds the function
with ``value_and_gradient`` (tgp_qehvi_value_grad), which routes it to L-BFGS-B; the default function is value-only."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import engine as _engine_mod
from ...data import Dataset
from ..function import _is_torch
from ..interface import AcquisitionFunctionClass, SingleModelAcquisitionBuilder
from .ehvi import _PartitionOwner, _stack_engines
from .pareto import Pareto, get_reference_point
from .partition import prepare_default_non_dominated_partition_bounds


class batch_ehvi(_PartitionOwner, AcquisitionFunctionClass):
    """The expected hypervolume improvement of a batch of B points, for minimisation, estimated on the fixed draws of
    ``sampler`` (a reparametrization sampler over the model stack) over the cells ``partition_bounds`` = (lower [K, P],
    upper [K, P]) of the non-dominated region.  x [..., B, D] -> [..., 1], B <= ``trieste_amd.engine.QEHVI_MAX_Q``."""

    def __init__(self, sampler, sampler_jitter: float, partition_bounds):
        self._sampler = sampler
        self._jitter = float(sampler_jitter)
        self._model = sampler._model
        self._engine = _stack_engines(self._model, type(self).__name__)[0]
        self._device_eps = None   # (the host draws it was copied from, the device, the copy)
        self.update(partition_bounds)

    def _eps_like(self, x, batch_size: int):
        """The sampler's draws [P, B, S] where the points live."""
        eps = self._sampler.eps(batch_size)
        if not (_is_torch(x) and x.is_cuda):
            return eps
        held = self._device_eps
        if held is None or held[0] is not eps or held[1] != x.device:
            import torch

            self._device_eps = held = (eps, x.device, torch.as_tensor(eps, device=x.device))
        return held[2]

    def __call__(self, x):
        if not _is_torch(x):
            x = np.asarray(x, dtype=np.float64)
        if len(x.shape) < 2:
            raise ValueError(f"batch query points must be [..., B, D], got input shape {tuple(x.shape)}")
        batch_size = int(x.shape[-2])
        if batch_size > _engine_mod.QEHVI_MAX_Q:
            raise ValueError(f"the batch expected hypervolume improvement takes batches of at most "
                             f"{_engine_mod.QEHVI_MAX_Q} points (2^B - 1 subsets per sample and cell), got {batch_size}")
        engines = self._engines()
        return _engine_mod.qehvi_values(engines, x, self._eps_like(x, batch_size), self._jitter)[..., None]


class differentiable_batch_ehvi(batch_ehvi):
    """:class:`batch_ehvi` with its gradient w.r.t. the batch: what ``tfp.math.value_and_gradient`` takes through
    ``predict_joint``, the Cholesky factors, the reparametrised samples and the inclusion-exclusion when the reference
    hands the function to ``batchify_joint(generate_continuous_optimizer)``, here in one device call per chunk
    (``trieste_amd.engine.qehvi_value_grad``: every model's joint posterior, the tail with its moment adjoints, every
    model's vector-Jacobian product).  Having ``value_and_gradient`` is what routes it to the continuous optimizer.  At a
    tie between two points' samples, or a sample exactly on a cell bound, the gradient is that of the first point and of
    the clamped (constant) side (include/tgp.h)."""

    def value_and_gradient(self, points):
        """points [R, B, D] -> (values [R], gradients [R, B, D])."""
        on_device = _is_torch(points) and points.is_cuda
        x = points if on_device else np.ascontiguousarray(points.cpu().numpy() if _is_torch(points) else points,
                                                          dtype=np.float64)
        if len(x.shape) != 3:
            raise ValueError(f"points must be [R, B, D], got shape {tuple(x.shape)}")
        R, B = int(x.shape[0]), int(x.shape[1])
        if B > _engine_mod.QEHVI_MAX_Q:
            raise ValueError(f"the batch expected hypervolume improvement takes batches of at most "
                             f"{_engine_mod.QEHVI_MAX_Q} points (2^B - 1 subsets per sample and cell), got {B}")
        engines = self._engines()
        eps = self._eps_like(x, B)
        values, grads = np.empty(R), np.empty(tuple(x.shape))
        chunk = max(1, _engine_mod.QEHVI_GRAD_MAX_POINTS // B)
        for r0 in range(0, R, chunk):
            v, g = _engine_mod.qehvi_value_grad(engines, x[r0:r0 + chunk], eps, self._jitter)
            if on_device:
                v, g = v.cpu().numpy(), g.cpu().numpy()
            values[r0:r0 + chunk], grads[r0:r0 + chunk] = np.asarray(v), np.asarray(g)
        return values, grads


class BatchMonteCarloExpectedHypervolumeImprovement(SingleModelAcquisitionBuilder):
    """Builder of the batch expected hypervolume improvement (Daulton et al. 2020, as the reference implements it):
    ``sample_size`` reparametrised samples of the stack's joint posterior per batch; front, reference point and partition
    as :class:`~trieste_amd.acquisition.multi_objective.ehvi.ExpectedHypervolumeImprovement`.  There is no
    ``update_acquisition_function`` override: the default prepares a new function, which draws fresh samples.
    ``differentiable=True`` builds the function with ``value_and_gradient`` (L-BFGS-B refinement of the joint batch instead
    of a random search); the default leaves the function value-only."""

    def __init__(self, sample_size: int, reference_point_spec=get_reference_point, *, jitter: float = 1e-6,
                 differentiable: bool = False):
        if not sample_size > 0:
            raise ValueError(f"sample_size must be positive, got {sample_size}")
        if not jitter >= 0.0:
            raise ValueError(f"jitter must be non-negative, got {jitter}")
        self._sample_size = sample_size
        self._jitter = jitter
        if callable(reference_point_spec):
            self._ref_point_spec = reference_point_spec
        else:
            self._ref_point_spec = np.asarray(reference_point_spec, dtype=np.float64)
        self._ref_point = None
        self._differentiable = bool(differentiable)

    def __repr__(self) -> str:
        extra = ", differentiable=True" if self._differentiable else ""
        if callable(self._ref_point_spec):
            return (f"BatchMonteCarloExpectedHypervolumeImprovement({self._sample_size!r},"
                    f" {self._ref_point_spec.__name__},"
                    f" jitter={self._jitter!r}{extra})")
        return (f"BatchMonteCarloExpectedHypervolumeImprovement({self._sample_size!r},"
                f" {self._ref_point_spec!r}"
                f" jitter={self._jitter!r}{extra})")

    def prepare_acquisition_function(self, model, dataset: Optional[Dataset] = None):
        if dataset is None or len(dataset) == 0:
            raise ValueError("Dataset must be populated.")
        mean, _ = model.predict(dataset.query_points)
        mean = np.asarray(mean, dtype=np.float64)
        spec = self._ref_point_spec
        self._ref_point = np.asarray(spec(mean) if callable(spec) else spec, dtype=np.float64)
        front = Pareto(mean).front
        screened_front = front[np.all(front <= self._ref_point, axis=-1)]
        partition_bounds = prepare_default_non_dominated_partition_bounds(self._ref_point, screened_front)
        if not hasattr(model, "reparam_sampler"):
            raise ValueError("The batch Monte-Carlo expected hyper-volume improvement function only supports models that "
                             f"implement a reparam_sampler method; received {model!r}")
        sampler = model.reparam_sampler(self._sample_size)
        cls = differentiable_batch_ehvi if self._differentiable else batch_ehvi
        return cls(sampler, self._jitter, partition_bounds)
