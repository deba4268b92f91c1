"""Expected hypervolume improvement (reference acquisition/function/multi_objective.py:49-250) over a stack of
engine-backed exact GPRs, one per objective: builder and function object.  Values and arg-max run on the device
(tgp_ehvi_values / tgp_ehvi_argmax); the Pareto front and its partition are host arithmetic on a few dozen points."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import engine as _engine_mod
from ...data import Dataset
from ..function import _is_torch, _require_engine
from ..interface import AcquisitionFunctionClass, SingleModelAcquisitionBuilder
from .pareto import Pareto, get_reference_point
from .partition import prepare_default_non_dominated_partition_bounds


def _stack_engines(model, who: str):
    """The engines of a stack of engine-backed models on one device, in output order."""
    members = getattr(model, "_models", None)
    if members is None:
        raise TypeError(f"{who} needs a ModelStack of engine-backed models (trieste_amd.models.GaussianProcessRegression), "
                        f"one per objective; received {model!r}.  There is no CPU evaluation path.")
    engines = [_require_engine(m, who) for m in members]
    if len({e.device for e in engines}) != 1:
        raise TypeError(f"{who} needs a ModelStack of engine-backed models on one device; received devices "
                        f"{[e.device for e in engines]}.  There is no CPU evaluation path.")
    return engines


class _PartitionOwner:
    """What the function objects over a stack share: their cells as the engine's tables, and the ownership token under which
    they sit on the stack's leading engine.  The partition is engine state: another function object over the same stack (an
    EHVI and a batch EHVI function, say), or a re-attached engine of a copied model, may have replaced it, so every call
    goes through :meth:`_engines`, which installs this object's cells unless the engine still carries its token."""

    def update(self, partition_bounds) -> None:
        """New cells (the front moved)."""
        lower, upper = (np.asarray(b, dtype=np.float64) for b in partition_bounds)
        if lower.ndim != 2 or lower.shape != upper.shape:
            raise ValueError(f"partition bounds must be two [K, P] arrays, got {lower.shape} and {upper.shape}")
        P = len(_stack_engines(self._model, type(self).__name__))
        if lower.shape[1] != P:
            raise ValueError(f"the partition has {lower.shape[1]} objectives, the model stack {P}")
        self._lb_points, self._ub_points = lower, upper
        self._tables = _engine_mod.ehvi_partition_tables(lower, upper)
        self._token = object()   # identifies (this function, this partition); never recurs while the engine holds it

    def _engines(self):
        """The stack's engines with this function's partition installed on the first."""
        engines = _stack_engines(self._model, type(self).__name__)
        self._engine = lead = engines[0]
        if getattr(lead, "_ehvi_owner", None) is not self._token:
            _engine_mod.ehvi_set_partition_tables(lead, *self._tables)   # (clears the engine's owner mark)
            lead._ehvi_owner = self._token
        return engines


class expected_hv_improvement(_PartitionOwner, AcquisitionFunctionClass):
    """EHVI of a single point under independent Gaussian marginals, for minimisation, over the cells ``partition_bounds``
    = (lower [K, P], upper [K, P]) of the non-dominated region.  The bound values are turned into per-objective tables of
    distinct values and per-cell indices here (exact float64 values) and live on the leading engine of the stack."""

    def __init__(self, model, partition_bounds):
        self._model = model
        engines = _stack_engines(model, type(self).__name__)
        self._engine = engines[0]
        self.update(partition_bounds)

    def _points(self, x):
        if not _is_torch(x):
            x = np.asarray(x, dtype=np.float64)
        if len(x.shape) < 2 or x.shape[-2] != 1:
            raise ValueError(f"This acquisition function only supports batch sizes of one, got input shape {tuple(x.shape)}")
        return x[..., 0, :]

    def __call__(self, x):
        points = self._points(x)
        return _engine_mod.ehvi_values(self._engines(), points)[..., None]

    # fused sweeps (no [M] values returned to the host)
    def argmax(self, points, index_base: int = 0):
        """points [M, D] -> (value, global index, point [D]); the first index wins ties."""
        return _engine_mod.ehvi_argmax(self._engines(), points, index_base)

    def argmax_sampled(self, seed: int, num_samples: int, lower, upper):
        """Arg-max over ``num_samples`` uniform candidates of the box generated on the device."""
        engines = self._engines()
        return _engine_mod.ehvi_argmax(engines, engines[0].sample_box(seed, 0, num_samples, lower, upper), 0)


class differentiable_expected_hv_improvement(expected_hv_improvement):
    """:class:`expected_hv_improvement` with its gradient w.r.t. the point: what ``tfp.math.value_and_gradient`` takes
    through ``predict``, the square root, Psi and nu when the reference hands the function to
    ``generate_continuous_optimizer``, here in one device call per chunk (``trieste_amd.engine.ehvi_value_grad``: every
    model's posterior, the tail with its moment adjoints, every model's vector-Jacobian product).  Having
    ``value_and_gradient`` is what routes it to the continuous optimizer."""

    def value_and_gradient(self, points):
        """points [R, D] -> (values [R], gradients [R, D])."""
        x = np.ascontiguousarray(points.cpu().numpy() if _is_torch(points) else points, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError(f"points must be [R, D], got shape {x.shape}")
        engines = self._engines()
        R = x.shape[0]
        values, grads = np.empty(R), np.empty(x.shape)
        chunk = _engine_mod.EHVI_GRAD_MAX_POINTS
        for r0 in range(0, R, chunk):
            v, g = _engine_mod.ehvi_value_grad(engines, x[r0:r0 + chunk])
            values[r0:r0 + chunk], grads[r0:r0 + chunk] = np.asarray(v), np.asarray(g)
        return values, grads


class ExpectedHypervolumeImprovement(SingleModelAcquisitionBuilder):
    """Builder of EHVI: the front of the posterior means at the observed points (which screens out observation noise), its
    reference point -- fixed, or computed from those means by ``reference_point_spec`` (default:
    :func:`get_reference_point`) -- and the partition of the region no front point dominates.  ``differentiable=True``
    builds the function with ``value_and_gradient`` (L-BFGS-B refinement instead of a random search); the default leaves
    the function value-only."""

    def __init__(self, reference_point_spec=get_reference_point, *, differentiable: bool = False):
        if callable(reference_point_spec):
            self._ref_point_spec = reference_point_spec
        else:
            self._ref_point_spec = np.asarray(reference_point_spec, dtype=np.float64)
        self._ref_point = None
        self._differentiable = bool(differentiable)

    def __repr__(self) -> str:
        extra = ", differentiable=True" if self._differentiable else ""
        if callable(self._ref_point_spec):
            return f"ExpectedHypervolumeImprovement({self._ref_point_spec.__name__}{extra})"
        return f"ExpectedHypervolumeImprovement({self._ref_point_spec!r}{extra})"

    def _partition_bounds(self, model, dataset: Optional[Dataset]):
        if dataset is None or len(dataset) == 0:
            raise ValueError("Dataset must be populated.")
        mean, _ = model.predict(dataset.query_points)
        mean = np.asarray(mean, dtype=np.float64)
        spec = self._ref_point_spec
        self._ref_point = np.asarray(spec(mean) if callable(spec) else spec, dtype=np.float64)
        front = Pareto(mean).front
        screened_front = front[np.all(front <= self._ref_point, axis=-1)]
        return prepare_default_non_dominated_partition_bounds(self._ref_point, screened_front)

    def prepare_acquisition_function(self, model, dataset: Optional[Dataset] = None):
        cls = differentiable_expected_hv_improvement if self._differentiable else expected_hv_improvement
        return cls(model, self._partition_bounds(model, dataset))

    def update_acquisition_function(self, function, model, dataset: Optional[Dataset] = None):
        if not isinstance(function, expected_hv_improvement):
            raise ValueError("function must be an expected_hv_improvement instance")
        function.update(self._partition_bounds(model, dataset))
        return function
