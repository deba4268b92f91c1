"""Active learning: the integrated variance reduction (IMSE) criterion, reference
trieste/acquisition/function/active_learning.py:250-415 (Picheny et al. 2010).

The reference evaluates ``model.conditional_predict_f(integration_points, additional_data=x)`` per candidate batch and
averages.  Here the conditioned variance is the Schur complement over the q query points, everything that depends on
(model, integration points) alone is built once on the device, and a candidate chunk costs the small-product posterior,
one more product and a tail kernel (``trieste_amd.engine.ivr_values``; include/tgp.h tgp_ivr_values).

And the batch criterion of D-optimal design, :class:`PredictiveVariance` (active_learning.py:36-110): the determinant of the
joint predictive covariance of a batch, factorised on the device (``trieste_amd.engine.pvar_values``), with an opt-in
gradient for the L-BFGS-B refinement of the batch."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import engine as _engine_mod
from ..data import Dataset
from ..sampler import JITTER
from .function import _is_torch, _require_engine
from .interface import AcquisitionFunctionClass, SingleModelAcquisitionBuilder


class PredictiveVariance(SingleModelAcquisitionBuilder):
    """Builder for the determinant of the predictive covariance matrix over the batch points (active_learning.py:36-83); for a
    batch of one point the predictive variance.  ``differentiable=True`` builds the function with ``value_and_gradient``
    (L-BFGS-B over the whole batch instead of a random search over batches); the default leaves it value-only."""

    def __init__(self, jitter: float = JITTER, *, differentiable: bool = False):
        """``jitter``: added to every entry of the covariance before its factorisation, as the reference adds it."""
        if not 0.0 <= float(jitter) < np.inf:
            raise ValueError(f"jitter must be finite and non-negative, got {jitter}")
        self._jitter = jitter
        self._differentiable = bool(differentiable)

    def __repr__(self) -> str:
        extra = ", differentiable=True" if self._differentiable else ""
        return f"PredictiveVariance(jitter={self._jitter!r}{extra})"

    def prepare_acquisition_function(self, model, dataset: Optional[Dataset] = None):
        if not hasattr(model, "predict_joint"):
            raise NotImplementedError(f"PredictiveVariance only works with models that support predict_joint; "
                                      f"received {model!r}")
        cls = differentiable_predictive_variance if self._differentiable else predictive_variance
        return cls(model, self._jitter)

    def update_acquisition_function(self, function, model, dataset: Optional[Dataset] = None):
        return function  # no need to update anything


class predictive_variance(AcquisitionFunctionClass):
    """x [..., q, D] -> [..., 1]: det(cov + jitter) of the joint predictive covariance of the batch, the jitter added to every
    entry as the reference does (active_learning.py:86-110); q = 1: the predictive variance.  Posterior, factorisation and
    determinant run on the device (``trieste_amd.engine.pvar_values``; include/tgp.h tgp_pvar_values), 1 <= q <=
    ``trieste_amd.engine.PVAR_MAX_Q``; a batch whose covariance is not positive definite gets NaN.  Value only:
    ``batchify_joint`` sweeps it by random search; :class:`differentiable_predictive_variance` adds the gradient."""

    def __init__(self, model, jitter: float):
        if not hasattr(model, "predict_joint"):
            raise NotImplementedError(f"PredictiveVariance only works with models that support predict_joint; "
                                      f"received {model!r}")
        self._model = model
        self._engine = _require_engine(model, type(self).__name__)
        self._jitter = float(jitter)

    def _points(self, x):
        if not _is_torch(x):
            x = np.asarray(x, dtype=np.float64)
        if len(x.shape) < 2:
            raise ValueError(f"x must be [..., q, D], got shape {tuple(x.shape)}")
        q = int(x.shape[-2])
        if not 1 <= q <= _engine_mod.PVAR_MAX_Q:
            raise ValueError(f"PredictiveVariance takes batches of 1 to {_engine_mod.PVAR_MAX_Q} points, got {q}")
        return x

    def __call__(self, x):
        """x [..., q, D] -> [..., 1]."""
        return _engine_mod.pvar_values(_require_engine(self._model, type(self).__name__), self._points(x), self._jitter)[..., None]

    def log_det(self, x):
        """x [..., q, D] -> [..., 1] = log det(cov + jitter), for batches whose determinant underflows."""
        eng = _require_engine(self._model, type(self).__name__)
        return _engine_mod.pvar_values(eng, self._points(x), self._jitter, with_logdet=True)[1][..., None]


class differentiable_predictive_variance(predictive_variance):
    """:class:`predictive_variance` with its gradient w.r.t. the batch, d det = det tr(A^-1 dA) through ``predict_joint``, in
    one device call per chunk (``trieste_amd.engine.pvar_value_grad``).  Having ``value_and_gradient`` is what routes it to
    the continuous optimizer."""

    def value_and_gradient(self, points):
        """points [P, q, D] -> (values [P], gradients [P, q, D])."""
        x = np.ascontiguousarray(points.cpu().numpy() if _is_torch(points) else points, dtype=np.float64)
        if x.ndim != 3:
            raise ValueError(f"points must be [P, q, D], got shape {x.shape}")
        x = self._points(x)
        P, q, _ = x.shape
        eng = _require_engine(self._model, type(self).__name__)
        values, grads = np.empty(P), np.empty(x.shape)
        chunk = max(1, getattr(eng, "JOINT_SMALL_POINTS", 2048) // q)
        for g0 in range(0, P, chunk):
            v, g = _engine_mod.pvar_value_grad(eng, x[g0:g0 + chunk], self._jitter)
            values[g0:g0 + chunk], grads[g0:g0 + chunk] = np.asarray(v), np.asarray(g)
        return values, grads


class IntegratedVarianceReduction(SingleModelAcquisitionBuilder):
    """Builder for the reduction of the integral of the predicted variance over the search space given a batch of query
    points (active_learning.py:250-301)."""

    def __init__(self, integration_points, threshold=None):
        """``integration_points`` [P, D]: the points to integrate the predictive variance over; ``threshold``: None, a
        float, or a sequence of one or two increasing values."""
        self._integration_points = integration_points
        self._threshold = threshold

    def __repr__(self) -> str:
        return f"IntegratedVarianceReduction(threshold={self._threshold!r})"

    def prepare_acquisition_function(self, model, dataset: Optional[Dataset] = None):
        if not hasattr(model, "conditional_predict_f"):   # the reference's FastUpdateModel check (its message names the sibling)
            raise NotImplementedError(f"PredictiveVariance only works with FastUpdateModel models; received {model!r}")
        return integrated_variance_reduction(model, self._integration_points, self._threshold)

    def update_acquisition_function(self, function, model, dataset: Optional[Dataset] = None):
        return function  # no need to update anything: the function follows the model (see its docstring)


def _threshold_values(threshold) -> Optional[np.ndarray]:
    if threshold is None:
        return None
    if isinstance(threshold, (float, int)) and not isinstance(threshold, bool):
        return np.array([float(threshold)])
    try:
        t = np.asarray(threshold, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"threshold should be a float, a sequence or a rank 1 array, received {threshold!r}") from e
    if t.ndim != 1:
        raise ValueError(f"threshold should be a float, a sequence or a rank 1 array, received shape {t.shape}")
    if not 1 <= t.size <= 2:
        raise ValueError(f"threshold should have one or two values, received {t.size}")
    if t.size == 2 and not t[1] >= t[0]:
        raise ValueError(f"threshold values should be in increasing order, received {t}")
    return t


class integrated_variance_reduction(AcquisitionFunctionClass):
    r"""The reduction of the weighted average of the predicted variance over the integration points (the IMSE criterion),
    active_learning.py:304-415.  To maximise:

        \int (v_old(z) - v_new(z)) w(z) dz,

    of which, v_old being constant in the query points, the reference returns -mean_z(v_new(z) w(z)), and so does
    ``__call__``; :meth:`reduction` returns the non-negative query-dependent part mean_z((v_old - v_new)(z) w(z)), which is
    10^2 - 10^4 times smaller than the constant and keeps the digits the value has lost.

    Weights: 1 without a threshold; the posterior pdf at T with one threshold; P(T1 < f < T2) with two -- computed ONCE, from
    ``model.predict(integration_points)`` at construction, as in the reference (:398-405).  The weights are frozen; what
    depends on the model's data and hyper-parameters (the cross-covariances with the integration points, v_old) follows the
    model, rebuilt by the engine after every update.  That is what the reference's ``update_acquisition_function``
    (``return function``) amounts to.

    x [..., q, D] -> [..., 1], 1 <= q <= ``trieste_amd.engine.IVR_MAX_Q``.  Value only (no ``value_and_gradient``):
    ``batchify_joint`` sweeps it by random search over the joint space, as it does the default ``BatchExpectedImprovement``.

    One engine holds one integration set: the function installs its own points unless the engine still carries its token."""

    def __init__(self, model, integration_points, threshold=None):
        self._model = model
        self._engine = _require_engine(model, type(self).__name__)
        z = np.asarray(integration_points.cpu() if _is_torch(integration_points) else integration_points, dtype=np.float64)
        if z.ndim != 2:
            raise ValueError(f"integration_points must be of shape [N, D], got {z.shape}")
        if z.shape[0] < 1:
            raise ValueError("integration_points should contain at least one point")
        if z.shape[1] != self._engine.d:
            raise ValueError(f"integration_points have {z.shape[1]} dimensions, the model {self._engine.d}")
        self._integration_points = np.ascontiguousarray(z)
        t = _threshold_values(threshold)
        if t is None:
            self._weights = None
        else:
            from scipy.stats import norm

            mean_old, var_old = model.predict(self._integration_points)
            mean_old = np.asarray(mean_old, dtype=np.float64).reshape(-1)
            sd = np.sqrt(np.asarray(var_old, dtype=np.float64).reshape(-1))
            if t.size == 1:
                self._weights = norm.pdf(t[0], loc=mean_old, scale=sd)
            else:
                self._weights = norm.cdf(t[1], loc=mean_old, scale=sd) - norm.cdf(t[0], loc=mean_old, scale=sd)
            self._weights = np.ascontiguousarray(np.maximum(self._weights, 0.0))   # (a difference of cdfs may round below 0)
        self._token = object()

    @property
    def weights(self):
        """[P] (None: all ones)."""
        return self._weights

    def _installed(self):
        eng = self._engine = _require_engine(self._model, type(self).__name__)
        if getattr(eng, "_ivr_owner", None) is not self._token:
            _engine_mod.set_integration_points(eng, self._integration_points, self._weights)   # (clears the owner mark)
            eng._ivr_owner = self._token
        return eng

    def _points(self, x):
        if not _is_torch(x):
            x = np.asarray(x, dtype=np.float64)
        if len(x.shape) < 2:
            raise ValueError(f"x must be [..., q, D], got shape {tuple(x.shape)}")
        q = int(x.shape[-2])
        if not 1 <= q <= _engine_mod.IVR_MAX_Q:
            raise ValueError(f"IntegratedVarianceReduction takes batches of 1 to {_engine_mod.IVR_MAX_Q} points, got {q}")
        return x

    def __call__(self, x):
        """x [..., q, D] -> [..., 1] = -mean_z(v_new(z) w(z))."""
        x = self._points(x)
        return _engine_mod.ivr_values(self._installed(), x)[..., None]

    def reduction(self, x):
        """x [..., q, D] -> [..., 1] = mean_z((v_old - v_new)(z) w(z)) >= 0: ``__call__`` plus the constant it leaves out."""
        x = self._points(x)
        return _engine_mod.ivr_values(self._installed(), x, with_reduction=True)[1][..., None]
