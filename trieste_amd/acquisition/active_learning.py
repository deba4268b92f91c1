"""Active learning: the integrated variance reduction (IMSE) criterion, reference
trieste/acquisition/function/active_learning.py:250-415 (Picheny et al. 2010).

The reference evaluates ``model.conditional_predict_f(integration_points, additional_data=x)`` per candidate batch and
averages.  Here the conditioned variance is the Schur complement over the q query points, everything that depends on
(model, integration points) alone is built once on the device, and a candidate chunk costs the small-product posterior,
one more product and a tail kernel (``trieste_amd.engine.ivr_values``; include/tgp.h tgp_ivr_values)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import engine as _engine_mod
from ..data import Dataset
from .function import _is_torch, _require_engine
from .interface import AcquisitionFunctionClass, SingleModelAcquisitionBuilder


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
