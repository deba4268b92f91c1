"""Thin object wrapper over the C-ABI: one :class:`GPEngine` == one GPR model resident on one GPU.

Arrays may be numpy float64 arrays (host; staged by the library) or torch float64 CUDA tensors
(device; passed by pointer, outputs are torch tensors on the same device).  torch is plumbing
only: device memory, streams and torch.distributed.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib

_NP = np.float64


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class _Arg:
    """Pointer + residency of one input array (keeps the backing object alive)."""

    def __init__(self, x, shape_tail: Optional[Tuple[int, ...]] = None):
        if _is_torch(x):
            import torch

            if x.dtype != torch.float64:
                x = x.to(torch.float64)
            if x.is_cuda:
                x = x.contiguous()
                self.keep, self.ptr, self.where = x, x.data_ptr(), _lib.DEVICE
                self.shape, self.device = tuple(x.shape), x.device
                return
            x = x.numpy()
        a = np.ascontiguousarray(x, dtype=_NP)
        self.keep, self.ptr, self.where = a, a.ctypes.data, _lib.HOST
        self.shape, self.device = a.shape, None


# -- one parser per kind of argument ------------------------------------------------------------------------------------
def _groups(lead) -> int:
    return int(np.prod(lead)) if lead else 1


def _batch_points(d: int, Xq, noun: str = "batch"):
    """Xq [..., q, d] -> (argument, leading shape, q, number of q-batches)."""
    a = _Arg(Xq)
    if len(a.shape) < 2 or a.shape[-1] != d:
        raise ValueError(f"{noun} query points must be [..., q, {d}], got {a.shape}")
    lead, q = a.shape[:-2], a.shape[-2]
    return a, lead, q, _groups(lead)


def _draws(a: _Arg, q: int, eps) -> _Arg:
    """eps [q, S], where the points ``a`` live."""
    e = _Arg(eps)
    if len(e.shape) != 2 or e.shape[0] != q:
        raise ValueError(f"eps must be [q={q}, S], got {e.shape}")
    if e.where != a.where:
        raise ValueError("Xq and eps must live in the same place (both host or both device)")
    return e


_MOMENT_FORMS = {"...": (1, False), "G": (2, True), "P, ...": (2, False)}   # leading axes -> (lowest rank of mean, exactly that)


def _moment_pair(mean, cov, form: str, same_place: bool = True):
    """mean [<form>, q] and cov [<form>, q, q] as a model's ``predict_joint`` returns them -> the two arguments."""
    m, c = _Arg(mean), _Arg(cov)
    low, exact = _MOMENT_FORMS[form]
    if len(m.shape) < low or (exact and len(m.shape) != low) or c.shape != m.shape + (m.shape[-1],):
        raise ValueError(f"mean must be [{form}, q] and cov [{form}, q, q], got {m.shape} and {c.shape}")
    if same_place and m.where != c.where:
        raise ValueError("mean and cov must live in the same place (both host or both device)")
    return m, c


def _marginal_pair(mean, var):
    """mean, var [P, M] objective-major -> the two arguments."""
    m, v = _Arg(mean), _Arg(var)
    if len(m.shape) != 2 or m.shape != v.shape:
        raise ValueError(f"mean and var must both be [P, M], got {m.shape} and {v.shape}")
    if m.where != v.where:
        raise ValueError("mean and var must live in the same place (both host or both device)")
    return m, v


def _value_grad_outputs(m: _Arg, lead, second_shape):
    """The outputs of a tail with its adjoints where the moments live: value [lead], the mean's adjoint in the mean's shape, the
    second moment's in ``second_shape`` -> ((value, gmean, gsecond), their three pointers)."""
    outs = [GPEngine._out(m, shape) for shape in (lead, m.shape, second_shape)]
    return tuple(o[0] for o in outs), tuple(o[1] for o in outs)


class GPEngine:
    def __init__(self, d: int, kernel: str = "matern52", device: int = 0):
        """An exact-GPR engine on ``device`` for inputs of ``d`` dimensions, 1 <= d <= 1024 (``_lib.MAX_D``).  Above 32
        dimensions the sweeps run in float64 only (the int8 precisions are refused) and trajectories are refused."""
        self._lib = _lib.load()
        if kernel not in _lib.KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}; choose from {sorted(_lib.KERNELS)}")
        h = C.c_void_p()
        rc = self._lib.tgp_create(int(device), int(d), _lib.KERNELS[kernel], C.byref(h))
        _lib.check(self._lib, None, rc)
        self._h = h
        self._owned = True
        self.d, self.kernel, self.device = int(d), kernel, int(device)
        self.N = 0

    @classmethod
    def _borrowed(cls, handle, d: int, kernel: str, device: int) -> "GPEngine":
        """A view of a handle owned by someone else (a :class:`~trieste_amd.group.GPEngineGroup` member):
        same methods, never destroys the handle."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h, self._owned = handle, False
        self.d, self.kernel, self.device, self.N = int(d), kernel, int(device), 0
        return self

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                self._lib.tgp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        _lib.check(self._lib, self._h, rc)

    def use_torch_stream(self):
        """Queue this engine's kernels on torch's current CUDA stream of its device."""
        import torch

        self._chk(self._lib.tgp_set_stream(self._h, C.c_void_p(
            torch.cuda.current_stream(self.device).cuda_stream)))
        self._private_stream = False

    def use_private_stream(self):
        """Give this engine its own (non-blocking) stream, so that several engines driven from several
        host threads overlap on the GPU -- the latency-bound factorisation chain of one model leaves most
        of the chip idle (used by ``GaussianProcessRegression.find_best_model_initialization``)."""
        self._chk(self._lib.tgp_use_private_stream(self._h))
        self._private_stream = True

    @property
    def on_private_stream(self) -> bool:
        """True after ``use_private_stream``: nothing orders this engine's kernels against torch's streams."""
        return bool(getattr(self, "_private_stream", False))

    def set_variant(self, v: int):
        self._chk(self._lib.tgp_set_variant(self._h, int(v)))

    def set_update_concurrency(self, n: int = 1):
        """``update`` on ``n`` engines at once (tgp_set_update_concurrency): this engine's persistent update kernel takes
        1 / n of the compute units, so that n engines factorising concurrently on private streams run side by side.
        The factor does not depend on n."""
        self._chk(self._lib.tgp_set_update_concurrency(self._h, int(n)))

    def set_precision(self, precision: str = "f64"):
        """Arithmetic of the plain sweeps (tgp_set_precision): "f64" (default, the parity path); "i8x4" / "i8x5" --
        W K* on the int8 matrix cores with four / five 8-bit digit planes per operand (emulated-precision throughput
        options: x5 holds the plain parity tolerance on every tested model, x4 only on well-conditioned ones);
        "auto" -- the int8 sweep with an a-posteriori repair: every candidate whose own error bound exceeds the
        parity tolerance (and, in a fused arg-max, every candidate that could still be the float64 winner) is
        recomputed in float64 inside the same call; four planes, then five, then float64 when too many candidates
        needed it.  Results hold the parity tolerance candidate by candidate and the arg-max is the float64 one -- to
        the 8-sigma error model the bounds come from (a statistical model, not a worst case); every sweep re-checks a
        uniform sample of its candidates AND the unflagged candidates whose bounds sit closest to their tolerance in float64
        against their bounds and leaves the rung when one fails (:meth:`get_auto_report`, :meth:`get_auto_strata`; the
        synchronising calls repeat their sweep on the next rung before returning, the ``*_async`` / group calls take the
        demotion at their next call).  The samples are compared, not written back: values are a pure function of
        (model, rung, candidate).  Float64 remains the only arithmetic the parity claims are made on."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}; choose from {sorted(_lib.PRECISIONS)}")
        self._chk(self._lib.tgp_set_precision(self._h, _lib.PRECISIONS[precision]))

    def get_precision(self):
        """-> (requested, what the next plain sweep runs, fraction of its candidates the last "auto" sweep recomputed
        in float64 or -1.0): tgp_get_precision."""
        req, eff, frac = C.c_int(), C.c_int(), C.c_double()
        self._chk(self._lib.tgp_get_precision(self._h, C.byref(req), C.byref(eff), C.byref(frac)))
        names = {v: k for k, v in _lib.PRECISIONS.items()}
        return names[req.value], names[eff.value], frac.value

    def set_auto_sigma(self, k_sigma: float = 8.0):
        """K_SIGMA of the "auto" precision's per-candidate error bound (tgp_set_auto_sigma; restarts the ladder)."""
        self._chk(self._lib.tgp_set_auto_sigma(self._h, float(k_sigma)))

    def get_auto_report(self):
        """The canary of the "auto" precision since its ladder last restarted (tgp_get_auto_report) ->
        dict(checked, violations, worst_ratio, demotions, level): sampled candidates compared in float64, samples outside
        their bound, worst |var_f64 - var_int8| / bound, rungs left because of a violation, current rung (0 four planes,
        1 five, 2 float64, -1 not "auto")."""
        chk, viol, worst, dem, lev = C.c_int64(), C.c_int64(), C.c_double(), C.c_int(), C.c_int()
        self._chk(self._lib.tgp_get_auto_report(self._h, C.byref(chk), C.byref(viol), C.byref(worst), C.byref(dem),
                                                C.byref(lev)))
        return dict(checked=chk.value, violations=viol.value, worst_ratio=worst.value, demotions=dem.value, level=lev.value)

    def get_auto_strata(self):
        """The canary's report per stratum (tgp_get_auto_strata) -> dict(uniform=dict(checked, violations, worst_ratio),
        adversarial=dict(...), slack_saved): the uniform 1-in-4096 sample and the adversarial one (per 1 / 64 of a sweep the
        unflagged candidate whose bound sits closest to its tolerance)."""
        chk, viol, worst, slack = (C.c_int64 * 2)(), (C.c_int64 * 2)(), (C.c_double * 2)(), C.c_int64()
        self._chk(self._lib.tgp_get_auto_strata(self._h, chk, viol, worst, C.byref(slack)))
        return dict(uniform=dict(checked=chk[0], violations=viol[0], worst_ratio=worst[0]),
                    adversarial=dict(checked=chk[1], violations=viol[1], worst_ratio=worst[1]), slack_saved=slack.value)

    # -- model state -----------------------------------------------------------------------------
    def clone_from(self, other: "GPEngine") -> None:
        """Become a copy of ``other`` (hyper-parameters, data, cached factorisation): tgp_clone_from."""
        if not isinstance(other, GPEngine):
            raise TypeError(f"can only clone from a GPEngine, got {other!r}")
        self._chk(self._lib.tgp_clone_from(self._h, other._h))
        self.N = other.N

    def clone(self) -> "GPEngine":
        """A new engine on the same device holding a copy of this one's state."""
        twin = GPEngine(self.d, self.kernel, device=self.device)
        twin.clone_from(self)
        return twin

    def set_penalization(self, kind: str, pending=None, radius=None, scale=None) -> None:
        """Multiply every acquisition result by prod_p phi_p(x) around the pending points until cleared with
        ``kind="none"`` (tgp_set_penalization; greedy_batch.py:250-389)."""
        if kind not in _lib.PENALIZERS:
            raise ValueError(f"unknown penalizer {kind!r}; choose from {sorted(_lib.PENALIZERS)}")
        if kind == "none" or pending is None or len(pending) == 0:
            self._chk(self._lib.tgp_set_penalization(self._h, 0, None, None, None, 0))
            return
        pts = np.ascontiguousarray(np.asarray(pending, dtype=_NP))
        if pts.ndim != 2 or pts.shape[1] != self.d:
            raise ValueError(f"pending points must be [P, {self.d}], got {pts.shape}")
        P = pts.shape[0]
        r = np.ascontiguousarray(np.asarray(radius, dtype=_NP).reshape(-1))
        sc = np.ascontiguousarray(np.asarray(scale, dtype=_NP).reshape(-1))
        if r.shape[0] != P or sc.shape[0] != P:
            raise ValueError(f"radius and scale must hold P={P} values, got {r.shape}, {sc.shape}")
        self._chk(self._lib.tgp_set_penalization(self._h, _lib.PENALIZERS[kind], pts.ctypes.data, r.ctypes.data,
                                                 sc.ctypes.data, P))

    def set_min_value_samples(self, samples) -> None:
        """Samples of the objective's minimum value used by the "mes" / "gibbon" acquisition kinds
        (tgp_set_min_value_samples); an empty array clears them."""
        sm = np.ascontiguousarray(np.asarray(samples, dtype=_NP).reshape(-1))
        self._chk(self._lib.tgp_set_min_value_samples(self._h, sm.ctypes.data if sm.size else None, int(sm.size)))

    def set_repulsion(self, twin: "GPEngine" = None, weight: float = 1.0) -> None:
        """GIBBON's repulsion term: ``twin`` is this model conditioned additionally on the pending points
        (tgp_set_repulsion); None clears.  The engine keeps a reference so the twin outlives the setting."""
        if twin is None:
            self._chk(self._lib.tgp_set_repulsion(self._h, None, 0.0))
            self._twin = None
            return
        if not isinstance(twin, GPEngine):
            raise TypeError(f"the repulsion twin must be a GPEngine, got {twin!r}")
        self._chk(self._lib.tgp_set_repulsion(self._h, twin._h, float(weight)))
        self._twin = twin

    def penalization_values(self, Xq):
        """prod_p phi_p(x) of the penalization currently set, at Xq [..., d] -> [...]."""
        a, lead, M = self._flat(Xq)
        out, po = self._out(a, lead)
        self._chk(self._lib.tgp_penalization_values(self._h, a.ptr, M, po, a.where))
        return out

    def penalized(self, kind: str, pending, radius, scale):
        """Context manager: the penalization is active inside the block only."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.set_penalization(kind, pending, radius, scale)
            try:
                yield self
            finally:
                self.set_penalization("none")

        return scope()

    def set_hyper(self, variance: float, lengthscales, noise_variance: float, mean_const: float = 0.0):
        ls = np.ascontiguousarray(np.broadcast_to(np.asarray(lengthscales, dtype=_NP), (self.d,)))
        self._chk(self._lib.tgp_set_hyper(self._h, float(variance), ls.ctypes.data,
                                          float(noise_variance), float(mean_const)))
        self.N = 0

    def set_data(self, X, Y):
        ax = _Arg(X)
        ay = _Arg(Y)
        if len(ax.shape) != 2 or ax.shape[1] != self.d:
            raise ValueError(f"X must be [N, {self.d}], got {ax.shape}")
        n = ax.shape[0]
        if int(np.prod(ay.shape)) != n:
            raise ValueError(f"Y must hold N={n} observations, got shape {ay.shape}")
        if ax.where != ay.where:
            raise ValueError("X and Y must both be host arrays or both device tensors")
        self._chk(self._lib.tgp_set_data(self._h, ax.ptr, ay.ptr, n, ax.where))
        self.N = n

    def append_data(self, Xnew, Ynew):
        """Extend the data set by k rows with unchanged hyper-parameters: only the trailing block of the
        factor is recomputed (tgp_append_data)."""
        ax = _Arg(Xnew)
        ay = _Arg(Ynew)
        if len(ax.shape) != 2 or ax.shape[1] != self.d:
            raise ValueError(f"Xnew must be [k, {self.d}], got {ax.shape}")
        k = ax.shape[0]
        if int(np.prod(ay.shape)) != k:
            raise ValueError(f"Ynew must hold k={k} observations, got shape {ay.shape}")
        if ax.where != ay.where:
            raise ValueError("Xnew and Ynew must both be host arrays or both device tensors")
        self._chk(self._lib.tgp_append_data(self._h, ax.ptr, ay.ptr, k, ax.where))
        self.N += k

    def nlml(self, with_gradient: bool = True):
        """(negative log marginal likelihood, gradient [d + 3] w.r.t. lengthscales, variance, noise, mean);
        ``with_gradient=False`` returns (value, None) and skips the K^-1 product."""
        v = C.c_double()
        if not with_gradient:
            self._chk(self._lib.tgp_nlml(self._h, C.byref(v), None))
            return v.value, None
        g = np.empty(self.d + 3)
        self._chk(self._lib.tgp_nlml(self._h, C.byref(v), g.ctypes.data))
        return v.value, g

    def nlml_trial(self) -> float:
        """The value ``nlml(False)`` would give after ``set_data`` with the data already on the device, at the current
        hyper-parameters (tgp_nlml_trial: the factor only from N = 3841 on).  Leaves the engine WITHOUT a posterior --
        for the throw-away evaluations of a fit's prior draws."""
        v = C.c_double()
        self._chk(self._lib.tgp_nlml_trial(self._h, C.byref(v)))
        return v.value

    def update_is_persistent(self, N: int) -> bool:
        """Is ``set_data`` at N training points ONE persistent launch on this engine (tgp_update_is_persistent)?"""
        yes = C.c_int()
        self._chk(self._lib.tgp_update_is_persistent(self._h, int(N), C.byref(yes)))
        return bool(yes.value)

    def nlml_trial_batch(self, hypers):
        """B trial evaluations on the data already on the device (tgp_nlml_trial_batch): ``hypers`` [B, d + 3] =
        (variance, lengthscales [d], noise variance, mean) per member -> (values [B], ok [B]); a member whose kernel
        matrix is not positive definite gets NaN / False.  From N = 3841 on up to sixteen members share one persistent
        launch; the engine's own hyper-parameters and posterior are untouched."""
        hy = np.ascontiguousarray(hypers, dtype=np.float64)
        if hy.ndim != 2 or hy.shape[1] != self.d + 3:
            raise ValueError(f"hypers must be [B, {self.d + 3}] (variance, lengthscales, noise, mean), got {hy.shape}")
        B = hy.shape[0]
        values = np.empty(B, dtype=np.float64)
        status = np.zeros(B, dtype=np.int32)
        if B:
            self._chk(self._lib.tgp_nlml_trial_batch(self._h, hy.ctypes.data, B, values.ctypes.data, status.ctypes.data))
        return values, status == 0

    def release_scratch(self):
        """Free the process-wide scratch the batched trial evaluations keep on this engine's device
        (tgp_release_scratch): gigabytes at N = 4096, kept between fits on purpose; the next batched fit allocates again."""
        rc = self._lib.tgp_release_scratch(int(self.device))
        if rc != 0:
            raise RuntimeError(f"tgp_release_scratch failed with status {rc}")

    def get_factor(self):
        """(L, W = L^-1, alpha) as numpy arrays (tests / diagnostics)."""
        n = self.N
        L, W, al = np.empty((n, n)), np.empty((n, n)), np.empty(n)
        self._chk(self._lib.tgp_get_factor(self._h, L.ctypes.data, W.ctypes.data, al.ctypes.data, _lib.HOST))
        return L, W, al

    # -- outputs ---------------------------------------------------------------------------------
    @staticmethod
    def _out(arg: _Arg, shape):
        if arg.where == _lib.DEVICE:
            import torch

            t = torch.empty(shape, dtype=torch.float64, device=arg.device)
            return t, t.data_ptr()
        a = np.empty(shape, dtype=_NP)
        return a, a.ctypes.data

    def _flat(self, Xq):
        a = _Arg(Xq)
        if len(a.shape) < 1 or a.shape[-1] != self.d:
            raise ValueError(f"query points must have trailing dimension {self.d}, got {a.shape}")
        lead = a.shape[:-1]
        return a, lead, _groups(lead)

    def predict(self, Xq):
        a, lead, M = self._flat(Xq)
        mean, pm = self._out(a, lead)
        var, pv = self._out(a, lead)
        self._chk(self._lib.tgp_predict(self._h, a.ptr, M, pm, pv, a.where))
        return mean, var

    def predict_mean(self, Xq):
        a, lead, M = self._flat(Xq)
        mean, pm = self._out(a, lead)
        self._chk(self._lib.tgp_predict_mean(self._h, a.ptr, M, pm, a.where))
        return mean

    def predict_joint(self, Xq):
        a, lead, q, G = _batch_points(self.d, Xq, "joint")
        mean, pm = self._out(a, lead + (q,))
        cov, pc = self._out(a, lead + (q, q))
        self._chk(self._lib.tgp_predict_joint(self._h, a.ptr, G, q, pm, pc, a.where))
        return mean, cov

    def sample_joint(self, Xq, eps, jitter: float = 1e-6):
        """Exact joint posterior samples: Xq [n, d], eps [n, S] standard normal -> [S, n]."""
        a, e = _Arg(Xq), _Arg(eps)
        if len(a.shape) != 2 or a.shape[1] != self.d:
            raise ValueError(f"query points must be [n, {self.d}], got {a.shape}")
        if len(e.shape) != 2 or e.shape[0] != a.shape[0]:
            raise ValueError(f"eps must be [n={a.shape[0]}, S], got {e.shape}")
        if a.where != e.where:
            raise ValueError("Xq and eps must both be host arrays or both be CUDA tensors")
        out, po = self._out(a, (e.shape[1], a.shape[0]))
        self._chk(self._lib.tgp_sample_joint(self._h, a.ptr, a.shape[0], e.ptr, e.shape[1], float(jitter), po, a.where))
        return out

    def cov_between(self, X1, X2):
        """X1 [P1, d], X2 [P2, d] -> posterior cross-covariance [P1, P2] (unclipped)."""
        a1, a2 = _Arg(X1), _Arg(X2)
        if len(a1.shape) != 2 or len(a2.shape) != 2 or a1.shape[1] != self.d or a2.shape[1] != self.d:
            raise ValueError(f"query points must be [P, {self.d}], got {a1.shape} and {a2.shape}")
        if a1.where != a2.where:
            raise ValueError("X1 and X2 must both be host arrays or both be CUDA tensors")
        out, po = self._out(a1, (a1.shape[0], a2.shape[0]))
        self._chk(self._lib.tgp_cov_between(self._h, a1.ptr, a1.shape[0], a2.ptr, a2.shape[0], po, a1.where))
        return out

    def eta(self) -> float:
        v = C.c_double()
        self._chk(self._lib.tgp_eta(self._h, C.byref(v)))
        return v.value

    def acq_values(self, acq: str, param: float, Xq):
        a, lead, M = self._flat(Xq)
        out, po = self._out(a, lead)
        self._chk(self._lib.tgp_acq_values(self._h, _lib.ACQ[acq], float(param), a.ptr, M, po, a.where))
        return out

    def acq_value_grad(self, acq: str, param: float, Xq):
        """Xq [P, d] -> (values [P], gradients [P, d]) of the acquisition function."""
        a, lead, P = self._flat(Xq)
        val, pv = self._out(a, lead)
        grad, pg = self._out(a, lead + (self.d,))
        self._chk(self._lib.tgp_acq_value_grad(self._h, _lib.ACQ[acq], float(param), a.ptr, P, pv, pg, a.where))
        return val, grad

    def acq_argmax(self, acq: str, param: float, Xq, index_base: int = 0):
        """-> (best value, global index, best point [d] as numpy)."""
        a, _, M = self._flat(Xq)
        bv, bi = C.c_double(), C.c_int64()
        bx = np.empty(self.d)
        self._chk(self._lib.tgp_acq_argmax(self._h, _lib.ACQ[acq], float(param), a.ptr, M, int(index_base),
                                           C.byref(bv), C.byref(bi), bx.ctypes.data, a.where))
        return bv.value, bi.value, bx

    def acq_argmax_pair(self, acq: str, param: float, Xq, index_base: int = 0):
        """The fused arg-max with the winner left ON THE DEVICE: Xq a CUDA tensor [M, d] -> CUDA float64 tensor
        [2] = (value, global index as an int64 bit pattern).  Only enqueues on the engine's stream
        (tgp_acq_argmax_async): no host synchronisation -- gather the pairs of all ranks, merge them with
        :meth:`merge_winners`, read the result once."""
        import torch

        if not _is_torch(Xq) or not Xq.is_cuda:  # host candidates: put them on this engine's device first
            Xq = torch.as_tensor(np.ascontiguousarray(Xq, dtype=_NP)).to(f"cuda:{self.device}")
        a, _, M = self._flat(Xq)
        pair = torch.empty(2, dtype=torch.float64, device=a.device)
        self._chk(self._lib.tgp_acq_argmax_async(self._h, _lib.ACQ[acq], float(param), a.ptr, M, int(index_base),
                                                 pair.data_ptr()))
        return pair

    def merge_winners(self, gathered, minimize: bool = False):
        """gathered: CUDA float64 tensor [P, 2, V] (an all-gather of P ranks' [2, V] pairs) -> CUDA tensor [2, V]
        with the winners under (max value -- min if ``minimize`` --, min global index); enqueue only."""
        import torch

        if not (_is_torch(gathered) and gathered.is_cuda and gathered.dtype == torch.float64 and gathered.dim() == 3
                and gathered.shape[1] == 2):
            raise ValueError("gathered must be a CUDA float64 tensor [P, 2, V]")
        g = gathered.contiguous()
        out = torch.empty((2, g.shape[2]), dtype=torch.float64, device=g.device)
        self._chk(self._lib.tgp_merge_winners_async(self._h, g.data_ptr(), int(g.shape[0]), int(g.shape[2]),
                                                    1 if minimize else 0, out.data_ptr()))
        return out

    def synchronize(self) -> None:
        """Wait for everything enqueued on the engine's stream (tgp_stream_synchronize)."""
        self._chk(self._lib.tgp_stream_synchronize(self._h))

    def acq_topk(self, acq: str, param: float, Xq, k: int, index_base: int = 0):
        a, _, M = self._flat(Xq)
        vals, idx = np.empty(k), np.empty(k, dtype=np.int64)
        self._chk(self._lib.tgp_acq_topk(self._h, _lib.ACQ[acq], float(param), a.ptr, M, int(index_base),
                                         int(k), vals.ctypes.data, idx.ctypes.data, a.where))
        return vals, idx

    def sample_box(self, seed: int, first: int, M: int, lower, upper):
        """Uniform candidates [M, d] generated on the device (torch CUDA tensor)."""
        import torch

        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=_NP), (self.d,)))
        up = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=_NP), (self.d,)))
        out = torch.empty((M, self.d), dtype=torch.float64, device=f"cuda:{self.device}")
        self._chk(self._lib.tgp_sample_box(self._h, int(seed), int(first), int(M), lo.ctypes.data,
                                           up.ctypes.data, out.data_ptr()))
        return out

    def qei(self, Xq, eps, eta: float, jitter: float = 1e-6):
        a, lead, q, G = _batch_points(self.d, Xq)
        e = _draws(a, q, eps)
        out, po = self._out(a, lead)
        self._chk(self._lib.tgp_qei(self._h, a.ptr, G, q, e.ptr, e.shape[1], float(eta), float(jitter), po,
                                    a.where))
        return out

    JOINT_SMALL_POINTS = 2048   # tgp_joint_forward / tgp_joint_vjp: points (groups x q) per call

    def _joint_small(self, Xq):
        a = _Arg(Xq)
        if len(a.shape) != 3 or a.shape[-1] != self.d:
            raise ValueError(f"batch query points must be [G, q, {self.d}], got {a.shape}")
        G, q = a.shape[0], a.shape[1]
        if G * q > self.JOINT_SMALL_POINTS:
            raise ValueError(f"{G} groups of {q} points: at most {self.JOINT_SMALL_POINTS} points per call (chunk the groups)")
        return a, G, q

    def joint_forward(self, Xq):
        """Xq [G, q, d] (G * q <= 2048) -> mean [G, q], cov [G, q, q]: ``predict_joint`` of the handful of q-batches an
        L-BFGS-B iteration holds, as a skinny product (tgp_joint_forward)."""
        a, G, q = self._joint_small(Xq)
        mean, pm = self._out(a, (G, q))
        cov, pc = self._out(a, (G, q, q))
        if G:
            self._chk(self._lib.tgp_joint_forward(self._h, a.ptr, G, q, pm, pc, a.where))
        return mean, cov

    def joint_vjp(self, Xq, gmean, gcov):
        """d/dXq [G, q, d] of sum gmean * mean + sum gcov * cov (tgp_joint_vjp): the engine's share of a batch acquisition
        function's gradient."""
        a, G, q = self._joint_small(Xq)
        gm, gc = _Arg(gmean), _Arg(gcov)
        if gm.shape != (G, q) or gc.shape != (G, q, q):
            raise ValueError(f"gmean must be [{G}, {q}] and gcov [{G}, {q}, {q}], got {gm.shape} and {gc.shape}")
        if gm.where != a.where or gc.where != a.where:
            raise ValueError("Xq, gmean and gcov must live in the same place (all host or all device)")
        grad, pg = self._out(a, (G, q, self.d))
        if G:
            self._chk(self._lib.tgp_joint_vjp(self._h, a.ptr, G, q, gm.ptr, gc.ptr, pg, a.where))
        return grad

    @staticmethod
    def qei_value_grad_fits(q: int, S: int) -> bool:
        """Does tgp_qei_value_grad take groups of q points with S draws (one wave per group, everything in LDS)?"""
        return 1 <= q <= 64 and 8 * (2 * q * (q | 1) + 128) + 4 * ((S + 1) & ~1) <= 160 * 1024

    def qei_value_grad(self, Xq, eps, eta: float, jitter: float = 1e-6):
        """Xq [G, q, d] (G * q <= 2048, q <= 64), eps [q, S] -> (qEI [G], gradient [G, q, d]) in one device call
        (tgp_qei_value_grad)."""
        a, G, q = self._joint_small(Xq)
        e = _draws(a, q, eps)
        val, pv = self._out(a, (G,))
        grad, pg = self._out(a, (G, q, self.d))
        if G:
            self._chk(self._lib.tgp_qei_value_grad(self._h, a.ptr, G, q, e.ptr, e.shape[1], float(eta), float(jitter), pv, pg,
                                                   a.where))
        return val, grad

    def reparam_samples(self, Xq, eps, jitter: float = 1e-6):
        """Xq [..., q, d], eps [q, S] -> samples [..., S, q]."""
        a, lead, q, G = _batch_points(self.d, Xq)
        e = _draws(a, q, eps)
        S = e.shape[1]
        out, po = self._out(a, lead + (S, q))
        self._chk(self._lib.tgp_reparam_samples(self._h, a.ptr, G, q, e.ptr, S, float(jitter), po, a.where))
        return out

    def last_kernel_ms(self):
        ms, n = C.c_double(), C.c_int()
        self._chk(self._lib.tgp_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- trajectories ----------------------------------------------------------------------------
    def trajectory_rff(self, rff_W, rff_b, eps) -> "Trajectory":
        """B trajectories f_b(x) = phi(x) . theta_b + c with theta ~ the posterior of the RFF weights given
        the data (reference RandomFourierFeatureTrajectorySampler), theta = mean + chol(cov) eps[:, b]."""
        return Trajectory(self, rff_W, rff_b, eps, None)

    def trajectory(self, rff_W, rff_b, w, xi) -> "Trajectory":
        return Trajectory(self, rff_W, rff_b, w, xi)


def prune_counters(eng: "GPEngine"):
    """(candidate blocks, blocks given up, row blocks skipped) of ``eng``'s most recent arg-max; zeros when it did not run
    the pruned EI sweep (tgp_get_prune_counters).  A measurement aid beside the engine, not part of the surface the
    acquisition code drives: synchronises the engine's stream."""
    b, g, r = C.c_int64(), C.c_int64(), C.c_int64()
    eng._chk(eng._lib.tgp_get_prune_counters(eng._h, C.byref(b), C.byref(g), C.byref(r)))
    return b.value, g.value, r.value


def prune_screened(eng: "GPEngine"):
    """Of the blocks given up in ``eng``'s most recent arg-max, those given up by the mean screen, before their first row
    block (tgp_get_prune_screened); 0 when it did not run the pruned EI sweep.  Synchronises the engine's stream."""
    s = C.c_int64()
    eng._chk(eng._lib.tgp_get_prune_screened(eng._h, C.byref(s)))
    return s.value


def prune_prescreened(eng: "GPEngine"):
    """Of the blocks the mean screen gave up in ``eng``'s most recent arg-max, those the float32 pre-screen dismissed before
    their float64 mean pass (tgp_get_prune_prescreened).  Synchronises the engine's stream."""
    s = C.c_int64()
    eng._chk(eng._lib.tgp_get_prune_prescreened(eng._h, C.byref(s)))
    return s.value


def prune_tiles(eng: "GPEngine"):
    """(blocks pre-listed for the exact mean pass, wave-tile work items) of ``eng``'s most recent arg-max
    (tgp_get_prune_tiles); items is 0 when the few-blocks path was not taken.  Synchronises the engine's stream."""
    p, t = C.c_int64(), C.c_int64()
    eng._chk(eng._lib.tgp_get_prune_tiles(eng._h, C.byref(p), C.byref(t)))
    return p.value, t.value


def prescreen_means(eng: "GPEngine", Xq):
    """(mean32, E) per candidate: the posterior mean as the pre-screen forms it on the device and the bound it holds for
    |mean32 - mean| (tgp_prescreen_means).  A test and measurement aid."""
    a, lead, M = eng._flat(Xq)
    m32, pm = eng._out(a, lead)
    E, pe = eng._out(a, lead)
    eng._chk(eng._lib.tgp_prescreen_means(eng._h, a.ptr, M, pm, pe, a.where))
    return m32, E


def set_prune_split(eng: "GPEngine", max_survivors: int = -1, max_groups: int = 0):
    """The split regime of the pruned EI sweep (tgp_set_prune_split): blocks that survive the mean screen are cut into
    ranges of row blocks when at most ``max_survivors`` survive (-1: the derived cap, 0: never), into at most
    ``max_groups`` ranges each (0: up to the row blocks).  Same bits either way: a test and A/B aid."""
    eng._chk(eng._lib.tgp_set_prune_split(eng._h, int(max_survivors), int(max_groups)))


def prune_split(eng: "GPEngine"):
    """(survivors of the mean screen, split work items) of ``eng``'s most recent arg-max (tgp_get_prune_split); items is 0
    when the survivors ran whole.  Synchronises the engine's stream."""
    s, i = C.c_int64(), C.c_int64()
    eng._chk(eng._lib.tgp_get_prune_split(eng._h, C.byref(s), C.byref(i)))
    return s.value, i.value


class Trajectory:
    """B decoupled trajectories sharing one RFF basis (tgp_traj_*)."""

    def __init__(self, eng: GPEngine, rff_W, rff_b, w, xi=None):
        """Decoupled trajectories from prior weights w [F, B] and noise draws xi [N, B]; with
        ``xi=None`` ``w`` holds standard-normal draws eps [F, B] for the RFF weight posterior
        (tgp_traj_create_rff: no canonical part)."""
        self._eng = eng
        Wf = np.ascontiguousarray(rff_W, dtype=_NP)
        bf = np.ascontiguousarray(rff_b, dtype=_NP).reshape(-1)
        F = Wf.shape[0]
        if Wf.shape != (F, eng.d) or bf.shape != (F,):
            raise ValueError("rff_W must be [F, d] and rff_b [F]")
        w = np.ascontiguousarray(np.asarray(w, dtype=_NP).reshape(F, -1))
        B = w.shape[1]
        t = C.c_void_p()
        if xi is None:
            rc = eng._lib.tgp_traj_create_rff(eng._h, Wf.ctypes.data, bf.ctypes.data, F, w.ctypes.data, B, C.byref(t))
        else:
            xi = np.ascontiguousarray(np.asarray(xi, dtype=_NP).reshape(eng.N, -1))
            if xi.shape[1] != B:
                raise ValueError(f"xi must be [N, B={B}], got {xi.shape}")
            rc = eng._lib.tgp_traj_create(eng._h, Wf.ctypes.data, bf.ctypes.data, F, w.ctypes.data,
                                          xi.ctypes.data, B, C.byref(t))
        eng._chk(rc)
        self._t, self.F, self.B = t, F, B
        self.N = eng.N  # the model it was drawn from: the library refuses the trajectory once that model is replaced

    def theta(self):
        """Feature weights [F, B] of an RFF-weight trajectory."""
        self._live()
        out = np.empty((self.F, self.B))
        self._eng._chk(self._eng._lib.tgp_traj_get_theta(self._t, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_t", None):
            self._eng._lib.tgp_traj_destroy(self._t)
            self._t = None

    def _live(self):
        """The C trajectory keeps a pointer to its model handle: refuse to run once either is closed."""
        if not getattr(self, "_t", None) or not getattr(self._eng, "_h", None):
            raise RuntimeError("the trajectory (or the engine it belongs to) has been closed")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def v(self):
        self._live()
        out = np.empty((self.N, self.B))
        self._eng._chk(self._eng._lib.tgp_traj_get_v(self._t, out.ctypes.data))
        return out

    def __call__(self, Xq):
        """Xq [M, d] (shared) or [M, B, d] (per-trajectory inputs) -> [M, B]."""
        self._live()
        a = _Arg(Xq)
        d = self._eng.d
        if len(a.shape) == 2 and a.shape[1] == d:
            per, M = 0, a.shape[0]
        elif len(a.shape) == 3 and a.shape[1] == self.B and a.shape[2] == d:
            per, M = 1, a.shape[0]
        else:
            raise ValueError(f"trajectory inputs must be [M, {d}] or [M, {self.B}, {d}], got {a.shape}")
        out, po = GPEngine._out(a, (M, self.B))
        self._eng._chk(self._eng._lib.tgp_traj_eval(self._t, a.ptr, M, per, po, a.where))
        return out

    def value_and_gradient(self, Xq):
        """Xq [P, B, d] (trajectory b at its own point) -> (values [P, B], gradients [P, B, d])."""
        self._live()
        a = _Arg(Xq)
        d = self._eng.d
        if len(a.shape) != 3 or a.shape[1] != self.B or a.shape[2] != d:
            raise ValueError(f"trajectory inputs must be [P, {self.B}, {d}], got {a.shape}")
        P = a.shape[0]
        val, pv = GPEngine._out(a, (P, self.B))
        grad, pg = GPEngine._out(a, (P, self.B, d))
        self._eng._chk(self._eng._lib.tgp_traj_value_grad(self._t, a.ptr, P, pv, pg, a.where))
        return val, grad

    def argmin_pairs(self, Xq, index_base: int = 0):
        """The arg-min of all B trajectories with the winners left ON THE DEVICE: Xq a CUDA tensor [M, d] -> CUDA
        float64 tensor [2, B] (values, then global indices as int64 bit patterns); enqueue only
        (tgp_traj_argmin_async)."""
        import torch

        self._live()
        a = _Arg(Xq)
        if len(a.shape) != 2 or a.shape[1] != self._eng.d or a.where != _lib.DEVICE:
            raise ValueError("argmin_pairs needs device-resident candidates [M, d] (a CUDA tensor)")
        pairs = torch.empty((2, self.B), dtype=torch.float64, device=a.device)
        self._eng._chk(self._eng._lib.tgp_traj_argmin_async(self._t, a.ptr, a.shape[0], int(index_base),
                                                            pairs.data_ptr()))
        return pairs

    def argmin(self, Xq, index_base: int = 0):
        self._live()
        a = _Arg(Xq)
        if len(a.shape) != 2 or a.shape[1] != self._eng.d:
            raise ValueError("arg-min candidates must be [M, d]")
        vals, idx = np.empty(self.B), np.empty(self.B, dtype=np.int64)
        self._eng._chk(self._eng._lib.tgp_traj_argmin(self._t, a.ptr, a.shape[0], int(index_base),
                                                      vals.ctypes.data, idx.ctypes.data, a.where))
        return vals, idx


# -- analytic batch EI (tgp_batch_ei / tgp_batch_ei_moments) ---------------------------------------------------------------
# Module-level functions, not methods: an object that brings its own ``batch_ei`` / ``batch_ei_moments`` (a stand-in engine
# of the host-logic tests) is deferred to; a :class:`GPEngine` goes to the library.
BATCH_EI_MAX_Q = 16


def _sobol_args(a: _Arg, q: int, w1, w2):
    """The two Sobol point sets [S, q] and [S, q - 1], brought to where the first argument lives."""
    if a.where == _lib.DEVICE:
        import torch

        w1, w2 = (w if _is_torch(w) and w.is_cuda else torch.as_tensor(np.ascontiguousarray(w, dtype=_NP)).to(a.device)
                  for w in (w1, w2))
    elif any(_is_torch(w) and w.is_cuda for w in (w1, w2)):
        raise ValueError("the Sobol points are on the device but the first argument is a host array")
    p1, p2 = _Arg(w1), _Arg(w2)
    S = p1.shape[0] if len(p1.shape) == 2 else -1
    if p1.shape != (S, q) or p2.shape != (S, q - 1):
        raise ValueError(f"w1 must be [S, {q}] and w2 [S, {q - 1}], got {p1.shape} and {p2.shape}")
    return p1, p2, S


def _check_bei_q(q: int) -> None:
    if not 2 <= q <= BATCH_EI_MAX_Q:
        raise ValueError(f"the analytic batch EI takes 2 <= q <= {BATCH_EI_MAX_Q} points per batch, got {q}")


def batch_ei(engine, Xq, w1, w2, eta: float):
    """Xq [..., q, d] (2 <= q <= 16), Sobol points w1 [S, q] and w2 [S, q - 1] in [0, 1) -> [...]: the analytic multi-point
    expected improvement of every q-batch (reference ``batch_expected_improvement.__call__``), posterior and tail on the
    device (tgp_batch_ei).  Value only."""
    if not isinstance(engine, GPEngine) and hasattr(engine, "batch_ei"):
        return engine.batch_ei(Xq, w1, w2, eta)
    a, lead, q, G = _batch_points(engine.d, Xq)
    _check_bei_q(q)
    p1, p2, S = _sobol_args(a, q, w1, w2)
    out, po = GPEngine._out(a, lead)
    engine._chk(engine._lib.tgp_batch_ei(engine._h, a.ptr, G, q, p1.ptr, p2.ptr, S, float(eta), po, a.where))
    return out


def batch_ei_moments(engine, mean, cov, w1, w2, eta: float):
    """The same tail on caller-supplied moments: mean [..., q], cov [..., q, q] as a model's ``predict_joint`` returns them
    -> [...] (tgp_batch_ei_moments == the reference's ``_compute_batch_expected_improvement`` behind the 1e-6 and the
    change of sign of ``__call__``).  Needs no data on the engine."""
    if not isinstance(engine, GPEngine) and hasattr(engine, "batch_ei_moments"):
        return engine.batch_ei_moments(mean, cov, w1, w2, eta)
    m, c = _moment_pair(mean, cov, "...")
    lead, q = m.shape[:-1], m.shape[-1]
    _check_bei_q(q)
    p1, p2, S = _sobol_args(m, q, w1, w2)
    out, po = GPEngine._out(m, lead)
    engine._chk(engine._lib.tgp_batch_ei_moments(engine._h, m.ptr, c.ptr, _groups(lead), q, p1.ptr, p2.ptr, S, float(eta), po,
                                                 m.where))
    return out


def batch_ei_moments_grad(engine, mean, cov, w1, w2, eta: float):
    """The tail with its adjoints on caller-supplied moments: mean [G, q], cov [G, q, q] -> (value [G], gmean [G, q],
    gcov [G, q, q]) with gcov symmetric, d value = sum gcov * dcov for every symmetric dcov (tgp_batch_ei_moments_grad).
    Needs no data on the engine."""
    if not isinstance(engine, GPEngine) and hasattr(engine, "batch_ei_moments_grad"):
        return engine.batch_ei_moments_grad(mean, cov, w1, w2, eta)
    m, c = _moment_pair(mean, cov, "G")
    G, q = m.shape
    _check_bei_q(q)
    p1, p2, S = _sobol_args(m, q, w1, w2)
    outs, ptrs = _value_grad_outputs(m, (G,), c.shape)
    engine._chk(engine._lib.tgp_batch_ei_moments_grad(engine._h, m.ptr, c.ptr, G, q, p1.ptr, p2.ptr, S, float(eta), *ptrs, m.where))
    return outs


IVR_MAX_Q, IVR_MAX_P = _lib.IVR_MAX_Q, _lib.IVR_MAX_P


def set_integration_points(engine, Z, weights=None) -> None:
    """The integration set of :func:`ivr_values`: Z [P, d] (1 <= P <= ``IVR_MAX_P``), weights [P] finite and >= 0 or None
    (all ones), both numpy or both CUDA tensors; None or an empty Z clears the setting (tgp_set_integration_points).  Engine
    state: the engine copies both, builds what depends on the model at the next ``ivr_values`` and rebuilds it whenever its
    data or hyper-parameters change.  A clone does not inherit the setting.  Clears the engine's ``_ivr_owner`` mark."""
    if not isinstance(engine, GPEngine) and hasattr(engine, "set_integration_points"):
        return engine.set_integration_points(Z, weights)
    engine._ivr_owner = None
    if Z is None or int(np.prod(tuple(Z.shape) if hasattr(Z, "shape") else np.shape(Z))) == 0:
        engine._chk(engine._lib.tgp_set_integration_points(engine._h, None, 0, None, _lib.HOST))
        return
    z = _Arg(Z)
    if len(z.shape) != 2 or z.shape[1] != engine.d:
        raise ValueError(f"integration points must be [P, {engine.d}], got {z.shape}")
    P, pw = z.shape[0], None
    if weights is not None:
        w = _Arg(weights)
        if int(np.prod(w.shape)) != P:
            raise ValueError(f"weights must hold P={P} values, got shape {w.shape}")
        if w.where != z.where:
            raise ValueError("Z and weights must live in the same place (both host or both device)")
        pw = w.ptr
    engine._chk(engine._lib.tgp_set_integration_points(engine._h, z.ptr, P, pw, z.where))


def ivr_values(engine, Xq, with_reduction: bool = False):
    """Xq [..., q, d] (1 <= q <= ``IVR_MAX_Q``) -> [...]: the integrated variance reduction criterion of every q-batch over
    the engine's integration points, the reference's ``-reduce_mean(conditional variance * weights)`` (tgp_ivr_values);
    ``with_reduction=True`` -> (value, reduction), reduction >= 0 the query-dependent part, value = reduction - c0.  The
    reduction is orders of magnitude smaller than the constant c0, so it keeps the digits the value has lost."""
    if not isinstance(engine, GPEngine) and hasattr(engine, "ivr_values"):
        return engine.ivr_values(Xq, with_reduction)
    a, lead, q, G = _batch_points(engine.d, Xq)
    if not 1 <= q <= IVR_MAX_Q:
        raise ValueError(f"the integrated variance reduction takes 1 <= q <= {IVR_MAX_Q} points per batch, got {q}")
    out, po = GPEngine._out(a, lead)
    red, pr = GPEngine._out(a, lead) if with_reduction else (None, None)
    engine._chk(engine._lib.tgp_ivr_values(engine._h, a.ptr, G, q, po, pr, a.where))
    return (out, red) if with_reduction else out


def ivr_last_ms(engine):
    """Device time of the last :func:`ivr_values` -> (posterior, cross product, tail) in ms, summed over its chunks."""
    p, c, t = C.c_double(), C.c_double(), C.c_double()
    engine._chk(engine._lib.tgp_ivr_last_ms(engine._h, C.byref(p), C.byref(c), C.byref(t)))
    return p.value, c.value, t.value


def ivr_moments(engine, cov, cross, weights=None, noise: float = 0.0):
    """The IVR tail on caller-supplied moments: cov [G, q, q] (``predict_joint``'s), cross [G, q, P] = cov(x_i, z), weights [P]
    or None, ``noise`` added to cov's diagonal -> reduction [G] = (1/P) sum_z w_z |chol(cov + noise I)^-1 cross_.z|^2
    (tgp_ivr_moments).  Needs no data on the engine."""
    c, x = _Arg(cov), _Arg(cross)
    if len(c.shape) != 3 or c.shape[1] != c.shape[2] or len(x.shape) != 3 or x.shape[:2] != c.shape[:2]:
        raise ValueError(f"cov must be [G, q, q] and cross [G, q, P], got {c.shape} and {x.shape}")
    G, q, P = x.shape
    if not 1 <= q <= IVR_MAX_Q:
        raise ValueError(f"the integrated variance reduction takes 1 <= q <= {IVR_MAX_Q} points per batch, got {q}")
    w = None if weights is None else _Arg(weights)
    if w is not None and int(np.prod(w.shape)) != P:
        raise ValueError(f"weights must hold P={P} values, got shape {w.shape}")
    if c.where != x.where or (w is not None and w.where != c.where):
        raise ValueError("cov, cross and weights must live in the same place (all host or all device)")
    out, po = GPEngine._out(c, (G,))
    engine._chk(engine._lib.tgp_ivr_moments(engine._h, c.ptr, x.ptr, None if w is None else w.ptr, G, q, P, float(noise), po,
                                            c.where))
    return out


def _qei_moment_args(mean, cov, eps):
    (m, c), e = _moment_pair(mean, cov, "G", same_place=False), _Arg(eps)
    G, q = m.shape
    if not 1 <= q <= 64:
        raise ValueError(f"the Monte-Carlo qEI takes 1 <= q <= 64 points per batch, got {q}")
    if len(e.shape) != 2 or e.shape[0] != q or e.shape[1] < 1:
        raise ValueError(f"eps must be [q={q}, S >= 1], got {e.shape}")
    if m.where != c.where or m.where != e.where:
        raise ValueError("mean, cov and eps must live in the same place (all host or all device)")
    return m, c, e, G, q, e.shape[1]


def qei_moments(engine, mean, cov, eps, eta: float, jitter: float = 1e-6, samples: bool = False):
    """The Monte-Carlo qEI tail on caller-supplied moments: mean [G, q], cov [G, q, q] as a model's ``predict_joint`` returns
    them, eps [q, S] -> value [G] (``GPEngine.qei``'s, from the same kernel); with ``samples=True`` -> (value, samples
    [G, S, q]), the samples being ``GPEngine.reparam_samples``' (tgp_qei_moments).  Needs no data on the engine."""
    m, c, e, G, q, S = _qei_moment_args(mean, cov, eps)
    out, po = GPEngine._out(m, (G,))
    sam, ps = GPEngine._out(m, (G, S, q)) if samples else (None, None)
    engine._chk(engine._lib.tgp_qei_moments(engine._h, m.ptr, c.ptr, G, q, e.ptr, S, float(eta), float(jitter), po, ps, m.where))
    return (out, sam) if samples else out


def qei_moments_grad(engine, mean, cov, eps, eta: float, jitter: float = 1e-6):
    """The tail with its adjoints on caller-supplied moments -> (value [G], gmean [G, q], gcov [G, q, q]) with gcov symmetric,
    d value = sum gcov * dcov for every symmetric dcov (tgp_qei_moments_grad); (q, S) within ``GPEngine.qei_value_grad_fits``.
    Needs no data on the engine."""
    m, c, e, G, q, S = _qei_moment_args(mean, cov, eps)
    outs, ptrs = _value_grad_outputs(m, (G,), c.shape)
    engine._chk(engine._lib.tgp_qei_moments_grad(engine._h, m.ptr, c.ptr, G, q, e.ptr, S, float(eta), float(jitter), *ptrs, m.where))
    return outs


def batch_ei_value_grad(engine, Xq, w1, w2, eta: float):
    """Xq [G, q, d] (2 <= q <= 16, G * q <= 2048) -> (analytic batch EI [G], its gradient [G, q, d]) in one device call:
    the joint posterior, the tail with its moment adjoints and the posterior's vector-Jacobian product
    (tgp_batch_ei_value_grad)."""
    if not isinstance(engine, GPEngine) and hasattr(engine, "batch_ei_value_grad"):
        return engine.batch_ei_value_grad(Xq, w1, w2, eta)
    a, G, q = engine._joint_small(Xq)
    _check_bei_q(q)
    p1, p2, S = _sobol_args(a, q, w1, w2)
    val, pv = GPEngine._out(a, (G,))
    grad, pg = GPEngine._out(a, (G, q, engine.d))
    if G:
        engine._chk(engine._lib.tgp_batch_ei_value_grad(engine._h, a.ptr, G, q, p1.ptr, p2.ptr, S, float(eta), pv, pg, a.where))
    return val, grad


# ---- expected hypervolume improvement (tgp_ehvi_*; include/tgp.h) -----------------------------------------------------
EHVI_MAX_P, EHVI_MAX_BOUNDS, EHVI_MAX_CELLS = _lib.EHVI_MAX_P, _lib.EHVI_MAX_BOUNDS, _lib.EHVI_MAX_CELLS


def ehvi_tile_width(P: int, V: int) -> int:
    """Candidates per workgroup of the EHVI kernel: the largest power of two <= 64 whose table of 8 P V C bytes fits 160 KiB
    of LDS (V = the largest number of distinct bounds of an objective).  The kernel's 1024 threads are C lanes x 1024 / C
    slices of the cell list."""
    C = 64
    while C > 1 and 8 * P * V * C > 160 * 1024:
        C //= 2
    return C


def ehvi_partition_tables(lower, upper):
    """Cell bounds (lower, upper) [K, P] as a partition returns them -> (bounds [P, Vmax] rows ascending and padded with their
    last value, n_bounds [P] int32, lower_idx [K, P] int32, upper_idx [K, P] int32): per objective the distinct float64 values
    of all bounds (``np.unique``: exact values, no tolerance) and every cell's positions in them."""
    lo, up = np.asarray(lower, dtype=_NP), np.asarray(upper, dtype=_NP)
    if lo.ndim != 2 or lo.shape != up.shape:
        raise ValueError(f"partition bounds must be two [K, P] arrays, got {lo.shape} and {up.shape}")
    K, P = lo.shape
    rows, li, ui = [], np.empty((K, P), np.int32), np.empty((K, P), np.int32)
    for j in range(P):
        values, inverse = np.unique(np.concatenate([lo[:, j], up[:, j]]), return_inverse=True)
        rows.append(values)
        li[:, j], ui[:, j] = inverse[:K], inverse[K:]
    n = np.array([len(r) for r in rows], dtype=np.int32)
    bounds = np.empty((P, max(int(n.max()), 1) if P else 1), dtype=_NP)
    for j, r in enumerate(rows):
        bounds[j, : len(r)] = r
        bounds[j, len(r):] = r[-1] if len(r) else 0.0
    return bounds, n, li, ui


def ehvi_set_partition_tables(engine, bounds, n_bounds, lower_idx, upper_idx) -> None:
    """Install the partition in table form (tgp_set_ehvi_partition): bounds [P, Vmax], n_bounds [P], indices [K, P]."""
    b = np.ascontiguousarray(bounds, dtype=_NP)
    n = np.ascontiguousarray(n_bounds, dtype=np.int32)
    li = np.ascontiguousarray(lower_idx, dtype=np.int32)
    ui = np.ascontiguousarray(upper_idx, dtype=np.int32)
    if b.ndim != 2 or n.shape != (b.shape[0],) or li.ndim != 2 or li.shape != ui.shape or li.shape[1] != b.shape[0]:
        raise ValueError(f"bounds must be [P, Vmax], n_bounds [P] and the indices [K, P], got {b.shape}, {n.shape}, "
                         f"{li.shape} and {ui.shape}")
    engine._ehvi_owner = None   # whichever function object installed the previous partition no longer owns the engine's
    engine._chk(engine._lib.tgp_set_ehvi_partition(engine._h, int(b.shape[0]), b.ctypes.data, int(b.shape[1]), n.ctypes.data,
                                                   li.ctypes.data, ui.ctypes.data, int(li.shape[0])))


def ehvi_set_partition(engine, lower, upper) -> None:
    """Install the cells (lower, upper) [K, P] of the non-dominated region on ``engine`` -- the LEADING engine of the stack, the
    one :func:`ehvi_values` / :func:`ehvi_argmax` are called with first.  ``None`` or K = 0 clears the state."""
    if lower is None or np.asarray(lower).shape[0] == 0:
        engine._ehvi_owner = None
        engine._chk(engine._lib.tgp_set_ehvi_partition(engine._h, 0, None, 0, None, None, None, 0))
        return
    ehvi_set_partition_tables(engine, *ehvi_partition_tables(lower, upper))


def ehvi_moments(engine, mean, var):
    """The EHVI tail on caller-supplied moments: mean, var [P, M] objective-major (host arrays or CUDA tensors) -> [M]
    (tgp_ehvi_moments).  Needs a partition on the engine and no data."""
    m, v = _marginal_pair(mean, var)
    out, po = GPEngine._out(m, (m.shape[1],))
    engine._chk(engine._lib.tgp_ehvi_moments(engine._h, m.ptr, v.ptr, int(m.shape[1]), po, m.where))
    return out


def _handles(engines):
    engines = list(engines)
    if not engines:
        raise ValueError("a stack needs at least one engine")
    return engines, (C.c_void_p * len(engines))(*[e._h.value if hasattr(e._h, "value") else e._h for e in engines])


def ehvi_values(engines, Xq):
    """engines: one :class:`GPEngine` per objective (the first carries the partition); Xq [..., d] -> EHVI [...]: every
    engine's ``predict`` and the tail in one device call (tgp_ehvi_values)."""
    engines, hs = _handles(engines)
    a, lead, M = engines[0]._flat(Xq)
    out, po = GPEngine._out(a, lead)
    engines[0]._chk(engines[0]._lib.tgp_ehvi_values(hs, len(engines), a.ptr, M, po, a.where))
    return out


def ehvi_argmax(engines, Xq, index_base: int = 0):
    """-> (best EHVI, global index, best point [d] as numpy) over the candidates Xq [M, d]; the first index wins ties."""
    engines, hs = _handles(engines)
    a, _, M = engines[0]._flat(Xq)
    bv, bi = C.c_double(), C.c_int64()
    bx = np.empty(engines[0].d)
    engines[0]._chk(engines[0]._lib.tgp_ehvi_argmax(hs, len(engines), a.ptr, M, int(index_base), C.byref(bv), C.byref(bi),
                                                    bx.ctypes.data, a.where))
    return bv.value, bi.value, bx


EHVI_GRAD_MAX_POINTS = 2048  # points per tgp_ehvi_value_grad call (callers chunk)


def ehvi_grad_tile_width(P: int, V: int) -> int:
    """Candidates per workgroup of the EHVI gradient kernel: the largest power of two <= 8 whose three tables of
    24 P V C bytes fit 160 KiB of LDS.  A function of (P, V) alone; 2 at P = 4, V = 512."""
    C = 8
    while C > 1 and 24 * P * V * C > 160 * 1024:
        C //= 2
    return C


def ehvi_moments_grad(engine, mean, var):
    """The EHVI tail with the adjoints of the moments on caller-supplied moments: mean, var [P, M] objective-major ->
    (value [M], gmean [P, M], gvar [P, M]) (tgp_ehvi_moments_grad).  Needs a partition on the engine and no data."""
    m, v = _marginal_pair(mean, var)
    outs, ptrs = _value_grad_outputs(m, (m.shape[1],), v.shape)
    engine._chk(engine._lib.tgp_ehvi_moments_grad(engine._h, m.ptr, v.ptr, int(m.shape[1]), *ptrs, m.where))
    return outs


def ehvi_value_grad(engines, Xq):
    """engines: one :class:`GPEngine` per objective (the first carries the partition); Xq [M, d], 1 <= M <= 2048 ->
    (EHVI [M], its gradient [M, d]) in one device call: every engine's small-product posterior, the gradient tail, every
    engine's vector-Jacobian product and their sum (tgp_ehvi_value_grad)."""
    engines, hs = _handles(engines)
    a = _Arg(Xq)
    if len(a.shape) != 2 or a.shape[1] != engines[0].d:
        raise ValueError(f"Xq must be [M, {engines[0].d}], got shape {tuple(a.shape)}")
    M = int(a.shape[0])
    val, pv = GPEngine._out(a, (M,))
    grad, pg = GPEngine._out(a, (M, engines[0].d))
    engines[0]._chk(engines[0]._lib.tgp_ehvi_value_grad(hs, len(engines), a.ptr, M, pv, pg, a.where))
    return val, grad


def ehvi_last_ms(engine):
    """(summed time of the posterior sweeps, time of the tail kernel) of the engine's most recent EHVI call, in ms."""
    s, t = C.c_double(), C.c_double()
    engine._chk(engine._lib.tgp_ehvi_last_ms(engine._h, C.byref(s), C.byref(t)))
    return s.value, t.value


# ---- batch Monte-Carlo expected hypervolume improvement (tgp_qehvi_*; include/tgp.h) -----------------------------------
QEHVI_MAX_Q = _lib.QEHVI_MAX_Q
QEHVI_SLICES = 4  # cell slices of the qEHVI kernel (one wave each): slice w takes cells w, w + 4, ...


def qehvi_sample_chunk(P: int, q: int) -> int:
    """Samples the qEHVI kernel keeps in LDS at a time: the largest multiple of 64 with 8 P q C <= 32 KiB, at most 512.  A
    function of (P, q) alone; 128 at P = 4, q = 8."""
    return min(512, (32 * 1024 // (8 * P * q)) // 64 * 64)


def qehvi_sum_roundings(P: int, q: int, S: int, K: int) -> int:
    """The rounding count of the qEHVI kernel's documented summation: P + 1 per product, the 2^q - 1 terms of
    a (sample, cell), a lane's cells-of-its-slice x samples, the 3 additions over the slices, the 6 of the butterfly over the
    lanes and the division by S."""
    return (P + 1) + (2 ** q - 1) + -(-K // QEHVI_SLICES) * -(-S // 64) + 3 + 6 + 1


def _qehvi_eps(P: int, q: int, eps, where):
    e = _Arg(eps)
    if len(e.shape) != 3 or e.shape[0] != P or e.shape[1] != q:
        raise ValueError(f"eps must be [P={P}, q={q}, S], got {e.shape}")
    if e.where != where:
        raise ValueError("the moments or points and eps must live in the same place (both host or both device)")
    return e


def qehvi_moments(engine, mean, cov, eps, jitter: float = 1e-6):
    """The qEHVI tail on caller-supplied joint moments as the models return them: mean [P, ..., q], cov [P, ..., q, q]
    objective-major, eps [P, q, S] -> [...] (tgp_qehvi_moments).  Needs a partition on the engine and no data."""
    m, c = _moment_pair(mean, cov, "P, ...")
    P, lead, q = m.shape[0], m.shape[1:-1], m.shape[-1]
    e = _qehvi_eps(P, q, eps, m.where)
    out, po = GPEngine._out(m, lead)
    engine._chk(engine._lib.tgp_qehvi_moments(engine._h, m.ptr, c.ptr, _groups(lead), q, e.ptr, int(e.shape[2]), float(jitter), po,
                                              m.where))
    return out


def qehvi_values(engines, Xq, eps, jitter: float = 1e-6):
    """engines: one :class:`GPEngine` per objective (the first carries the partition); Xq [..., q, d], eps [P, q, S] ->
    qEHVI [...]: every engine's ``predict_joint`` and the tail in one device call (tgp_qehvi_values)."""
    engines, hs = _handles(engines)
    a, lead, q, G = _batch_points(engines[0].d, Xq)
    e = _qehvi_eps(len(engines), q, eps, a.where)
    out, po = GPEngine._out(a, lead)
    engines[0]._chk(engines[0]._lib.tgp_qehvi_values(hs, len(engines), a.ptr, G, q, e.ptr, int(e.shape[2]), float(jitter), po,
                                                     a.where))
    return out


QEHVI_GRAD_MAX_POINTS = 2048  # points (groups x q) per tgp_qehvi_value_grad call (callers chunk)


def qehvi_grad_sample_chunk(P: int, q: int) -> int:
    """Samples the qEHVI gradient kernel keeps in LDS at a time: besides the samples one adjoint slot per sample and cell
    slice, next to the factors, the means, the adjoint work matrices and the sums of gmean and Lbar -- the largest multiple
    of 64, at most 512, with 8 (5 P q C + P (2 q^2 + q + q (q + 3) / 2)) <= 160 KiB.  A function of (P, q) alone; 64 at
    P = 4, q = 8."""
    fixed = P * (2 * q * q + q + q * (q + 3) // 2)
    return min(512, ((160 * 1024 - 8 * fixed) // (8 * (QEHVI_SLICES + 1) * P * q)) // 64 * 64)


def qehvi_grad_sum_roundings(P: int, q: int, S: int, K: int) -> int:
    """The rounding count of one adjoint entry of the qEHVI gradient kernel ahead of the Cholesky adjoint:
    2 P - 3 per partial product (its P - 1 factors and their P - 2 products); the at most 2^(q-1) terms of a (sample, cell)
    that hold a point, once into a level's register sum and once per flush of a level into the wave's slot, over the cells of
    a slice; the 3 additions over the slices, the product with eps, the 6 of the butterfly, the 64-blocks, and the scaling
    by 1 / S (two roundings)."""
    return (2 * P - 3) + 2 ** (q - 1) * (1 + -(-K // QEHVI_SLICES)) + 3 + 1 + 6 + -(-S // 64) + 2


def qehvi_moments_grad(engine, mean, cov, eps, jitter: float = 1e-6):
    """The qEHVI tail with the adjoints of the joint moments on caller-supplied moments: mean [P, ..., q], cov [P, ..., q, q]
    objective-major, eps [P, q, S] -> (value [...], gmean [P, ..., q], gcov [P, ..., q, q] symmetric)
    (tgp_qehvi_moments_grad).  The value is :func:`qehvi_moments`' bit for bit.  Needs a partition and no data."""
    m, c = _moment_pair(mean, cov, "P, ...")
    P, lead, q = m.shape[0], m.shape[1:-1], m.shape[-1]
    e = _qehvi_eps(P, q, eps, m.where)
    outs, ptrs = _value_grad_outputs(m, lead, c.shape)
    engine._chk(engine._lib.tgp_qehvi_moments_grad(engine._h, m.ptr, c.ptr, _groups(lead), q, e.ptr, int(e.shape[2]), float(jitter),
                                                   *ptrs, m.where))
    return outs


def qehvi_value_grad(engines, Xq, eps, jitter: float = 1e-6):
    """engines: one :class:`GPEngine` per objective (the first carries the partition); Xq [G, q, d] with 1 <= G and
    G q <= 2048, eps [P, q, S] -> (qEHVI [G], its gradient [G, q, d]) in one device call: every engine's joint posterior,
    the gradient tail, every engine's vector-Jacobian product and their sum (tgp_qehvi_value_grad)."""
    engines, hs = _handles(engines)
    a = _Arg(Xq)
    if len(a.shape) != 3 or a.shape[2] != engines[0].d:
        raise ValueError(f"Xq must be [G, q, {engines[0].d}], got shape {tuple(a.shape)}")
    G, q = int(a.shape[0]), int(a.shape[1])
    e = _qehvi_eps(len(engines), q, eps, a.where)
    val, pv = GPEngine._out(a, (G,))
    grad, pg = GPEngine._out(a, tuple(a.shape))
    engines[0]._chk(engines[0]._lib.tgp_qehvi_value_grad(hs, len(engines), a.ptr, G, q, e.ptr, int(e.shape[2]), float(jitter),
                                                         pv, pg, a.where))
    return val, grad
