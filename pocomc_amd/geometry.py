"""``Geometry`` -- what ``pocomc/geometry.py:31-59`` (+ ``pocomc/student.py:5-85``) hands the MCMC step
(``t_mean, t_cov, t_nu, normal_mean, normal_cov``: SURVEY.md section 8(a) G1), fitted on the device.

``fit`` takes the sample where it lives -- theta is the float32 output of ``flow.forward`` on the GPU, the pool's ``u``
a float64 device array -- and runs three reductions there (``csrc/pool.hip``): weighted first / second moments
(``pmc_moments``), the systematic resampling of ``geometry.py:52`` (``pmc_resample_systematic``) and the per-column
median of ``student.py:45`` (``pmc_column_medians``: one segmented radix sort).  Only ``D`` and ``D x D`` numbers
come back.

What ``fit_mvstud`` (``student.py:5-85``) really computes
--------------------------------------------------------
Its EM loop starts from ``mu = median``, ``Sigma = cov * (n-1)/n + diag(var)/n``, ``nu = 20`` (``:45-48``) and first
updates ``nu`` through ``opt_nu`` (``:35-42``): if ``func0(1e300) >= 0`` it returns ``nu = inf`` -- and ``fit_mvstud``
returns the START values (``:59-60``) -- otherwise it calls ``scipy.optimize.bisect(func0, 1e-300, 1e300)`` with the
default ``maxiter=100``, which cannot converge (100 halvings of a 1e300-wide bracket leave 7.9e269) and raises
``RuntimeError``.  At ``nu = 1e300`` every EM weight ``(nu + dim) / (nu + delta)`` is exactly 1.0 in float64, so
``func0(1e300)`` does not depend on the data at all: it is the constant evaluated in :func:`_func0_at_1e300` (0.0 with
this scipy: psi and log agree to the last bit at 5e299).  The reference's t-fit is therefore ALWAYS
``(median, start Sigma, inf)`` with ``t_nu`` replaced by 1e6 (``geometry.py:58-59``); a build whose libm made the
constant negative would raise from ``bisect`` on every call.  This class reproduces exactly that: the start values from
the device, the same constant test, the same error.

That "always ``inf``" holds for ``Geometry(student="reference")``, the default.  ``Geometry(student="em")`` runs the fit
the reference sets out to do (``student.py:53-85``) with a root finder for ``nu`` that works -- a bracket of
``[0.1, 1e4]`` instead of ``[1e-300, 1e300]`` -- from the same start values, on the device (``pmc_student_em``,
``csrc/student.hip``; the algorithm is stated in ``include/pocomc_amd.h``).  Gaussian rows leave it at the first
iteration with ``nu = inf`` and the start values: the reference mode's result, bit for bit.  Heavy-tailed rows give the
finite ``nu`` the t-preconditioned Crank-Nicolson step was written for.

``Geometry(student="em_weighted")`` fits on the weights themselves (``pmc_student_em_weighted``): every row enters each sum
of the EM with ``w_r / sum w`` instead of through one systematic resample, so the fit draws no random number, needs no
second moments pass and no medians, and is the same on every call.  It starts from the weighted mean and the weighted
scatter ``S / V1`` of the moments pass that forms ``normal_mean`` / ``normal_cov``, and runs up to ``n_dim = 157``, the
width of the MCMC step.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _func0_at_1e300(dim: int) -> float:
    """``func0(1e300)`` of ``student.py:36-38`` with its data terms at their exact values (weights == 1.0):
    ``sum(log w) / n = 0.0`` and ``sum(w) / n = 1.0``; same operation order."""
    from scipy import special
    nu = 1e300
    return float(-special.psi(nu / 2) + np.log(nu / 2) + 0.0 - 1.0 + 1 + special.psi((nu + dim) / 2)
                 - np.log((nu + dim) / 2))


def _as_device(a, keep32=True):
    """Device view of a sample: float32 stays float32 (theta), everything else becomes float64."""
    dev = _lib.require_gpu()
    if isinstance(a, torch.Tensor):
        t = a
    else:
        a = np.asarray(a)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if (keep32 and a.dtype == np.float32) else np.float64))
    if t.dtype != torch.float32 or not keep32:
        t = t.to(torch.float64)
    return t.to(dev).contiguous()


def moments(x, idx=None, w=None):
    """``(mean [D], S [D, D], V1, V2)`` of the rows ``x[idx]`` with weights ``w`` on the device (``pmc_moments``);
    the results come back as float64 numpy arrays."""
    lib = _lib.load()
    n = int(idx.numel()) if idx is not None else int(x.shape[0])
    D = int(x.shape[1])
    dev = x.device
    mean = torch.empty(D, dtype=torch.float64, device=dev)
    S = torch.empty(D, D, dtype=torch.float64, device=dev)
    v = torch.empty(2, dtype=torch.float64, device=dev)
    nbytes = int(lib.pmc_moments_workspace_bytes(D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f32 = x.dtype == torch.float32
    with torch.cuda.device(dev):
        _lib.check(lib.pmc_moments(None if f32 else _lib.ptr(x), _lib.ptr(x) if f32 else None,
                                   _lib.ptr(idx) if idx is not None else None, _lib.ptr(w) if w is not None else None,
                                   n, D, _lib.ptr(mean), _lib.ptr(S), _lib.ptr(v), _lib.ptr(ws), nbytes,
                                   _lib.stream_handle()), "pmc_moments")
    out = torch.cat([mean, S.reshape(-1), v]).cpu().numpy()
    return out[:D], out[D:D + D * D].reshape(D, D), float(out[-2]), float(out[-1])


def column_medians(x, idx=None):
    """``np.median(x[idx], axis=0)`` on the device (``pmc_column_medians``), in the input's precision; NaN for a column
    that holds a NaN, like numpy."""
    lib = _lib.load()
    n = int(idx.numel()) if idx is not None else int(x.shape[0])
    D = int(x.shape[1])
    dev = x.device
    f32 = x.dtype == torch.float32
    med = torch.empty(D, dtype=x.dtype, device=dev)
    nbytes = int(lib.pmc_column_medians_workspace_bytes(n, D, int(f32)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pmc_column_medians(None if f32 else _lib.ptr(x), _lib.ptr(x) if f32 else None,
                                          _lib.ptr(idx) if idx is not None else None, n, D,
                                          None if f32 else _lib.ptr(med), _lib.ptr(med) if f32 else None, _lib.ptr(ws),
                                          nbytes, _lib.stream_handle()), "pmc_column_medians")
    return med.cpu().numpy()


STUDENT_MAX_D = 128                                                        # PMC_STUDENT_MAX_D
STUDENT_STATUS = ("converged", "max_iter", "nu_inf", "lower_clamp", "not_pd", "nonfinite")     # PMC_STUDENT_*


def student_em(x, idx, mu, sigma, tol=1e-6, max_iter=100):
    """The EM fit of a multivariate Student-t to the rows ``x[idx]`` (device tensor, float64 or float32; ``idx`` int64
    device tensor or None) from the start values ``mu`` [D], ``sigma`` [D, D] (numpy), on the device (``pmc_student_em``).
    Returns ``(mu, sigma, info)``: float64 numpy arrays and ``dict(nu=, iterations=, status=, host_reads=)`` with
    ``status`` one of ``STUDENT_STATUS`` and ``nu = inf`` for rows no heavier-tailed than a normal."""
    lib = _lib.load()
    n = int(idx.numel()) if idx is not None else int(x.shape[0])
    D = int(x.shape[1])
    if D > STUDENT_MAX_D:
        raise ValueError(f"student_em: n_dim = {D} is above {STUDENT_MAX_D}, the largest the device fit supports")
    if n <= D:
        raise ValueError(f"student_em: {n} rows cannot fit a {D}-dimensional Student-t (more rows than dimensions needed)")
    dev = x.device
    start = np.concatenate([np.asarray(mu, dtype=np.float64).reshape(D), np.asarray(sigma, dtype=np.float64).reshape(D * D)])
    io = torch.from_numpy(start).to(dev)
    nbytes = int(lib.pmc_student_em_workspace_bytes(n, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res = (C.c_double * 4)()
    f32 = x.dtype == torch.float32
    with torch.cuda.device(dev):
        _lib.check(lib.pmc_student_em(None if f32 else _lib.ptr(x), _lib.ptr(x) if f32 else None,
                                      _lib.ptr(idx) if idx is not None else None, n, D, _lib.ptr(io),
                                      C.c_void_p(io.data_ptr() + 8 * D), float(tol), int(max_iter), res, _lib.ptr(ws), nbytes,
                                      _lib.stream_handle()), "pmc_student_em")
    out = io.cpu().numpy()
    info = dict(nu=float(res[0]), iterations=int(res[1]), status=STUDENT_STATUS[int(res[2])], host_reads=int(res[3]))
    return out[:D], out[D:].reshape(D, D), info


STUDENT_W_MAX_D = 157                                                      # PMC_STUDENT_W_MAX_D


def student_em_weighted(x, w, mu, sigma, tol=1e-6, max_iter=100):
    """The EM fit of a multivariate Student-t to the rows ``x`` (device tensor, float64 or float32) with the weights ``w``
    (float64 device tensor [n], ``>= 0``, any scale) from the start values ``mu`` [D], ``sigma`` [D, D] (numpy), on the
    device (``pmc_student_em_weighted``).  Returns ``(mu, sigma, info)`` like :func:`student_em`; ``info`` also holds
    ``rows_positive`` (rows with ``w > 0``: the others are never read) and ``ess`` (Kish, ``(sum w)^2 / sum w^2``).
    Weights that are negative or not finite, or no more rows of positive weight than dimensions: ``ValueError``."""
    lib = _lib.load()
    n, D = int(x.shape[0]), int(x.shape[1])
    if D > STUDENT_W_MAX_D:
        raise ValueError(f"student_em_weighted: n_dim = {D} is above {STUDENT_W_MAX_D}, the largest the device fit supports")
    if n <= D:
        raise ValueError(f"student_em_weighted: {n} rows cannot fit a {D}-dimensional Student-t (more rows of positive "
                         "weight than dimensions needed)")
    if w.dtype != torch.float64 or int(w.numel()) != n:
        raise ValueError("student_em_weighted: w must be a float64 tensor with one weight per row")
    dev = x.device
    start = np.concatenate([np.asarray(mu, dtype=np.float64).reshape(D), np.asarray(sigma, dtype=np.float64).reshape(D * D)])
    io = torch.from_numpy(start).to(dev)
    nbytes = int(lib.pmc_student_em_weighted_workspace_bytes(n, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res = (C.c_double * 6)()
    f32 = x.dtype == torch.float32
    with torch.cuda.device(dev):
        rc = lib.pmc_student_em_weighted(None if f32 else _lib.ptr(x), _lib.ptr(x) if f32 else None, _lib.ptr(w), n, D,
                                         _lib.ptr(io), C.c_void_p(io.data_ptr() + 8 * D), float(tol), int(max_iter), res,
                                         _lib.ptr(ws), nbytes, _lib.stream_handle())
    if rc != 0:
        msg = (lib.pmc_last_error() or b"").decode()
        if "weights must be" in msg or "rows of positive weight" in msg:       # (the weight check: the caller's input)
            raise ValueError(msg)
        _lib.check(rc, "pmc_student_em_weighted")
    out = io.cpu().numpy()
    info = dict(nu=float(res[0]), iterations=int(res[1]), status=STUDENT_STATUS[int(res[2])], host_reads=int(res[3]),
                rows_positive=int(res[4]), ess=float(res[5]))
    return out[:D], out[D:].reshape(D, D), info


class Geometry:
    """``pocomc/geometry.py:5-59``.  ``student``: ``"reference"`` (default) reproduces the reference's t-fit, which always
    ends at its start values with ``t_nu = 1e6``; ``"em"`` fits location, scatter and degrees of freedom by EM on the
    device (module docstring) and records ``student_info = dict(iterations=, status=, nu=)``; ``"em_weighted"`` runs that
    fit on the weights themselves instead of on a resample (no random number, ``n_dim <= 157``) and adds ``rows_positive=``
    and ``ess=`` to ``student_info``."""

    student = "reference"                      # (objects unpickled from checkpoints older than the attribute)
    student_info = None

    def __init__(self, student="reference"):
        if student not in ("reference", "em", "em_weighted"):
            raise ValueError(f"Invalid student {student}. Options are 'reference', 'em' or 'em_weighted'.")
        self.student = student
        self.student_info = None
        self.normal_mean = self.normal_cov = self.t_mean = self.t_cov = self.t_nu = None

    def fit(self, theta, weights=None):
        """``theta``: (n, D) numpy array or torch tensor (device tensors are used in place); ``weights``: (n,) or None."""
        from .tools import systematic_resample
        th = _as_device(theta)
        n, D = int(th.shape[0]), int(th.shape[1])
        if self.student == "em_weighted":
            return self._fit_weighted(th, weights)
        if self.student == "em":                                           # (before any launch)
            if D > STUDENT_MAX_D:
                raise ValueError(f"Geometry.fit: student='em' supports n_dim <= {STUDENT_MAX_D}, got {D}")
            if n <= D:
                raise ValueError(f"Geometry.fit: student='em' needs more rows than dimensions, got {n} rows of {D}")
        if weights is None:
            mean, S, _, _ = moments(th)
            self.normal_mean = mean                                        # np.mean(theta, axis=0)
            self.normal_cov = S / (n - 1)                                  # np.cov(theta.T)
            idx = None
        else:
            w = _as_device(weights, keep32=False)
            mean, S, v1, v2 = moments(th, None, w)
            self.normal_mean = mean                                        # np.average(theta, axis=0, weights=weights)
            self.normal_cov = S / (v1 - v2 / v1)                           # np.cov(theta.T, aweights=weights): ddof = 1
            idx = systematic_resample(n, weights=w, device_indices=True)   # geometry.py:52 (one np.random.random())
        # ---- fit_mvstud(sample): its start values are its result (module docstring)
        Ss = S if idx is None else moments(th, idx)[1]                     # (unweighted: the scatter matrix just formed)
        med = column_medians(th, idx)                                      # student.py:45
        var = np.diag(Ss) / n
        if th.dtype == torch.float32:
            var = var.astype(np.float32)                                   # np.var of a float32 array is a float32
        sigma = Ss / n + (1 / n) * np.diag(var)                            # student.py:46-47: cov*(n-1)/n + diag(var)/n
        if self.student == "em" or _func0_at_1e300(D) >= 0:                # student.py:39-40 -> :59-60
            nu = np.inf
        else:
            raise RuntimeError("Failed to converge after 100 iterations (scipy.optimize.bisect(func0, 1e-300, 1e300), "
                               "pocomc/student.py:42)")
        # The reference fails loudly on such input (NaN / inf rows: scipy's bisect raises on a NaN bracket; a singular
        # scatter matrix: linalg.solve in the EM step raises LinAlgError) -- the shortcut above must not turn that into a
        # silent NaN geometry that surfaces later, or never
        if not (np.isfinite(med).all() and np.isfinite(sigma).all()):
            raise ValueError("Geometry.fit: non-finite values in theta (median / scatter matrix are not finite)")
        # (the reference's own failure condition: ``linalg.solve(cov, ...)`` of the EM step, student.py:70, raises on an
        #  exactly singular matrix only -- near-singular or slightly indefinite scatter matrices pass there and pass here)
        try:
            np.linalg.solve(sigma, np.eye(D))
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("Geometry.fit: the scatter matrix of theta is singular (student.py:70 solves with it)")
        if self.student == "em":
            med, sigma, info = student_em(th, idx, med, sigma)
            if info["status"] == "not_pd":
                raise np.linalg.LinAlgError(f"Geometry.fit: the scatter matrix of the Student-t fit is not positive definite "
                                            f"(EM iteration {info['iterations']})")
            if info["status"] == "nonfinite":
                raise ValueError(f"Geometry.fit: non-finite values in the Student-t fit (EM iteration {info['iterations']})")
            nu = info["nu"]
            self.student_info = dict(iterations=info["iterations"], status=info["status"], nu=nu)
        self.t_mean, self.t_cov, self.t_nu = med, sigma, nu
        if not np.isfinite(self.t_nu):
            self.t_nu = 1e6                                                # geometry.py:58-59

    def _fit_weighted(self, th, weights):
        """``student="em_weighted"``: one moments pass, then the EM on the weights (``None``: ones).  The fields are set
        together at the end: a fit that raises leaves the geometry as it was."""
        n, D = int(th.shape[0]), int(th.shape[1])
        if D > STUDENT_W_MAX_D:                                            # (before any launch)
            raise ValueError(f"Geometry.fit: student='em_weighted' supports n_dim <= {STUDENT_W_MAX_D}, got {D}")
        if n <= D:
            raise ValueError(f"Geometry.fit: student='em_weighted' needs more rows of positive weight than dimensions, "
                             f"got {n} rows of {D}")
        if weights is None:
            w = torch.ones(n, dtype=torch.float64, device=th.device)
            mean, S, v1, v2 = moments(th)
            normal_cov = S / (n - 1)                                       # np.cov(theta.T)
        else:
            w = _as_device(weights, keep32=False)
            mean, S, v1, v2 = moments(th, None, w)
            normal_cov = S / (v1 - v2 / v1)                                # np.cov(theta.T, aweights=weights): ddof = 1
        sigma = S / v1                                                     # the ML-normalised weighted scatter
        if not (np.isfinite(mean).all() and np.isfinite(sigma).all()):
            raise ValueError("Geometry.fit: non-finite values in theta or the weights (weighted mean / scatter matrix are "
                             "not finite)")
        try:
            np.linalg.solve(sigma, np.eye(D))
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("Geometry.fit: the weighted scatter matrix of theta is singular")
        mu, sigma, info = student_em_weighted(th, w, mean, sigma)
        if info["status"] == "not_pd":
            raise np.linalg.LinAlgError(f"Geometry.fit: the scatter matrix of the Student-t fit is not positive definite "
                                        f"(EM iteration {info['iterations']})")
        if info["status"] == "nonfinite":
            raise ValueError(f"Geometry.fit: non-finite values in the Student-t fit (EM iteration {info['iterations']})")
        self.normal_mean, self.normal_cov = mean, normal_cov
        self.student_info = dict(iterations=info["iterations"], status=info["status"], nu=info["nu"],
                                 rows_positive=info["rows_positive"], ess=info["ess"])
        self.t_mean, self.t_cov = mu, sigma
        self.t_nu = info["nu"] if np.isfinite(info["nu"]) else 1e6         # geometry.py:58-59
