"""``Prior`` -- host-side mirror of ``pocomc/prior.py``: a product of frozen
``scipy.stats`` distributions.  It is a host black box like the likelihood
(SURVEY.md section 2 row 8); uniform / normal factors are evaluated with one vectorised numpy
expression instead of one scipy call per dimension (same values).

The MCMC step can evaluate it on the device instead (``device_descriptor``, ``include/pocomc_amd.h`` pmc_prior_t):
``device="auto"`` does so for products of uniform / normal factors (the device's values are scipy's bit for bit),
``device=True`` for every family in ``DEVICE_FAMILIES`` (scipy's values to ~1e-12 relative, the same support),
``device=False`` never.

``DevicePrior`` is the other kind of prior: any joint density, written once as a GPU function (``logpdf_device``), that the
MCMC step calls on the device like a device likelihood (``Sampler(device_likelihood=True, device_prior=True)``).

``FlowPrior`` is such a prior made of a finished run: its trained flow and fitted scaler are a normalised density on the
prior's box, evaluated by two launches around the flow's own forward kernel (``csrc/flow_prior.hip``).

``JointPrior`` puts such a flow prior on some columns of ``x`` and a table of scipy factors on the others, in the same number
of launches (``csrc/joint_prior.hip``); its blocks form takes several flow priors on disjoint blocks of columns, in B + 2
launches and still one pass over ``x``.

``GaussianPrior`` is a correlated normal, ``N(mean, cov)``: one float64 launch (``csrc/gauss_prior.hip``), alone or as a block of
a ``JointPrior`` next to flow blocks and a table.

``TruncatedGaussianPrior`` is that normal restricted to a box and normalised: the box's mass is one number, computed once on
the host, and the same launch tests the box (``pmc_gauss_box_logpdf``); alone or as a block of a ``JointPrior``.

``GaussianMixturePrior`` is a weighted sum of up to 32 such normals on up to 64 columns, closed by a log-sum-exp: one float64
launch (``csrc/gauss_mix_prior.hip``), alone or as a block of a ``JointPrior``; ``from_samples`` fits it by EM in numpy.

``KDEPrior`` is a weighted Gaussian kernel density estimate of up to 65536 samples on up to 16 columns with one shared
bandwidth matrix: a row is whitened once and the kernels are an n x M streaming log-sum-exp, one float64 launch
(``csrc/kde_prior.hip``), alone or as a block of a ``JointPrior``; nothing is fitted.

Next to a HOST likelihood ``FlowPrior`` and ``JointPrior`` (without Gaussian blocks) can be evaluated by the MCMC step
itself (``step_stage``, kernel option ``step_prior``): the same
three launches on the step's stream, on the device's copy of x', while the host evaluates the likelihood."""
from __future__ import annotations

import numpy as np

# scipy.stats name -> PMC_PRIOR_* family code (include/pocomc_amd.h)
DEVICE_FAMILIES = {"uniform": 1, "norm": 2, "truncnorm": 3, "loguniform": 4, "reciprocal": 4, "lognorm": 5,
                   "halfnorm": 6, "expon": 7, "gamma": 8, "invgamma": 9, "beta": 10, "cauchy": 11, "halfcauchy": 12,
                   "laplace": 13, "t": 14}
NPAR = 4           # PMC_PRIOR_NPAR: three family constants, then log(scale)


def _log_gauss_mass(a, b):
    """log of the normal mass of [a, b], as scipy's truncnorm computes it (so that far-tail truncations agree)."""
    try:
        from scipy.stats._continuous_distns import _log_gauss_mass as lgm
        return float(lgm(a, b))
    except ImportError:                                   # (private helper moved: take it from truncnorm.logpdf itself)
        from scipy.stats import norm, truncnorm
        z = 0.5 * (a + b) if np.isfinite(a) and np.isfinite(b) else (b - 1.0 if np.isfinite(b) else
                                                                      a + 1.0 if np.isfinite(a) else 0.0)
        return float(norm.logpdf(z) - truncnorm.logpdf(z, a, b))


def _factor(j, d):
    """(family code, loc, scale, (p0, p1, p2)) of factor j for the device, or ValueError naming it.  The constants are
    computed in float64 the way scipy's ``_logpdf`` computes them (scipy.special)."""
    import scipy.special as sc
    dist = getattr(d, "dist", None)
    name = getattr(dist, "name", None)
    if name is None or not hasattr(d, "args") or not hasattr(d, "kwds"):
        raise ValueError(f"Prior(device=True): dimension {j}: {type(d).__name__} is not a frozen scipy.stats distribution")
    if name not in DEVICE_FAMILIES:
        raise ValueError(f"Prior(device=True): dimension {j}: the device does not evaluate scipy.stats.{name} "
                         f"(it evaluates {', '.join(sorted(DEVICE_FAMILIES))})")
    try:
        shapes, loc, scale = dist._parse_args(*d.args, **d.kwds)
        shapes = tuple(float(v) for v in shapes)
        loc, scale = float(loc), float(scale)
        ok = bool(np.all(dist._argcheck(*shapes))) if shapes else True
    except (TypeError, ValueError) as e:
        raise ValueError(f"Prior(device=True): dimension {j}: scipy.stats.{name}: {e}") from None
    if not (ok and np.isfinite(loc) and np.isfinite(scale) and scale > 0 and not np.isnan(shapes).any()):
        raise ValueError(f"Prior(device=True): dimension {j}: scipy.stats.{name}{shapes} with loc={loc}, scale={scale} "
                         "has invalid parameters")
    p = (0.0, 0.0, 0.0)
    if name == "truncnorm":
        a, b = shapes
        p = (a, b, _log_gauss_mass(a, b))
    elif name in ("loguniform", "reciprocal"):
        a, b = shapes
        p = (a, b, float(np.log(np.log(b) - np.log(a))))
    elif name == "lognorm":
        s, = shapes
        p = (s, 2 * (s * s), 0.0)
    elif name == "halfnorm":
        p = (0.0, 0.0, float(0.5 * np.log(2.0 / np.pi)))
    elif name == "gamma":
        a, = shapes
        p = (a - 1.0, 0.0, float(sc.gammaln(a)))
    elif name == "invgamma":
        a, = shapes
        p = (a + 1, 0.0, float(sc.gammaln(a)))
    elif name == "beta":
        a, b = shapes
        p = (a - 1.0, b - 1.0, float(sc.betaln(a, b)))
    elif name == "cauchy":
        p = (0.0, 0.0, float(np.log(np.pi)))
    elif name == "halfcauchy":
        p = (0.0, 0.0, float(np.log(2.0 / np.pi)))
    elif name == "t":
        df, = shapes
        p = (df, np.inf, 0.0) if np.isinf(df) else \
            (df, (df + 1) / 2, float(np.log(sc.poch(0.5 * df, 0.5)) - 0.5 * (np.log(df) + np.log(np.pi))))
    return DEVICE_FAMILIES[name], loc, scale, p


class Prior:
    def __init__(self, dists=None, device="auto"):
        if device not in ("auto", True, False):
            raise ValueError(f"Prior: device must be 'auto', True or False, got {device!r}")
        self.dists = dists
        self.device = device
        self._fast = None
        try:
            kinds = [d.dist.name for d in dists]
            if all(k in ("uniform", "norm") for k in kinds):
                loc = np.array([d.kwds.get("loc", d.args[0] if len(d.args) > 0 else 0.0) for d in dists], float)
                scale = np.array([d.kwds.get("scale", d.args[1] if len(d.args) > 1 else 1.0) for d in dists], float)
                self._fast = (np.array([k == "uniform" for k in kinds]), loc, scale)
        except Exception:
            self._fast = None
        if device is True:
            self.device_table()                           # every factor must be one the device evaluates

    # ---------------------------------------------------------------- device
    def device_table(self):
        """The device's description of the prior as numpy arrays -- ``family`` (int32 [D], PMC_PRIOR_*), ``loc``,
        ``scale`` (float64 [D]) and ``par`` (float64 [NPAR, D]: the family constants of include/pocomc_amd.h, then
        log(scale); None when every factor is uniform / normal) -- or None when the prior stays on the host
        (``device=False``, or ``"auto"`` with a factor that is not uniform / normal).  ``device=True`` raises ValueError
        for the first factor the device does not evaluate.  No torch, no GPU."""
        if self.device is False:
            return None
        if self.device == "auto":
            if self._fast is None:
                return None
            is_u, loc, scale = self._fast
            return dict(family=np.where(is_u, 1, 2).astype(np.int32), loc=loc.copy(), scale=scale.copy(), par=None)
        rows = [_factor(j, d) for j, d in enumerate(self.dists)]
        family = np.array([r[0] for r in rows], np.int32)
        loc = np.array([r[1] for r in rows], float)
        scale = np.array([r[2] for r in rows], float)
        par = None
        if (family > 2).any():
            par = np.empty((NPAR, len(rows)))
            par[:3] = np.array([r[3] for r in rows], float).T
            par[3] = np.log(scale)
        return dict(family=family, loc=loc, scale=scale, par=par)

    def device_descriptor(self, device=None):
        """``pmc_prior_t`` for the MCMC engine (``device_table`` uploaded once), or ``None`` when the prior stays on the
        host (then ``logpdf`` is called on the host like any black box)."""
        if getattr(self, "_ddesc", None) is None:
            tab = self.device_table()
            if tab is None:
                return None
            import torch
            from . import _lib
            dev = device if device is not None else _lib.require_gpu()
            arrs = [tab["family"], tab["loc"], tab["scale"]] + ([] if tab["par"] is None else [tab["par"]])
            self._dtensors = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]
            n_ext = int((tab["family"] > 2).sum())
            self._ddesc = _lib.pmc_prior_t(family=self._dtensors[0].data_ptr(), loc=self._dtensors[1].data_ptr(),
                                           scale=self._dtensors[2].data_ptr(), D=len(tab["family"]), reserved=0,
                                           par=self._dtensors[3].data_ptr() if n_ext else None, n_extended=n_ext,
                                           reserved2=0)
        return self._ddesc

    def __getstate__(self):
        st = self.__dict__.copy()
        st.pop("_ddesc", None); st.pop("_dtensors", None)
        return st

    def __setstate__(self, st):
        st.setdefault("device", "auto")                   # (states saved before the choice existed)
        self.__dict__.update(st)

    def logpdf(self, x):
        """``pocomc/prior.py:70-100``."""
        if self._fast is not None:
            is_u, loc, scale = self._fast
            x = np.asarray(x, dtype=float)
            out = np.zeros(len(x))
            if is_u.any():
                xu = x[:, is_u]
                inside = np.all((xu >= loc[is_u]) & (xu <= loc[is_u] + scale[is_u]), axis=1)
                out += np.where(inside, -np.sum(np.log(scale[is_u])), -np.inf)
            if (~is_u).any():
                z = (x[:, ~is_u] - loc[~is_u]) / scale[~is_u]
                out += np.sum(-0.5 * z * z - np.log(scale[~is_u]) - 0.5 * np.log(2 * np.pi), axis=1)
            return out
        logp = np.zeros(len(x))
        for i, dist in enumerate(self.dists):
            logp += dist.logpdf(x[:, i])
        return logp

    def rvs(self, size=1):
        """``pocomc/prior.py:102-133``."""
        return np.transpose([dist.rvs(size=size) for dist in self.dists])

    @property
    def bounds(self):
        """``pocomc/prior.py:135-153``."""
        return np.array([dist.support() for dist in self.dists])

    @property
    def dim(self):
        return len(self.dists)


class DevicePrior:
    """A prior in pocoMC's own protocol (``logpdf / rvs / bounds / dim``, the class its documentation asks for where a
    prior is no product of independent factors: an ordering constraint, a hierarchical prior, a simplex) around ONE
    function that lives on the GPU.

    ``logpdf_device(x)``  gets an ``(n, D)`` float64 tensor on the device (rows in walker order; inside the MCMC steps a
                          column-major view, on the step's stream) and returns an ``(n,)`` float64 or float32 tensor on that
                          device: the log density of every row, -inf outside the support.  Row-wise, free of side effects,
                          and it does not keep its input, whose buffer is reused.
    ``bounds``            ``(D, 2)`` floats, the box the support lies in (+-inf or NaN: unbounded on that side);
    ``rvs(size)``         draws ``(size, D)`` numpy rows from the prior (host: used once, before the first iteration);
    ``dim``               D, checked against ``bounds`` when given.

    ``logpdf(x)`` (numpy in, numpy out) uploads, calls ``logpdf_device`` and downloads: one source of truth, usable wherever
    a prior is.  There is no ``device_descriptor``: the device has no table for it, it calls the function."""

    def __init__(self, logpdf_device, bounds, rvs, dim=None):
        if not callable(logpdf_device):
            raise ValueError(f"DevicePrior: logpdf_device must be callable, got {type(logpdf_device).__name__}")
        if not callable(rvs):
            raise ValueError(f"DevicePrior: rvs must be callable, got {type(rvs).__name__}")
        try:
            b = np.array(bounds, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("DevicePrior: bounds must be a (D, 2) array of floats") from None
        if b.ndim != 2 or b.shape[1] != 2 or b.shape[0] < 1:
            raise ValueError(f"DevicePrior: bounds must have shape (D, 2), got {b.shape}")
        lo = np.where(np.isnan(b[:, 0]), -np.inf, b[:, 0])
        hi = np.where(np.isnan(b[:, 1]), np.inf, b[:, 1])
        if not np.all(lo < hi):
            j = int(np.argmin(lo < hi))
            raise ValueError(f"DevicePrior: bounds of dimension {j}: lower {b[j, 0]} is not below upper {b[j, 1]}")
        if dim is not None and (int(dim) != dim or int(dim) != len(b)):
            raise ValueError(f"DevicePrior: dim = {dim!r} but bounds has {len(b)} rows")
        self.logpdf_device = logpdf_device
        self._bounds = b
        self._rvs = rvs

    def logpdf(self, x):
        import torch
        from . import _lib
        from .mcmc import device_logp
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"DevicePrior.logpdf: expected shape (n, {self.dim}), got {x.shape}")
        dev = _lib.require_gpu()
        out = device_logp(self.logpdf_device(torch.from_numpy(x).to(dev)), len(x), dev)
        return out.to(torch.float64).cpu().numpy()

    def rvs(self, size=1):
        x = np.asarray(self._rvs(size), dtype=np.float64)
        if x.shape != (size, self.dim):
            raise ValueError(f"DevicePrior.rvs: expected shape ({size}, {self.dim}) from rvs, got {x.shape}")
        return x

    @property
    def bounds(self):
        return self._bounds.copy()

    @property
    def dim(self):
        return len(self._bounds)


def _step_stage(owner, flow_prior, n, device, joint=None):
    """``pmc_prior_stage_t`` of ``owner`` (a ``FlowPrior``, or a ``JointPrior`` with ``joint = (flow_cols, rdesc, rest_cols)``)
    for the ``n`` rows of one step engine, with one workspace set of its own.  The descriptor keeps what it points into alive
    (``_keep``): the engine that holds it holds the tensors, the prior's descriptors and the prior."""
    import ctypes as C
    import torch
    from . import _lib
    from .mcmc import _on_device, _pinned_take
    flow, n = flow_prior.flow, int(n)
    if n < 1:
        raise ValueError(f"{type(owner).__name__}.step_stage: n must be at least 1, got {n}")
    dev = torch.device(flow.device)
    if device is not None:
        _on_device(torch.empty(0, device=dev), device, f"{type(owner).__name__}.step_stage")
    Df = flow_prior.dim
    with torch.cuda.device(dev):
        ws = dict(u32=torch.empty(n, Df, dtype=torch.float32, device=dev),
                  z=torch.empty(n, Df, dtype=torch.float32, device=dev),
                  lp32=torch.empty(n, dtype=torch.float32, device=dev),
                  ldj=torch.empty(n, dtype=torch.float64, device=dev),
                  rest_logp=torch.empty(n, dtype=torch.float64, device=dev) if joint is not None else None,
                  inside=torch.empty(n, dtype=torch.int32, device=dev),
                  count=torch.zeros(2, dtype=torch.int64, device=dev))
        image, per_t = None, 0
        if flow.precision == "bf16":
            _, image, per_t = flow._bf16_image()
    h_count = _pinned_take((2,), torch.int64)
    h_count.zero_()
    flow_cols, rdesc, rest_cols = joint if joint is not None else (None, None, None)
    desc = _lib.pmc_prior_stage_t(
        scaler=C.cast(C.pointer(flow_prior._sdesc), C.c_void_p), maf=C.cast(C.pointer(flow._desc), C.c_void_p),
        image16=image.data_ptr() if image is not None else None, image_per_transform=int(per_t),
        flow_cols=flow_cols.data_ptr() if joint is not None else None,
        rest=C.cast(C.pointer(rdesc), C.c_void_p) if joint is not None else None,
        rest_cols=rest_cols.data_ptr() if joint is not None else None,
        u32=ws["u32"].data_ptr(), z=ws["z"].data_ptr(), lp32=ws["lp32"].data_ptr(), ldj=ws["ldj"].data_ptr(),
        rest_logp=ws["rest_logp"].data_ptr() if joint is not None else None, inside=ws["inside"].data_ptr(),
        count=ws["count"].data_ptr(), h_count=h_count.data_ptr())
    desc._keep = (owner, ws, image, joint)
    desc.counts = h_count             # (the pinned words: the engine reads them, and recycles the tensor with its own)
    return desc


class FlowPrior:
    """The density a finished run leaves behind, as a prior: a trained ``Flow`` and a fitted diagonal ``Reparameterize``,

        ``log p(x) = flow.log_prob(u(x)) - log|dx/du|``,   ``u = scaler.forward(x)``,

    normalised on the scaler's box.  The posterior of one experiment becomes the prior of the next; the evidence of the second
    run is then that of its data given the first run's.

    ``logpdf_device(x)``  the ``DevicePrior`` contract: an ``(n, D)`` float64 tensor on the flow's device in, an ``(n,)``
                          float64 tensor out, on the current stream, in three launches -- ``pmc_flow_prior_pre`` (u as
                          float32, the scaler's log-determinant, the support test), the flow's own forward call with
                          ``log_prob`` (so a ``precision="bf16"`` flow keeps its matrix-core kernel), ``pmc_flow_prior_post``.
                          No host synchronisation; no copy of ``x`` when it is C-contiguous or the MCMC step's column-major
                          view (any other layout is made contiguous first).  -inf outside the support, on a bound and for
                          rows with a NaN or an inf; never NaN, never +inf.  A row's value does not depend on the layout, on
                          ``n`` or on its place in ``x``.
    ``logpdf(x)``         numpy in, numpy out, through the same function.
    ``rvs(size)``         base draw from torch's global CPU generator (as ``Flow.sample``), ``flow.inverse``, ``scaler.inverse``.
    ``bounds``, ``dim``   the scaler's.

    The density is float32 flow arithmetic: ``log p`` carries the flow kernels' relative error (1e-5 affine, 1e-4 spline).
    The prior owns copies of both parts: later ``set_params`` / ``fit`` calls on the source flow or scaler do not move it.  The
    scaler's boundary flags (periodic / reflective) are ignored: the forward map does not use them.  There is no
    ``device_descriptor``: the step calls the function.

    ``from_sampler(s)`` takes a finished run's own flow and scaler; ``from_samples(x, weights, bounds)`` and
    ``from_sampler(s, columns=...)`` fit a new flow on weighted samples -- the run's density on a subset of its parameters,
    for ``JointPrior``."""

    MAX_DIM = 157            # the widest MCMC step (pmc_flow_prior_pre refuses wider calls)
    RVS_ROUNDS = 8           # redraws of rows that land outside the support before rvs gives up
    _WORKSPACES = 8          # row counts whose workspaces are kept

    def __init__(self, flow, scaler):
        from .flow import Flow
        from .scaler import Reparameterize
        if not isinstance(flow, Flow):
            raise ValueError(f"FlowPrior: flow must be a pocomc_amd.Flow, got {type(flow).__name__}")
        if not isinstance(scaler, Reparameterize):
            raise ValueError(f"FlowPrior: scaler must be a pocomc_amd.Reparameterize, got {type(scaler).__name__}")
        if not scaler.diagonal:
            raise ValueError("FlowPrior: the scaler must be diagonal (diagonal=False scalers transform arrays only)")
        if scaler.mu is None or scaler.sigma is None:
            raise ValueError("FlowPrior: the scaler is not fitted (mu is None)")
        if flow.n_dim != scaler.ndim:
            raise ValueError(f"FlowPrior: the flow has {flow.n_dim} dimensions, the scaler {scaler.ndim}")
        if flow.n_dim > self.MAX_DIM:
            raise ValueError(f"FlowPrior: n_dim = {flow.n_dim} is too large (n_dim <= {self.MAX_DIM})")
        self._restore(flow.__getstate__(), self._scaler_state(scaler), flow.device)

    @staticmethod
    def _finished(sampler):
        walkers = getattr(sampler, "walkers", None)
        beta = None if walkers is None else walkers.get("beta")
        if beta is None or 1.0 - float(beta) >= 1e-4:
            raise ValueError("FlowPrior.from_sampler: the sampler has not run to beta = 1"
                             + ("" if beta is None else f" (beta = {float(beta):.6g})"))

    @classmethod
    def from_sampler(cls, sampler, columns=None, flow="nsf6", train_config=None):
        """The prior a finished ``Sampler`` run leaves.  ``columns=None``: ``sampler.flow`` and ``sampler.scaler`` themselves
        (``flow`` and ``train_config`` are not used); ``ValueError`` unless the sampler is preconditioned, has run to beta = 1
        and has trained its flow.  ``columns``: the run's density on those of its parameters, in that order -- a flow cannot
        be marginalised, so a new one is fitted on those columns of ``sampler.posterior()`` with its weights, on those rows of
        the sampler's bounds (``from_samples``; ``ValueError`` unless the sampler has run to beta = 1)."""
        if columns is None:
            if not getattr(sampler, "preconditioned", False):
                raise ValueError("FlowPrior.from_sampler: the sampler is not preconditioned (precondition=False): it trains "
                                 "no flow")
            cls._finished(sampler)
            if getattr(sampler, "flow_untrained", True):
                raise ValueError("FlowPrior.from_sampler: the sampler's flow has not been trained")
            return cls(sampler.flow, sampler.scaler)
        cls._finished(sampler)
        scaler = sampler.scaler
        k = len(columns) if hasattr(columns, "__len__") else 1
        cols, _ = JointPrior.layout(columns, k, scaler.ndim - k)         # (checks them: distinct integers in [0, ndim))
        samples, weights = sampler.posterior()[:2]
        bounds = np.stack([scaler.low, scaler.high], axis=1)[cols]
        return cls.from_samples(np.asarray(samples)[:, cols], weights, bounds=bounds, flow=flow, transform=scaler.transform,
                                train_config=train_config)

    TRAIN_KEYS = ("validation_split", "epochs", "batch_size", "patience", "learning_rate", "annealing", "gaussian_scale",
                  "laplace_scale", "noise", "shuffle", "clip_grad_norm", "verbose")

    @classmethod
    def from_samples(cls, x, weights=None, bounds=None, flow="nsf6", transform="probit", train_config=None):
        """A flow prior fitted on weighted samples: ``x`` ``(n, D)`` rows strictly inside ``bounds`` (``(D, 2)``, +-inf or NaN:
        unbounded on that side; None: unbounded), ``weights`` ``(n,)`` (None: uniform; normalised here).  A diagonal
        ``Reparameterize`` on ``bounds`` whose ``mu`` / ``sigma`` are the weighted mean and the weighted standard deviation
        (ddof 0) of the unscaled forward transform of ``x``; then ``Flow(D, flow)`` fitted on ``u = scaler.forward(x)`` with
        those weights, under the Sampler's ``train_config`` defaults (``validation_split=0.5, epochs=5000,
        batch_size=min(n // 2, 512), patience=D, learning_rate=1e-3, annealing=False, clip_grad_norm=1.0, shuffle=True``),
        which ``train_config`` overrides.  The fit shuffles with torch's global CPU generator, as every ``Flow.fit``."""
        import torch
        from .flow import Flow
        from .scaler import Reparameterize
        try:
            x = np.array(x, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("FlowPrior.from_samples: x must be an (n, D) array of floats") from None
        if x.ndim != 2 or x.shape[0] < 2:
            raise ValueError(f"FlowPrior.from_samples: x must have shape (n, D) with n >= 2, got {x.shape}")
        n, D = x.shape
        if D < 2:
            raise ValueError(f"FlowPrior.from_samples: a flow needs at least 2 dimensions, got {D}")
        if D > cls.MAX_DIM:
            raise ValueError(f"FlowPrior.from_samples: n_dim = {D} is too large (n_dim <= {cls.MAX_DIM})")
        if bounds is None:
            b = np.stack([np.full(D, -np.inf), np.full(D, np.inf)], axis=1)
        else:
            b = np.array(bounds, dtype=np.float64)
            if b.shape != (D, 2):
                raise ValueError(f"FlowPrior.from_samples: bounds must have shape ({D}, 2), got {b.shape}")
            b = np.stack([np.where(np.isnan(b[:, 0]), -np.inf, b[:, 0]), np.where(np.isnan(b[:, 1]), np.inf, b[:, 1])], axis=1)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(x) & (x > b[:, 0]) & (x < b[:, 1])
        if not ok.all():
            r, j = np.argwhere(~ok)[0]
            raise ValueError(f"FlowPrior.from_samples: row {r} is outside the bounds (column {j}: {x[r, j]} is not strictly "
                             f"inside ({b[j, 0]}, {b[j, 1]}))")
        if weights is None:
            w = np.full(n, 1.0 / n)
        else:
            w = np.array(weights, dtype=np.float64)
            if w.shape != (n,):
                raise ValueError(f"FlowPrior.from_samples: weights must have shape ({n},), got {w.shape}")
            if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
                raise ValueError("FlowPrior.from_samples: weights must be finite, not negative and not all zero")
            w = w / w.sum()
        cfg = dict(validation_split=0.5, epochs=5000, batch_size=min(n // 2, 512), patience=D, learning_rate=1e-3,
                   annealing=False, clip_grad_norm=1.0, shuffle=True)
        for k, v in (train_config or {}).items():
            if k not in cls.TRAIN_KEYS:
                raise ValueError(f"FlowPrior.from_samples: train_config has no key {k!r} (keys: {', '.join(cls.TRAIN_KEYS)})")
            cfg[k] = v
        cfg["batch_size"] = int(min(n // 2, cfg["batch_size"]))
        scaler = Reparameterize(D, bounds=b, transform=transform)
        t = scaler._forward_device(x, scale=False)
        mu = np.sum(w[:, None] * t, axis=0)
        sigma = np.sqrt(np.sum(w[:, None] * (t - mu) ** 2, axis=0))
        if not (np.isfinite(mu).all() and np.isfinite(sigma).all() and (sigma > 0).all()):
            raise ValueError("FlowPrior.from_samples: a column's transformed samples have no finite, positive spread")
        scaler.mu, scaler.sigma = mu, sigma
        u = scaler.forward(x, check_input=False)
        f = Flow(D, flow)
        f.fit(torch.from_numpy(u.astype(np.float32)), weights=torch.from_numpy(w.astype(np.float32)), **cfg)
        return cls(f, scaler)

    # ----------------------------------------------------------------- state
    @staticmethod
    def _scaler_state(s):
        return dict(low=np.array(s.low, dtype=np.float64), high=np.array(s.high, dtype=np.float64), transform=s.transform,
                    scale=bool(s.scale), mu=np.array(s.mu, dtype=np.float64), sigma=np.array(s.sigma, dtype=np.float64))

    def _restore(self, flow_state, scaler_state, device=None):
        import copy
        import torch
        from .flow import Flow
        from .scaler import Reparameterize
        st = copy.deepcopy(scaler_state)
        D = len(st["low"])
        if device is None:
            from . import _lib
            device = _lib.require_gpu()
        with torch.cuda.device(device):
            self.flow = Flow.__new__(Flow)
            self.flow.__setstate__(copy.deepcopy(flow_state))
        self.scaler = Reparameterize(D, bounds=np.stack([st["low"], st["high"]], axis=1), transform=st["transform"],
                                     scale=st["scale"], diagonal=True, device=self.flow.device)
        self.scaler.mu, self.scaler.sigma = st["mu"], st["sigma"]
        self._sdesc = self.scaler.device_descriptor()       # (the scaler keeps the tensors it points to)
        self._ws = {}

    def __getstate__(self):
        return {"flow": self.flow.__getstate__(), "scaler": self._scaler_state(self.scaler)}

    def __setstate__(self, st):
        self._restore(st["flow"], st["scaler"])

    # ----------------------------------------------------------------- density
    def _workspace(self, n):
        import torch
        ws = self._ws.get(n)
        if ws is None:
            dev = self.flow.device
            ws = (torch.empty(n, self.dim, dtype=torch.float32, device=dev),      # u32
                  torch.empty(n, self.dim, dtype=torch.float32, device=dev),      # z (the flow writes it; not used)
                  torch.empty(n, dtype=torch.float32, device=dev),                # the flow's log_prob
                  torch.empty(n, dtype=torch.float64, device=dev),                # the scaler's log-determinant
                  torch.empty(n, dtype=torch.int32, device=dev))                  # inside the support
            while len(self._ws) >= self._WORKSPACES:
                self._ws.pop(next(iter(self._ws)))
            self._ws[n] = ws
        return ws

    def logpdf_device(self, x):
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        D = self.dim
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"FlowPrior.logpdf_device: expected an (n, {D}) float64 tensor, got {what}")
        _on_device(x, self.flow.device, "FlowPrior.logpdf_device")
        n = x.shape[0]
        out = torch.empty(n, dtype=torch.float64, device=self.flow.device)
        if n == 0:
            return out
        # the two layouts the kernel reads with coalesced loads; everything else is copied once
        if x.is_contiguous():
            strides = (D, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (D, 1)
        u32, z, lp32, ldj, inside = self._workspace(n)
        lib = self.flow.lib
        with torch.cuda.device(self.flow.device):
            _lib.check(lib.pmc_flow_prior_pre(C.byref(self._sdesc), C.c_void_p(x.data_ptr()), strides[0], strides[1], n,
                                              _lib.ptr(u32), _lib.ptr(ldj), _lib.ptr(inside), _lib.stream_handle()),
                       "pmc_flow_prior_pre")
            self.flow._forward_call(u32, z, None, lp32, n)
            _lib.check(lib.pmc_flow_prior_post(_lib.ptr(lp32), _lib.ptr(ldj), _lib.ptr(inside), _lib.ptr(out), n,
                                               _lib.stream_handle()), "pmc_flow_prior_post")
        return out

    def logpdf(self, x):
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"FlowPrior.logpdf: expected shape (n, {self.dim}), got {x.shape}")
        return self.logpdf_device(torch.from_numpy(x).to(self.flow.device)).cpu().numpy()

    def step_stage(self, n, device=None):
        """``pmc_prior_stage_t`` for a step engine of ``n`` rows on ``device`` (None: the flow's): the MCMC step of a HOST
        likelihood then evaluates this prior itself, on its own stream, from its device copy of x' (kernel option
        ``step_prior``, ``StepEngine.set_step_prior``) -- the three launches of ``logpdf_device``, the same bits.  One
        workspace set per call; the descriptor keeps it and this prior alive."""
        return _step_stage(self, self, n, device)

    # ----------------------------------------------------------------- draws
    def _inside(self, x):
        lo = np.where(np.isfinite(self.scaler.low), self.scaler.low, -np.inf)
        hi = np.where(np.isfinite(self.scaler.high), self.scaler.high, np.inf)
        return np.all(np.isfinite(x) & (x > lo) & (x < hi), axis=1)

    def rvs(self, size=1):
        import torch
        size = int(size)
        x = np.empty((size, self.dim), dtype=np.float64)
        todo = np.arange(size)
        for _ in range(1 + self.RVS_ROUNDS):
            if len(todo) == 0:
                return x
            z = torch.randn(len(todo), self.dim, dtype=torch.float32)
            u, _ = self.flow.inverse(z)
            xi, _ = self.scaler.inverse(u.numpy().astype(np.float64))
            x[todo] = xi
            todo = todo[~self._inside(xi)]
        if len(todo):
            raise RuntimeError(f"FlowPrior.rvs: {len(todo)} of {size} rows are still outside the support after "
                               f"{self.RVS_ROUNDS} redraws")
        return x

    @property
    def bounds(self):
        return np.stack([self.scaler.low, self.scaler.high], axis=1)

    @property
    def dim(self):
        return self.scaler.ndim


class GaussianPrior:
    """A correlated normal prior, ``x ~ N(mean, cov)`` in ``1 <= k <= 157`` dimensions: what an earlier result leaves where it
    is a mean and a covariance matrix -- a published constraint, a Fisher forecast, a Laplace approximation -- and no flow.

    ``mean``  ``(k,)`` finite floats; ``cov``  ``(k, k)`` finite, exactly symmetric (``np.array_equal(cov, cov.T)``: the user
    symmetrises) and positive definite (``np.linalg.cholesky`` succeeds).  ``ValueError`` names what is wrong.  The constructor
    is numpy alone: ``L = cholesky(cov)``, ``Linv = solve_triangular(L, I, lower=True)`` packed by rows (row i: i + 1 entries)
    and ``logc = sum(log(diag(L))) + 0.5 k log(2 pi)``, all float64 (``device_block()``); the device's copies are made at the
    first device call and dropped on pickling.

    ``logpdf_device(x)``  the ``DevicePrior`` contract: an ``(n, k)`` float64 tensor on the device in, an ``(n,)`` float64 tensor
                          out, on the current stream, in ONE launch (``pmc_gauss_blocks_logpdf``, ``csrc/gauss_prior.hip``) and
                          no host synchronisation; no copy of ``x`` when it is C-contiguous or the MCMC step's column-major
                          view (any other layout is made contiguous first).  The value is
                          ``-0.5 |Linv (x - mean)|^2 - logc`` with every product and every sum rounded, in the order
                          ``include/pocomc_amd.h`` fixes: the bits of ``tests/gauss_prior_model.py``, whatever the layout,
                          ``n`` or the row's place in ``x``.  -inf for a row with a NaN or an inf and for a row whose arithmetic
                          gives NaN; never NaN, never +inf.
    ``logpdf(x)``         numpy in, numpy out, through the same function.
    ``rvs(size)``         ``mean + z @ L.T``, ``z`` standard normal from numpy's global generator (``Sampler(random_state=...)``
                          reaches it).
    ``bounds``, ``dim``   ``(k, 2)`` of -inf / +inf, and k.

    There is no ``device_descriptor`` and no ``step_stage``: the step calls the function (``Sampler(device_likelihood=True,
    device_prior=True)``).  ``JointPrior`` takes it as a block next to flow priors and a table.  Out of scope: singular
    covariances.  A box around it: ``TruncatedGaussianPrior``."""

    MAX_DIM = FlowPrior.MAX_DIM

    def __init__(self, mean, cov):
        self.__setstate__(self._constants(mean, cov))

    @classmethod
    def _constants(cls, mean, cov):
        """The checks and the host-side constants: the state of a ``GaussianPrior(mean, cov)``."""
        try:
            m = np.array(mean, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("GaussianPrior: mean must be a (k,) array of floats") from None
        try:
            c = np.array(cov, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("GaussianPrior: cov must be a (k, k) array of floats") from None
        if m.ndim != 1:
            raise ValueError(f"GaussianPrior: mean must have shape (k,), got {m.shape}")
        k = len(m)
        if not 1 <= k <= cls.MAX_DIM:
            raise ValueError(f"GaussianPrior: mean has {k} dimensions (1 <= k <= {cls.MAX_DIM})")
        if c.shape != (k, k):
            raise ValueError(f"GaussianPrior: cov must have shape ({k}, {k}), got {c.shape}")
        if not np.isfinite(m).all():
            raise ValueError(f"GaussianPrior: mean[{int(np.argmin(np.isfinite(m)))}] is not finite")
        if not np.isfinite(c).all():
            i, j = np.argwhere(~np.isfinite(c))[0]
            raise ValueError(f"GaussianPrior: cov[{i}, {j}] is not finite")
        if not np.array_equal(c, c.T):
            i, j = np.argwhere(c != c.T)[0]
            raise ValueError(f"GaussianPrior: cov is not symmetric (cov[{i}, {j}] = {c[i, j]!r}, cov[{j}, {i}] = {c[j, i]!r}); "
                             "symmetrise it, 0.5 * (cov + cov.T)")
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError("GaussianPrior: cov is not positive definite (np.linalg.cholesky fails)") from None
        from scipy.linalg import solve_triangular
        Linv = solve_triangular(L, np.eye(k), lower=True)
        logc = float(np.sum(np.log(np.diag(L))) + 0.5 * k * np.log(2 * np.pi))
        if not (np.isfinite(Linv).all() and np.isfinite(logc)):
            raise ValueError("GaussianPrior: cov is too close to singular: the inverse of its Cholesky factor is not finite")
        return dict(mean=m, cov=c, L=L, linv_packed=np.ascontiguousarray(Linv[np.tril_indices(k)]), logc=logc)

    # ----------------------------------------------------------------- state
    def __getstate__(self):
        return dict(mean=self.mean.copy(), cov=self.cov.copy(), L=self.L.copy(), linv_packed=self.linv_packed.copy(),
                    logc=self.logc)

    def __setstate__(self, st):
        self.mean = np.array(st["mean"], dtype=np.float64)
        self.cov = np.array(st["cov"], dtype=np.float64)
        self.L = np.array(st["L"], dtype=np.float64)
        self.linv_packed = np.array(st["linv_packed"], dtype=np.float64)
        self.logc = float(st["logc"])
        self._dev = None

    def device_block(self):
        """The device's constants as numpy arrays: ``mean`` (k,), ``linv_packed`` (k (k + 1) / 2,): row i of the inverse of
        the Cholesky factor at ``i (i + 1) / 2``, and ``logc`` (a 0-d array).  No torch, no GPU."""
        return dict(mean=self.mean.copy(), linv_packed=self.linv_packed.copy(), logc=np.array(self.logc, dtype=np.float64))

    def _device(self, device):
        """The device's copies and the one-block descriptor, made once, on ``device``."""
        if self._dev is None:
            import torch
            from . import _lib
            k = self.dim
            dev = torch.device(device)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d = dict(device=dev, mean=up(self.mean), linv=up(self.linv_packed), cols=up(np.arange(k, dtype=np.int32)))
            g = _lib.pmc_gauss_blocks_t(n_blocks=1, D=k, rest=None, rest_cols=None)
            g.dim[0], g.logc[0] = k, self._logc_device
            g.cols[0], g.mean[0], g.linv[0] = d["cols"].data_ptr(), d["mean"].data_ptr(), d["linv"].data_ptr()
            d["desc"] = g                                   # (it points into the tensors next to it)
            self._dev = d
        return self._dev

    # ----------------------------------------------------------------- density
    def logpdf_device(self, x):
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        k, who = self.dim, type(self).__name__
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != k:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"{who}.logpdf_device: expected an (n, {k}) float64 tensor, got {what}")
        if not x.is_cuda:
            raise ValueError(f"{who}.logpdf_device: expected a tensor on the GPU, got one on {x.device}")
        d = self._device(x.device)
        _on_device(x, d["device"], f"{who}.logpdf_device")
        n = x.shape[0]
        out = torch.empty(n, dtype=torch.float64, device=x.device)
        if n == 0:
            return out
        # the two layouts the kernel reads with coalesced loads; everything else is copied once
        if x.is_contiguous():
            strides = (k, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (k, 1)
        with torch.cuda.device(x.device):
            self._launch(d, C.c_void_p(x.data_ptr()), strides, n, _lib.ptr(out))
        return out

    _logc_device = property(lambda self: self.logc)      # the constant the device subtracts

    def _launch(self, d, x_ptr, strides, n, out_ptr):
        import ctypes as C
        from . import _lib
        _lib.check(_lib.load().pmc_gauss_blocks_logpdf(C.byref(d["desc"]), x_ptr, strides[0], strides[1], n, None, out_ptr,
                                                       _lib.stream_handle()), "pmc_gauss_blocks_logpdf")

    def logpdf(self, x):
        import torch
        from . import _lib
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"{type(self).__name__}.logpdf: expected shape (n, {self.dim}), got {x.shape}")
        dev = self._dev["device"] if self._dev is not None else _lib.require_gpu()
        return self.logpdf_device(torch.from_numpy(x).to(dev)).cpu().numpy()

    # ----------------------------------------------------------------- draws
    def rvs(self, size=1):
        size = int(size)
        z = np.random.mtrand._rand.standard_normal((size, self.dim))     # (numpy's global generator, named: JointPrior.rvs)
        return self.mean + z @ self.L.T

    @property
    def bounds(self):
        return np.stack([np.full(self.dim, -np.inf), np.full(self.dim, np.inf)], axis=1)

    @property
    def dim(self):
        return len(self.mean)


MAX_CORRELATED_BOUNDS = 12        # bounded columns with a non-diagonal covariance whose box mass the constructor integrates
MAX_LOG_MASS_SPREAD = 1e-3        # |log mass (seed 0) - log mass (seed 1)| the constructor accepts: 30 times below the +-0.03
                                  # of a run's log-evidence
MASS_SEEDS = (20240229, 20240301)  # the two integrations' generators (never numpy's global one)
MASS_POINTS = 100_000             # lattice points per bounded column and seed, in MASS_SHIFTS randomly shifted copies
MASS_SHIFTS = 8
MASS_ABSEPS, MASS_RELEPS = 1e-9, 1e-7     # scipy's tolerances where scipy integrates (two bounded columns: its exact form)
MAX_RVS_DRAWS = 1e8               # rvs refuses when size / mass, the draws it expects to make, exceeds this


def _genz_box_mass(mean, cov, lo, hi, seed, points=None, shifts=None, chunk=1 << 16):
    """The mass of the box ``[lo, hi]`` under ``N(mean, cov)`` by Genz's separation of variables (A. Genz, "Numerical
    computation of multivariate normal probabilities", J. Comp. Graph. Stat. 1, 1992): the integral becomes one over the unit
    cube of d - 1 dimensions, taken with ``shifts`` randomly shifted Richtmyer lattices (generators sqrt(prime), the tent
    transform) of ``points / shifts`` points each; the narrowest columns are integrated first.  The shifts come from a
    generator of their own, seeded with ``seed``: the same arguments give the same bits, and numpy's global generator is not
    touched.  An interval beyond the mean is measured in the tail it lies in, so that its mass is a difference of small
    numbers and not of numbers next to 1.  numpy and scipy.special only."""
    from scipy.special import ndtr, ndtri
    d = len(mean)
    points = MASS_POINTS * d if points is None else int(points)
    shifts = MASS_SHIFTS if shifts is None else int(shifts)
    sd = np.sqrt(np.diag(cov))
    a, b = lo - mean, hi - mean
    order = np.argsort(ndtr(b / sd) - ndtr(a / sd), kind="stable")
    a, b = a[order], b[order]
    L = np.linalg.cholesky(cov[np.ix_(order, order)])
    rng = np.random.Generator(np.random.PCG64(seed))
    primes = [p for p in range(2, 64) if all(p % q for q in range(2, p))][:d - 1]
    gen = np.sqrt(np.array(primes, dtype=np.float64))
    n = -(-points // shifts)

    def interval(ai, bi):
        """(measured in the upper tail, the lower end's probability, the width) of [ai, bi] under the standard normal."""
        flip = ai > 0
        lo_, hi_ = np.where(flip, -bi, ai), np.where(flip, -ai, bi)
        dd = ndtr(lo_)
        return flip, dd, ndtr(hi_) - dd

    total = 0.0
    for _ in range(shifts):
        shift = rng.random(d - 1)
        acc = 0.0
        for k0 in range(1, n + 1, chunk):
            k = np.arange(k0, min(k0 + chunk, n + 1), dtype=np.float64)[:, None]
            w = np.abs(2.0 * ((k * gen + shift) % 1.0) - 1.0)
            y = np.empty((len(k), d - 1))
            flip, dd, wd = interval(np.full(len(k), a[0] / L[0, 0]), np.full(len(k), b[0] / L[0, 0]))
            f = wd.copy()
            for i in range(1, d):
                t = ndtri(np.clip(dd + w[:, i - 1] * wd, 1e-300, 1.0 - 2.0 ** -53))
                y[:, i - 1] = np.where(flip, -t, t)
                s = y[:, :i] @ L[i, :i]
                flip, dd, wd = interval((a[i] - s) / L[i, i], (b[i] - s) / L[i, i])
                f = f * wd
            acc += float(f.sum())
        total += acc / n
    return total / shifts


def _box_log_mass(mean, cov, bounds):
    """``(log_mass, log_mass_spread)`` of the box ``bounds`` under ``N(mean, cov)``: see ``TruncatedGaussianPrior``."""
    hint = "; log_mass= takes a value computed elsewhere"
    S = np.flatnonzero(np.isfinite(bounds).any(axis=1))
    if len(S) == 0:
        return 0.0, 0.0
    m, c, lo, hi = mean[S], cov[np.ix_(S, S)], bounds[S, 0], bounds[S, 1]           # the marginal on S: exact
    if len(S) == 1 or not (c - np.diag(np.diag(c))).any():
        sd = np.sqrt(np.diag(c))
        log_mass, spread = float(sum(_log_gauss_mass((lo[j] - m[j]) / sd[j], (hi[j] - m[j]) / sd[j]) for j in range(len(S)))), 0.0
    else:
        if len(S) > MAX_CORRELATED_BOUNDS:
            raise ValueError(f"TruncatedGaussianPrior: {len(S)} correlated bounded columns: the constructor integrates the box's "
                             f"mass for at most MAX_CORRELATED_BOUNDS = {MAX_CORRELATED_BOUNDS}" + hint)
        if len(S) == 2:
            # scipy's routine takes two columns in closed form (no sampling: the same bits on every call)
            from scipy.stats import multivariate_normal
            masses = [float(multivariate_normal.cdf(hi, m, c, maxpts=1000000 * len(S), abseps=MASS_ABSEPS, releps=MASS_RELEPS,
                                                    lower_limit=lo))] * 2
        else:
            masses = [_genz_box_mass(m, c, lo, hi, seed) for seed in MASS_SEEDS]
        if not all(np.isfinite(v) and v > 0.0 for v in masses):
            raise ValueError(f"TruncatedGaussianPrior: the box's mass under the normal is not positive and finite ({masses[0]!r}, "
                             f"{masses[1]!r}): the box lies too far out in the tail for the integration" + hint)
        log_mass = float(np.log(min(0.5 * (masses[0] + masses[1]), 1.0)))
        spread = float(abs(np.log(masses[0]) - np.log(masses[1])))
        if spread > MAX_LOG_MASS_SPREAD:
            raise ValueError(f"TruncatedGaussianPrior: two integrations of the box's mass differ by {spread:.3g} in the log "
                             f"(more than {MAX_LOG_MASS_SPREAD:g})" + hint)
    if not (np.isfinite(log_mass) and log_mass <= 0.0):
        raise ValueError(f"TruncatedGaussianPrior: the box's mass under the normal is not positive and finite (log mass "
                         f"{log_mass!r})" + hint)
    return log_mass, spread


class TruncatedGaussianPrior(GaussianPrior):
    """A correlated normal on a box: ``x ~ N(mean, cov)`` restricted to ``lo_j <= x_j <= hi_j`` and normalised,

        ``log p(x) = -0.5 |Linv (x - mean)|^2 - logc - log_mass`` inside the closed box, ``-inf`` outside,

    -- a published Gaussian constraint on parameters with hard limits (an amplitude above zero, a fraction in [0, 1]).

    ``mean``, ``cov``  as for ``GaussianPrior`` (the same checks, the same texts, ``1 <= k <= 157``); ``mean`` need not lie in
                       the box.
    ``bounds``         ``(k, 2)`` floats, ``lo_j < hi_j``; -inf / +inf for a one-sided limit or an untouched column, no NaN.
                       The value on a bound is finite and the first float beyond it is -inf (scipy's ``truncnorm``).
    ``log_mass``       None: the constructor computes the log of the box's mass under the normal (numpy and scipy, no torch,
                       no GPU).  With S the columns that have a finite limit, the marginal ``N(mean[S], cov[S, S])`` carries
                       all of it: 0.0 for an empty S; the sum of scipy's ``truncnorm`` masses for one column or a diagonal
                       ``cov[S, S]``; scipy's closed form for two correlated columns; otherwise two integrations by Genz's
                       method with two fixed seeds (``MASS_SEEDS``, ``MASS_POINTS`` per column), ``log_mass`` the log of
                       their mean and ``log_mass_spread`` the difference of their logs.  The same arguments give the same
                       bits, and numpy's global generator is not touched.  ``ValueError`` -- each says that ``log_mass=``
                       takes a value computed elsewhere -- for a spread above 1e-3, for a mass that is not positive and
                       finite, and for more than ``MAX_CORRELATED_BOUNDS`` = 12 correlated bounded columns.
                       A float: finite and <= 0, taken as given; ``log_mass_spread`` is then None.

    ``logc_box = logc + log_mass`` (one float64 addition) is what the device subtracts; ``device_block()`` gives ``mean``,
    ``linv_packed``, ``logc`` (= ``logc_box``), ``lo`` and ``hi``.  ``logpdf_device`` and ``logpdf`` follow ``GaussianPrior``'s
    contract -- one launch, no host synchronisation, no copy for the two coalesced layouts, never NaN, never +inf -- through
    ``pmc_gauss_box_logpdf``: the same kernel with the box test compiled in; a row inside has ``pmc_gauss_blocks_logpdf``'s bits
    for ``logc_box``, and with all-infinite bounds ``GaussianPrior``'s.  ``rvs(size)`` is rejection from ``mean + z @ L.T``
    (numpy's global generator, blocks of ``ceil(1.2 missing / mass) + 16`` rows, kept in draw order); ``RuntimeError`` before
    anything is drawn when ``size / mass > 1e8``.  ``bounds`` is the box, ``dim`` k.  The state is ``GaussianPrior``'s plus
    ``bounds``, ``log_mass`` and ``log_mass_spread``.  No ``device_descriptor``, no ``step_stage``; ``JointPrior`` takes it as a
    Gaussian block.  Out of scope: boxes that are not axis-aligned, and singular covariances."""

    def __init__(self, mean, cov, bounds, log_mass=None):
        st = self._constants(mean, cov)
        k = len(st["mean"])
        try:
            b = np.array(bounds, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"TruncatedGaussianPrior: bounds must be a ({k}, 2) array of floats") from None
        if b.shape != (k, 2):
            raise ValueError(f"TruncatedGaussianPrior: bounds must have shape ({k}, 2), got {b.shape}")
        if np.isnan(b).any():
            raise ValueError(f"TruncatedGaussianPrior: bounds of column {int(np.argwhere(np.isnan(b))[0][0])} hold a NaN")
        if not (b[:, 0] < b[:, 1]).all():
            j = int(np.argmin(b[:, 0] < b[:, 1]))
            raise ValueError(f"TruncatedGaussianPrior: column {j}: lo = {float(b[j, 0])!r} is not below hi = {float(b[j, 1])!r}")
        if log_mass is None:
            log_mass, spread = _box_log_mass(st["mean"], st["cov"], b)
        else:
            try:
                log_mass = float(log_mass)
            except (TypeError, ValueError):
                raise ValueError(f"TruncatedGaussianPrior: log_mass must be a finite float <= 0, got {log_mass!r}") from None
            if not (np.isfinite(log_mass) and log_mass <= 0.0):
                raise ValueError(f"TruncatedGaussianPrior: log_mass must be a finite float <= 0, got {log_mass!r}")
            spread = None
        self.__setstate__(dict(st, bounds=b, log_mass=log_mass, log_mass_spread=spread))

    # ----------------------------------------------------------------- state
    def __getstate__(self):
        return dict(GaussianPrior.__getstate__(self), bounds=self._bounds.copy(), log_mass=self.log_mass,
                    log_mass_spread=self.log_mass_spread)

    def __setstate__(self, st):
        GaussianPrior.__setstate__(self, st)
        self._bounds = np.array(st["bounds"], dtype=np.float64)
        self.log_mass = float(st["log_mass"])
        self.log_mass_spread = None if st["log_mass_spread"] is None else float(st["log_mass_spread"])
        self.logc_box = self.logc + self.log_mass

    _logc_device = property(lambda self: self.logc_box)

    def device_block(self):
        """``GaussianPrior.device_block`` with ``logc`` = ``logc_box`` and the box: ``lo``, ``hi`` (k,)."""
        return dict(mean=self.mean.copy(), linv_packed=self.linv_packed.copy(), logc=np.array(self.logc_box, dtype=np.float64),
                    lo=self._bounds[:, 0].copy(), hi=self._bounds[:, 1].copy())

    def _device(self, device):
        if self._dev is None:
            import torch
            from . import _lib
            d = GaussianPrior._device(self, device)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d["device"])
            d["lo"], d["hi"] = up(self._bounds[:, 0]), up(self._bounds[:, 1])
            box = _lib.pmc_gauss_box_t()
            box.lo[0], box.hi[0] = d["lo"].data_ptr(), d["hi"].data_ptr()
            d["box"] = box
        return self._dev

    def _launch(self, d, x_ptr, strides, n, out_ptr):
        import ctypes as C
        from . import _lib
        _lib.check(_lib.load().pmc_gauss_box_logpdf(C.byref(d["desc"]), C.byref(d["box"]), x_ptr, strides[0], strides[1], n,
                                                    None, out_ptr, _lib.stream_handle()), "pmc_gauss_box_logpdf")

    # ----------------------------------------------------------------- draws
    def rvs(self, size=1):
        size = int(size)
        mass = float(np.exp(self.log_mass))
        if size / mass > MAX_RVS_DRAWS:
            raise RuntimeError(f"TruncatedGaussianPrior.rvs: {size} rows at a box mass of {mass:.3g} need about {size / mass:.3g} "
                               f"draws of the untruncated normal (more than {MAX_RVS_DRAWS:g})")
        lo, hi = self._bounds[:, 0], self._bounds[:, 1]
        out, missing = [], size
        while missing > 0:
            m = int(np.ceil(1.2 * missing / mass)) + 16
            x = GaussianPrior.rvs(self, m)
            x = x[((x >= lo) & (x <= hi)).all(axis=1)][:missing]          # (in draw order)
            out.append(x)
            missing -= len(x)
        return np.concatenate(out) if out else np.empty((0, self.dim))

    @property
    def bounds(self):
        return self._bounds.copy()


class GaussianMixturePrior:
    """A mixture of correlated normals, ``p(x) = sum_c w_c N(x; mean_c, cov_c)``, with ``1 <= C <= 32`` components
    (``MAX_COMPONENTS``) on the same ``1 <= k <= 64`` columns (``MAX_DIM``): the earlier result that is not Gaussian and not
    worth a flow -- a bimodal or banana-shaped posterior on a few shared parameters, a published "sum of N Gaussians", two
    competing predictions.  Exactly normalised, exactly sampled, float64 throughout.  The two limits (and ``D <= 157`` in a
    ``JointPrior``) are what the kernel's LDS plan holds (``csrc/gauss_mix_prior.hip``); wider mixtures are out of scope.

    ``weights``  ``(C,)`` finite and strictly positive; the constructor divides by their sum and keeps
                 ``logw = log(weights / weights.sum())`` (exactly 0.0 for C = 1).
    ``means``    ``(C, k)``;  ``covs``  ``(C, k, k)``.  Every ``(means[c], covs[c])`` passes ``GaussianPrior``'s checks (finite,
                 exactly symmetric, positive definite); each ``ValueError`` is prefixed ``GaussianMixturePrior: component c: ``.
    The constructor is numpy and scipy alone; ``device_block()`` gives ``logw`` (C,), ``mean`` (C, k), ``linv_packed``
    (C, k (k + 1) / 2) in ``GaussianPrior``'s packing and ``logc`` (C,).  The state carries the inputs and these constants; the
    device's copies are made at the first device call and dropped on pickling.

    ``logpdf_device(x)``  the ``DevicePrior`` contract, as ``GaussianPrior.logpdf_device``: an ``(n, k)`` float64 tensor on the
                          device in, an ``(n,)`` float64 tensor out, on the current stream, in ONE launch
                          (``pmc_gauss_mix_logpdf``) and no host synchronisation; no copy of ``x`` when it is C-contiguous or
                          the MCMC step's column-major view (any other layout is made contiguous once); ``n == 0`` gives an
                          empty tensor.  The value is ``m + log(sum_c exp(t_c - m))``, ``t_c = g_c + logw_c`` with
                          ``GaussianPrior``'s ``g_c`` bit for bit and ``m = max_c t_c``, in the order ``include/pocomc_amd.h``
                          fixes (``tests/gauss_mix_model.py``).  -inf for a row with a NaN or an inf and for a row every
                          component gives -inf; never NaN, never +inf.  With one component: ``GaussianPrior``'s bits.
    ``logpdf(x)``         numpy in, numpy out, through the same function.
    ``rvs(size)``         two draws from numpy's GLOBAL generator (``Sampler(random_state=...)`` reaches it), in this order:
                          first the ``size`` component indices by the weights (``choice``), then ONE standard-normal
                          ``(size, k)`` block; row r is ``mean_c + z_r @ L_c.T`` for its component c.
    ``bounds``, ``dim``   ``(k, 2)`` of -inf / +inf, and k.

    ``from_samples(x, weights, n_components)`` fits the mixture to weighted samples by EM, ``from_sampler(s, columns=...)`` to
    a finished run's posterior.  There is no ``device_descriptor`` and no ``step_stage``: the step calls the function
    (``Sampler(device_likelihood=True, device_prior=True)``).  ``JointPrior`` takes it as a block.  Out of scope: more than 32
    components or 64 columns, a box around the mixture (``TruncatedGaussianPrior`` has one component), choosing C."""

    MAX_COMPONENTS = 32      # PMC_GAUSS_MIX_MAX_COMPONENTS
    MAX_DIM = 64             # PMC_GAUSS_MIX_MAX_DIM

    def __init__(self, weights, means, covs):
        self.__setstate__(self._constants(weights, means, covs))

    @classmethod
    def _constants(cls, weights, means, covs):
        """The checks and the host-side constants: the state of a ``GaussianMixturePrior(weights, means, covs)``."""
        who = "GaussianMixturePrior"
        arrays = []
        for name, a, what in (("weights", weights, "(C,)"), ("means", means, "(C, k)"), ("covs", covs, "(C, k, k)")):
            try:
                arrays.append(np.array(a, dtype=np.float64))
            except (TypeError, ValueError):
                raise ValueError(f"{who}: {name} must be a {what} array of floats") from None
        w, m, c = arrays
        if w.ndim != 1 or len(w) < 1:
            raise ValueError(f"{who}: weights must have shape (C,) with C >= 1, got {w.shape}")
        C = len(w)
        if C > cls.MAX_COMPONENTS:
            raise ValueError(f"{who}: {C} components (1 <= C <= {cls.MAX_COMPONENTS})")
        if m.ndim != 2 or m.shape[0] != C or m.shape[1] < 1:
            raise ValueError(f"{who}: means must have shape ({C}, k) with k >= 1, got {m.shape}")
        k = m.shape[1]
        if k > cls.MAX_DIM:
            raise ValueError(f"{who}: means have {k} dimensions (1 <= k <= {cls.MAX_DIM})")
        if c.shape != (C, k, k):
            raise ValueError(f"{who}: covs must have shape ({C}, {k}, {k}), got {c.shape}")
        if not (np.isfinite(w) & (w > 0)).all():
            j = int(np.argmin(np.isfinite(w) & (w > 0)))
            raise ValueError(f"{who}: weights[{j}] = {float(w[j])!r} is not finite and strictly positive")
        parts = []
        for j in range(C):
            try:
                parts.append(GaussianPrior._constants(m[j], c[j]))
            except ValueError as e:
                text = str(e)
                text = text[len("GaussianPrior: "):] if text.startswith("GaussianPrior: ") else text
                raise ValueError(f"{who}: component {j}: {text}") from None
        with np.errstate(all="ignore"):
            logw = np.log(w / w.sum())
        if not np.isfinite(logw).all():
            raise ValueError(f"{who}: weights[{int(np.argmin(np.isfinite(logw)))}] vanishes next to the weights' sum")
        return dict(weights=w, means=m, covs=c, logw=logw, L=np.stack([p["L"] for p in parts]),
                    linv_packed=np.stack([p["linv_packed"] for p in parts]), logc=np.array([p["logc"] for p in parts]),
                    fit_info=None)

    # ----------------------------------------------------------------- fits
    @classmethod
    def from_samples(cls, x, weights=None, n_components=2, seed=0, max_iter=500, tol=1e-8, cov_floor=1e-6):
        """The mixture fitted to weighted samples by EM, numpy and scipy alone.  ``x`` ``(n, k)`` finite rows, ``weights``
        ``(n,)`` finite, not negative, not all zero (None: uniform; normalised here), ``n_components`` = C.

        Seeding is k-means++ on the weighted rows (the first centre drawn by the weights, every next one by weight times
        squared distance to the nearest centre) from ``np.random.Generator(np.random.PCG64(seed))``: numpy's global generator
        is never touched and the same arguments give the same bits.  Start: ``w_c = 1 / C``, every ``cov_c`` the weighted
        sample covariance ``S0``.  Every M-step adds ``cov_floor * trace(S0) / k * I`` to every covariance and symmetrises it,
        ``0.5 (S + S.T)``.  The fit stops when the weighted mean log-density improves by less than ``tol``, or after
        ``max_iter`` E-steps.  ``ValueError`` when a component's responsibility mass falls below ``k + 1`` rows of the Kish
        effective sample size ``1 / sum(w^2)`` (a collapsed component: use fewer components), and for a covariance that is
        not positive definite.  ``prior.fit_info``: ``iterations`` (E-steps), ``converged`` and ``loglik``, the weighted mean
        log-density at every E-step (the last one is the returned mixture's).  Out of scope: choosing C, diagonal or tied
        covariances, bounded parameters."""
        from scipy.linalg import solve_triangular
        from scipy.special import logsumexp
        who = "GaussianMixturePrior.from_samples"
        try:
            x = np.array(x, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: x must be an (n, k) array of floats") from None
        if x.ndim != 2 or x.shape[0] < 2 or x.shape[1] < 1:
            raise ValueError(f"{who}: x must have shape (n, k) with n >= 2 and k >= 1, got {x.shape}")
        n, k = x.shape
        if k > cls.MAX_DIM:
            raise ValueError(f"{who}: x has {k} columns (1 <= k <= {cls.MAX_DIM})")
        if not np.isfinite(x).all():
            r, j = np.argwhere(~np.isfinite(x))[0]
            raise ValueError(f"{who}: x[{r}, {j}] is not finite")
        if weights is None:
            w = np.full(n, 1.0 / n)
        else:
            w = np.array(weights, dtype=np.float64)
            if w.shape != (n,):
                raise ValueError(f"{who}: weights must have shape ({n},), got {w.shape}")
            if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
                raise ValueError(f"{who}: weights must be finite, not negative and not all zero")
            w = w / w.sum()
        C = int(n_components)
        if C != n_components or not 1 <= C <= cls.MAX_COMPONENTS:
            raise ValueError(f"{who}: n_components = {n_components!r} (1 <= C <= {cls.MAX_COMPONENTS})")
        max_iter = int(max_iter)
        if max_iter < 1:
            raise ValueError(f"{who}: max_iter must be at least 1, got {max_iter}")
        rng = np.random.Generator(np.random.PCG64(seed))
        n_eff = 1.0 / np.sum(w * w)                                       # Kish
        xc = x - w @ x
        S0 = (w * xc.T) @ xc
        S0 = 0.5 * (S0 + S0.T)
        floor = cov_floor * np.trace(S0) / k * np.eye(k)
        # k-means++ on the weighted rows
        centres = [x[rng.choice(n, p=w)]]
        d2 = np.sum((x - centres[0]) ** 2, axis=1)
        for c in range(1, C):
            p = w * d2
            if not p.sum() > 0:
                raise ValueError(f"{who}: the rows with weight hold fewer than {C} distinct points; use fewer components")
            centres.append(x[rng.choice(n, p=p / p.sum())])
            d2 = np.minimum(d2, np.sum((x - centres[-1]) ** 2, axis=1))
        pi, means, covs = np.full(C, 1.0 / C), np.array(centres), np.stack([S0] * C)
        loglik, converged = [], False
        for it in range(max_iter):
            lr = np.empty((C, n))
            for c in range(C):
                try:
                    L = np.linalg.cholesky(covs[c])
                except np.linalg.LinAlgError:
                    raise ValueError(f"{who}: component {c}: its covariance is not positive definite at E-step {it}; use "
                                     "fewer components or a larger cov_floor") from None
                y = solve_triangular(L, (x - means[c]).T, lower=True)
                lr[c] = (np.log(pi[c]) - 0.5 * np.sum(y * y, axis=0)) - (np.sum(np.log(np.diag(L))) + 0.5 * k * np.log(2 * np.pi))
            lse = logsumexp(lr, axis=0)
            loglik.append(float(w @ lse))
            if it > 0 and loglik[-1] - loglik[-2] < tol:
                converged = True
                break
            if it == max_iter - 1:
                break                                                     # (the parameters stay those of the last E-step)
            resp = w * np.exp(lr - lse)                                   # (C, n): weight times responsibility
            mass = resp.sum(axis=1)
            for c in range(C):
                if mass[c] * n_eff < k + 1:
                    raise ValueError(f"{who}: component {c} has collapsed: its responsibility mass is {mass[c] * n_eff:.3g} "
                                     f"of {n_eff:.3g} effective rows (below k + 1 = {k + 1}); use fewer components")
                means[c] = (resp[c] @ x) / mass[c]
                xm = x - means[c]
                S = (resp[c] * xm.T) @ xm / mass[c] + floor
                covs[c] = 0.5 * (S + S.T)
            pi = mass / mass.sum()
        prior = cls(pi, means, covs)
        prior.fit_info = dict(iterations=len(loglik), converged=converged, loglik=np.array(loglik))
        return prior

    @classmethod
    def from_sampler(cls, sampler, columns=None, n_components=2, **fit):
        """The mixture fitted to a finished ``Sampler`` run's weighted posterior samples (``sampler.posterior()``), on
        ``columns`` of its parameters in that order (None: all of them), taken as ``FlowPrior.from_sampler(columns=...)``
        takes them; ``fit``: ``from_samples``'s other arguments.  ``ValueError`` unless the sampler has run to beta = 1."""
        FlowPrior._finished(sampler)
        ndim = sampler.scaler.ndim
        if columns is None:
            cols = np.arange(ndim)
        else:
            k = len(columns) if hasattr(columns, "__len__") else 1
            cols, _ = JointPrior.layout(columns, k, ndim - k)            # (checks them: distinct integers in [0, ndim))
        samples, weights = sampler.posterior()[:2]
        return cls.from_samples(np.asarray(samples)[:, cols], weights, n_components=n_components, **fit)

    # ----------------------------------------------------------------- state
    def __getstate__(self):
        fit = None if self.fit_info is None else dict(self.fit_info, loglik=np.array(self.fit_info["loglik"]))
        return dict(weights=self.weights.copy(), means=self.means.copy(), covs=self.covs.copy(), logw=self.logw.copy(),
                    L=self.L.copy(), linv_packed=self.linv_packed.copy(), logc=self.logc.copy(), fit_info=fit)

    def __setstate__(self, st):
        for key in ("weights", "means", "covs", "logw", "L", "linv_packed", "logc"):
            setattr(self, key, np.array(st[key], dtype=np.float64))
        self.fit_info = st.get("fit_info")
        self._dev = None

    def device_block(self):
        """The device's constants as numpy arrays: ``logw`` (C,), ``mean`` (C, k), ``linv_packed`` (C, k (k + 1) / 2): row i of
        component c's inverse Cholesky factor at ``[c, i (i + 1) / 2]``, and ``logc`` (C,).  No torch, no GPU."""
        return dict(logw=self.logw.copy(), mean=self.means.copy(), linv_packed=self.linv_packed.copy(), logc=self.logc.copy())

    def _device(self, device):
        """The device's copies and the descriptor of the mixture alone, made once, on ``device``."""
        if self._dev is None:
            import torch
            k = self.dim
            dev = torch.device(device)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d = dict(device=dev, logw=up(self.logw), mean=up(self.means), linv=up(self.linv_packed), logc=up(self.logc),
                     cols=up(np.arange(k, dtype=np.int32)))
            d["desc"] = self._descriptor(d, d["cols"], k)           # (it points into the tensors next to it)
            self._dev = d
        return self._dev

    def _descriptor(self, d, cols, D, rest=None, rest_cols=None):
        """``pmc_gauss_mix_t`` of this mixture on the columns ``cols`` (a device tensor) of a ``D``-column x."""
        from . import _lib
        return _lib.pmc_gauss_mix_t(n_comp=self.components, dim=self.dim, D=D, reserved=0, cols=cols.data_ptr(),
                                    logw=d["logw"].data_ptr(), mean=d["mean"].data_ptr(), linv=d["linv"].data_ptr(),
                                    logc=d["logc"].data_ptr(), rest=rest, rest_cols=rest_cols)

    # ----------------------------------------------------------------- density
    logpdf_device = GaussianPrior.logpdf_device      # the same checks and layouts around _device and _launch
    logpdf = GaussianPrior.logpdf

    def _launch(self, d, x_ptr, strides, n, out_ptr):
        import ctypes as C
        from . import _lib
        _lib.check(_lib.load().pmc_gauss_mix_logpdf(C.byref(d["desc"]), x_ptr, strides[0], strides[1], n, None, out_ptr,
                                                    _lib.stream_handle()), "pmc_gauss_mix_logpdf")

    # ----------------------------------------------------------------- draws
    def rvs(self, size=1):
        size = int(size)
        glob = np.random.mtrand._rand                                     # (numpy's global generator, named: JointPrior.rvs)
        comp = glob.choice(self.components, size=size, p=np.exp(self.logw))      # first the components ...
        z = glob.standard_normal((size, self.dim))                               # ... then one block of normals
        return self.means[comp] + np.einsum("rj,rij->ri", z, self.L[comp])

    @property
    def components(self):
        return len(self.logw)

    @property
    def bounds(self):
        return np.stack([np.full(self.dim, -np.inf), np.full(self.dim, np.inf)], axis=1)

    @property
    def dim(self):
        return self.means.shape[1]


class KDEPrior:
    """A weighted Gaussian kernel density estimate of samples, ``p(x) = sum_m w_m N(x; s_m, H)`` with ONE shared bandwidth
    matrix ``H``: the earlier result that arrives as a chain -- a published MCMC chain, another run's weighted posterior on a
    few shared parameters -- when nothing is to be fitted to it.  No fit, no random number, exactly normalised, exactly
    sampled, float64 throughout.  ``1 <= M <= 65536`` samples (``MAX_SAMPLES``) on ``1 <= k <= 16`` columns (``MAX_DIM``).

    The estimate has NO support restriction: around samples of a bounded parameter it puts mass outside the bounds (about
    half a kernel's for a sample on a bound).  Bounded parameters leak mass; a box around the estimate is out of scope.

    ``samples``    ``(M, k)`` floats;  ``weights``  ``(M,)`` finite, not negative, not all zero (None: equal).  Rows of weight
                   zero are dropped before anything else (their values are not looked at); what remains must be finite.
                   More than 65536 rows: thin the chain; more than 16 columns: choose fewer.
    ``bandwidth``  ``"scott"``, ``"silverman"``, a positive float ``f``, or a ``(k, k)`` symmetric positive definite matrix
                   taken as ``H`` itself.  For the first three ``H = f^2 C`` with ``C`` the weighted sample covariance as
                   ``scipy.stats.gaussian_kde`` forms it (divided by ``1 - sum w^2``, ``w`` the normalised weights),
                   ``neff = 1 / sum w^2``, Scott's ``f = neff^(-1 / (k + 4))`` and Silverman's
                   ``f = (neff (k + 2) / 4)^(-1 / (k + 4))``.  A ``C`` that is not positive definite (too few distinct rows)
                   is refused: a matrix ``bandwidth=`` takes an ``H`` from elsewhere.
    The constructor is numpy and scipy alone.  ``center`` is the weighted mean of the samples; ``linv_packed`` and
    ``logc = k / 2 log(2 pi) + 1/2 log|H|`` are ``GaussianPrior._constants(center, H)``'s (its checks and texts apply, behind
    ``KDEPrior: ``); ``t = (samples - center) @ Linv.T`` are the whitened samples and ``logw = log(w / sum w)`` (exactly 0.0
    for M = 1); ``device_block()`` gives them.  The state carries the inputs kept (the samples and weights after the drop,
    ``H``) and these constants; the device's copies are made at the first device call and dropped on pickling.

    ``logpdf_device(x)``  the ``DevicePrior`` contract, as ``GaussianPrior.logpdf_device``: an ``(n, k)`` float64 tensor on the
                          device in, an ``(n,)`` float64 tensor out, on the current stream, in ONE launch
                          (``pmc_kde_logpdf``, ``csrc/kde_prior.hip``) and no host synchronisation; no copy of ``x`` when it
                          is C-contiguous or the MCMC step's column-major view (any other layout is made contiguous once);
                          ``n == 0`` gives an empty tensor.  A row is whitened once, ``y = Linv (x - center)``, and the value
                          is ``(mx + log sum_m exp(e_m - mx)) - logc`` with ``e_m = -0.5 |y - t_m|^2 + logw_m`` and
                          ``mx = max_m e_m`` (``include/pocomc_amd.h``, ``tests/kde_model.py``): within
                          ``(M + 8) 2^-52 + 2^-50 (|v| + |logc|)`` of that statement.  -inf for a row with a NaN or an inf
                          and for a row every kernel gives -inf; never NaN, never +inf.  With one sample:
                          ``GaussianPrior(samples[0], H)``'s bits.
    ``logpdf(x)``         numpy in, numpy out, through the same function.
    ``rvs(size)``         two draws from numpy's GLOBAL generator (``Sampler(random_state=...)`` reaches it), in this order:
                          first the ``size`` sample indices by the weights (``choice``), then ONE standard-normal
                          ``(size, k)`` block; row r is ``samples[m_r] + z_r @ L.T``.
    ``bounds``, ``dim``   ``(k, 2)`` of -inf / +inf, and k.

    ``from_samples(x, weights, columns=...)`` selects columns first; ``from_sampler(s, columns=...)`` takes a finished run's
    weighted posterior.  There is no ``device_descriptor`` and no ``step_stage``: the step calls the function
    (``Sampler(device_likelihood=True, device_prior=True)``).  ``JointPrior`` takes it as a block.  Out of scope: a box or any
    other support restriction, per-sample bandwidths, thinning, more than 16 columns or 65536 samples."""

    MAX_DIM = 16             # PMC_KDE_MAX_DIM
    MAX_SAMPLES = 65536      # PMC_KDE_MAX_SAMPLES

    def __init__(self, samples, weights=None, bandwidth="scott"):
        self.__setstate__(self._constants(samples, weights, bandwidth))

    @classmethod
    def _constants(cls, samples, weights, bandwidth):
        """The checks and the host-side constants: the state of a ``KDEPrior(samples, weights, bandwidth)``."""
        who = "KDEPrior"
        try:
            s = np.array(samples, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: samples must be an (M, k) array of floats") from None
        if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError(f"{who}: samples must have shape (M, k) with M >= 1 and k >= 1, got {s.shape}")
        k = s.shape[1]
        if k > cls.MAX_DIM:
            raise ValueError(f"{who}: samples have {k} columns (1 <= k <= {cls.MAX_DIM}): choose fewer columns "
                             "(from_samples(..., columns=...)); the other parameters take other priors in a JointPrior")
        if weights is None:
            w = np.ones(len(s), dtype=np.float64)
        else:
            try:
                w = np.array(weights, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: weights must be an (M,) array of floats") from None
            if w.shape != (len(s),):
                raise ValueError(f"{who}: weights must have shape ({len(s)},), got {w.shape}")
            if not (np.isfinite(w) & (w >= 0)).all():
                j = int(np.argmin(np.isfinite(w) & (w >= 0)))
                raise ValueError(f"{who}: weights[{j}] = {float(w[j])!r} is not finite and non-negative")
            if not (w > 0).any():
                raise ValueError(f"{who}: every weight is zero")
            s, w = s[w > 0], w[w > 0]                                        # (before anything else)
        M = len(s)
        if M > cls.MAX_SAMPLES:
            raise ValueError(f"{who}: {M} samples of weight above zero (1 <= M <= {cls.MAX_SAMPLES}): thin the chain "
                             "(every j-th row, or a resample by the weights)")
        if not np.isfinite(s).all():
            i, j = np.argwhere(~np.isfinite(s))[0]
            raise ValueError(f"{who}: samples[{i}, {j}] is not finite (row {i} of the rows of weight above zero)")
        with np.errstate(all="ignore"):
            wn = w / w.sum()
            logw = np.log(wn)
        if not np.isfinite(logw).all():
            raise ValueError(f"{who}: a weight vanishes next to the weights' sum (or the sum overflows): rescale the weights")
        center = (wn[:, None] * s).sum(axis=0)
        xm = s - center
        factor = None
        matrix = not isinstance(bandwidth, str) and np.ndim(bandwidth) == 2
        if matrix:
            try:
                H = np.array(bandwidth, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: a matrix bandwidth must be a ({k}, {k}) array of floats") from None
            if H.shape != (k, k):
                raise ValueError(f"{who}: a matrix bandwidth must have shape ({k}, {k}), got {H.shape}")
        else:
            neff = 1.0 / float(np.sum(wn ** 2))
            if isinstance(bandwidth, str):
                if bandwidth == "scott":
                    factor = float(np.power(neff, -1.0 / (k + 4)))
                elif bandwidth == "silverman":
                    factor = float(np.power(neff * (k + 2.0) / 4.0, -1.0 / (k + 4)))
                else:
                    raise ValueError(f"{who}: bandwidth must be 'scott', 'silverman', a positive float or a ({k}, {k}) matrix, "
                                     f"got {bandwidth!r}")
            else:
                try:
                    factor = float(bandwidth)
                except (TypeError, ValueError):
                    raise ValueError(f"{who}: bandwidth must be 'scott', 'silverman', a positive float or a ({k}, {k}) "
                                     f"matrix, got {bandwidth!r}") from None
                if not (np.isfinite(factor) and factor > 0):
                    raise ValueError(f"{who}: the bandwidth factor must be finite and positive, got {factor!r}")
            # scipy.stats.gaussian_kde's covariance: np.cov(samples.T, aweights=wn), that is divided by 1 - sum wn^2
            with np.errstate(all="ignore"):
                Cw = (xm.T * wn) @ xm / (1.0 - float(np.sum(wn ** 2)))
            Cw = 0.5 * (Cw + Cw.T)
            # (k or fewer distinct rows span no k-dimensional volume, whatever rounding leaves on the diagonal)
            ok = bool(np.isfinite(Cw).all()) and len(np.unique(s, axis=0)) > k
            if ok:
                try:
                    np.linalg.cholesky(Cw)
                except np.linalg.LinAlgError:
                    ok = False
            if not ok:
                raise ValueError(f"{who}: the weighted covariance of the {M} samples is not positive definite (too few "
                                 "distinct rows): a matrix bandwidth=H takes an H from elsewhere")
            H = factor ** 2 * Cw
        try:
            g = GaussianPrior._constants(center, H)
        except ValueError as e:
            text = str(e)
            text = text[len("GaussianPrior: "):] if text.startswith("GaussianPrior: ") else text
            raise ValueError(f"{who}: {text} (mean: the samples' weighted mean, cov: the bandwidth matrix H)") from None
        k_idx = np.tril_indices(k)
        Linv = np.zeros((k, k), dtype=np.float64)
        Linv[k_idx] = g["linv_packed"]
        with np.errstate(all="ignore"):
            t = np.ascontiguousarray(xm @ Linv.T)
        if not np.isfinite(t).all():
            raise ValueError(f"{who}: the samples are too far apart for the bandwidth: a whitened sample is not finite")
        return dict(samples=s, weights=w, H=g["cov"], factor=factor, center=g["mean"], L=g["L"],
                    linv_packed=g["linv_packed"], logc=g["logc"], t=t, logw=logw)

    # ----------------------------------------------------------------- other sources
    @classmethod
    def from_samples(cls, x, weights=None, columns=None, bandwidth="scott"):
        """The estimate of the ``columns`` of ``x`` ``(n, d)`` in that order (None: all of them; distinct integers in
        ``[0, d)``), with the constructor's ``weights`` and ``bandwidth``."""
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError(f"KDEPrior.from_samples: x must have shape (n, d), got {x.shape}")
        if columns is not None:
            k = len(columns) if hasattr(columns, "__len__") else 1
            cols, _ = JointPrior.layout(columns, k, x.shape[1] - k)          # (checks them: distinct integers in [0, d))
            x = x[:, cols]
        return cls(x, weights, bandwidth)

    @classmethod
    def from_sampler(cls, sampler, columns=None, bandwidth="scott"):
        """The estimate of a finished ``Sampler`` run's weighted posterior samples (``sampler.posterior()``), on ``columns``
        of its parameters in that order (None: all of them), taken as ``FlowPrior.from_sampler(columns=...)`` takes them.
        ``ValueError`` unless the sampler has run to beta = 1."""
        FlowPrior._finished(sampler)
        samples, weights = sampler.posterior()[:2]
        return cls.from_samples(np.asarray(samples), weights, columns=columns, bandwidth=bandwidth)

    # ----------------------------------------------------------------- state
    _ARRAYS = ("samples", "weights", "H", "center", "L", "linv_packed", "t", "logw")

    def __getstate__(self):
        st = {key: getattr(self, key).copy() for key in self._ARRAYS}
        st.update(logc=self.logc, factor=self.factor)
        return st

    def __setstate__(self, st):
        for key in self._ARRAYS:
            setattr(self, key, np.array(st[key], dtype=np.float64))
        self.logc = float(st["logc"])
        self.factor = None if st.get("factor") is None else float(st["factor"])      # (None: H was given as a matrix)
        self._dev = None

    def device_block(self):
        """The device's constants as numpy arrays: ``center`` (k,), ``linv_packed`` (k (k + 1) / 2,) in ``GaussianPrior``'s
        packing, ``t`` (M, k) the whitened samples, ``logw`` (M,) and ``logc`` (a 0-d array).  No torch, no GPU."""
        return dict(center=self.center.copy(), linv_packed=self.linv_packed.copy(), t=self.t.copy(), logw=self.logw.copy(),
                    logc=np.array(self.logc, dtype=np.float64))

    def _device(self, device):
        """The device's copies and the descriptor of the estimate alone, made once, on ``device``."""
        if self._dev is None:
            import torch
            k = self.dim
            dev = torch.device(device)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            d = dict(device=dev, center=up(self.center), linv=up(self.linv_packed), t=up(self.t), logw=up(self.logw),
                     cols=up(np.arange(k, dtype=np.int32)))
            d["desc"] = self._descriptor(d, d["cols"], k)           # (it points into the tensors next to it)
            self._dev = d
        return self._dev

    def _descriptor(self, d, cols, D, rest=None, rest_cols=None):
        """``pmc_kde_t`` of this estimate on the columns ``cols`` (a device tensor) of a ``D``-column x."""
        from . import _lib
        return _lib.pmc_kde_t(n_samples=self.n_samples, dim=self.dim, D=D, reserved=0, cols=cols.data_ptr(),
                              center=d["center"].data_ptr(), linv=d["linv"].data_ptr(), t=d["t"].data_ptr(),
                              logw=d["logw"].data_ptr(), logc=self.logc, rest=rest, rest_cols=rest_cols)

    # ----------------------------------------------------------------- density
    logpdf_device = GaussianPrior.logpdf_device      # the same checks and layouts around _device and _launch
    logpdf = GaussianPrior.logpdf

    def _launch(self, d, x_ptr, strides, n, out_ptr):
        import ctypes as C
        from . import _lib
        _lib.check(_lib.load().pmc_kde_logpdf(C.byref(d["desc"]), x_ptr, strides[0], strides[1], n, None, out_ptr,
                                              _lib.stream_handle()), "pmc_kde_logpdf")

    # ----------------------------------------------------------------- draws
    def rvs(self, size=1):
        size = int(size)
        glob = np.random.mtrand._rand                                     # (numpy's global generator, named: JointPrior.rvs)
        idx = glob.choice(self.n_samples, size=size, p=self.weights / self.weights.sum())     # first the samples ...
        z = glob.standard_normal((size, self.dim))                                            # ... then one block of normals
        return self.samples[idx] + z @ self.L.T

    @property
    def n_samples(self):
        return len(self.logw)

    @property
    def bounds(self):
        return np.stack([np.full(self.dim, -np.inf), np.full(self.dim, np.inf)], axis=1)

    @property
    def dim(self):
        return self.samples.shape[1]


class JointPrior:
    """A flow prior on some of the parameters and scipy factors on the others:

        ``log p(x) = flow_prior.logpdf(x[:, columns]) + sum_m rest.dists[m].logpdf(x[:, rest_cols[m]])``.

    The usual case of two experiments that share a block of parameters: run A's posterior on the shared block (a
    ``FlowPrior``, see ``FlowPrior.from_sampler(a, columns=...)``) and ordinary priors on run B's own nuisance parameters.

    ``flow_prior``  a ``FlowPrior``;
    ``columns``     the positions in the joint ``x`` of the flow prior's dimensions: ``flow_prior.dim`` distinct integers, in
                    any order (``x[:, columns[k]]`` is the flow prior's dimension k);
    ``rest``        a ``Prior`` the device evaluates (``Prior(dists, device=True)``, or uniform / normal factors), with at
                    least one factor; its factors fill the remaining positions in increasing order.

    ``logpdf_device(x)``  the ``DevicePrior`` contract, in three launches on the current stream: ``pmc_joint_prior_pre`` (one
                          pass over ``x``: the flow block's u as float32, its scaler's log-determinant, the table factors' sum,
                          the support test), the flow's own forward call with ``log_prob``, ``pmc_joint_prior_post``.  No host
                          synchronisation; no copy of ``x`` when it is C-contiguous or the MCMC step's column-major view.  -inf
                          outside the support of either part, on a bound of the flow block, at a pole of a factor and for rows
                          with a NaN or an inf; never NaN, never +inf.  A row's value does not depend on the layout, on ``n``
                          or on its place in ``x``, and is ``flow_prior.logpdf_device`` of the gathered block plus
                          ``pmc_prior_logpdf`` of the gathered rest, bit for bit.
    ``logpdf(x)``         numpy in, numpy out, through the same function.
    ``rvs(size)``         the flow columns from ``flow_prior.rvs``, the others from ``rest.rvs``.
    ``bounds``, ``dim``   the two parts', merged by position.

    The prior owns copies of both parts (the flow prior through its pickled state, the table as arrays): later changes to the
    sources do not move it.  There is no ``device_descriptor``: the step calls the function.

    The blocks form: ``JointPrior([fp_0, fp_1, ...], [columns_0, columns_1, ...], rest=None)`` -- a list or tuple of
    1 <= B <= 8 ``FlowPrior`` s (on one device) and as many column lists; ``rest`` a ``Prior`` as above, or None when the blocks
    cover every column:

        ``log p(x) = sum_b flow_priors[b].logpdf(x[:, columns_b]) + sum_m rest.dists[m].logpdf(x[:, rest_cols[m]])``.

    ``flow_priors`` is the tuple of owned copies, ``blocks`` its length (0 in the single form, whose ``flow_prior`` the blocks
    form does not have).  ``logpdf_device`` is B + 2 launches and one pass over ``x``: ``pmc_joint_blocks_pre`` (every block's
    u as float32 -- each block with its own scaler, transform included --, the scalers' log-determinants, the table's sum, one
    support flag per row), every block's forward call with ``log_prob`` in block order (a ``precision="bf16"`` block keeps
    its matrix-core kernel), ``pmc_joint_blocks_post``; the value is the left-to-right float64 sum of the blocks'
    ``FlowPrior.logpdf_device`` on their gathered columns and ``pmc_prior_logpdf`` of the gathered rest, bit for bit, with
    the single form's contract otherwise.  ``rvs`` draws block 0, block 1, ... with each block's ``rvs`` (torch's global
    generator), then the rest with numpy's global generator.  ``step_stage`` gives the step a ``pmc_prior_blocks_stage_t``.

    Gaussian blocks: the list takes a ``GaussianPrior`` wherever it takes a ``FlowPrior`` (of one column too), at most 8 blocks
    of both kinds together, with or without a flow block: ``JointPrior([shared_a, planck], [[4, 0, 2], [1, 5, 6]], own)``,
    ``JointPrior([planck], [[1, 5, 6]], own)``.  ``blocks`` counts the blocks of both kinds, ``flow_priors`` and
    ``gaussian_priors`` are the owned copies of each kind in list order (a Gaussian block is copied through its state).  The
    value is the flow blocks' and the table's value as above, then ``+ g`` for every Gaussian block in list order -- the
    Gaussian blocks are added AFTER the flow blocks and the table, whatever their place in the list -- and equals the parts
    evaluated on their gathered columns and added in that order, bit for bit; -inf outside any part's support, never NaN.
    With a flow block the launches above run over the flow blocks and the table and one ``pmc_gauss_blocks_logpdf`` launch adds
    the Gaussian blocks in place (B_flow + 3 launches); without one that launch evaluates the table as well (one launch, one
    pass over ``x``).  ``rvs`` and ``bounds`` go by list order.  ``step_stage`` raises ``ValueError``: a prior with a Gaussian
    block is for ``logpdf`` and for ``device_prior=True``, not for the step of a host likelihood.

    A ``TruncatedGaussianPrior`` is a Gaussian block as well (a block kind of its own in the state, ``"gauss_box"``): it is
    listed in ``gaussian_priors``, added after the flow blocks and the table in list order, and refused by ``step_stage`` in
    the same words.  As soon as one block has a box the Gaussian launch is ``pmc_gauss_box_logpdf`` (plain Gaussian blocks go
    along without a box); without one it is ``pmc_gauss_blocks_logpdf`` as before.  The whole row is -inf as soon as any
    block's box is violated, ``bounds`` reports the box on those columns and ``rvs`` stays inside it.

    Mixture blocks: the list takes a ``GaussianMixturePrior`` wherever it takes a ``FlowPrior`` or a ``GaussianPrior`` (block
    kind ``"gmix"`` in the state; states without the kind still load), at most 8 blocks of all kinds, distinct columns, 157
    dimensions.  ``mixture_priors`` are the owned copies in list order, copied through their state.  The value is that of the
    same prior without its mixture blocks -- flow blocks in list order, the table, Gaussian blocks in list order -- THEN
    ``+ v`` for every mixture block in list order, ``v`` the block's own ``logpdf_device`` on its gathered columns: bit for bit
    that left-to-right float64 sum, -inf outside any part's support, never NaN.  Each mixture block is one
    ``pmc_gauss_mix_logpdf`` launch that adds in place behind the launches that exist; where no flow block and no Gaussian
    block precedes, the first mixture launch evaluates the table as well (one pass over ``x`` for that launch).  ``rvs`` and
    ``bounds`` go by list order; ``step_stage`` raises ``ValueError`` as for a Gaussian block.  A prior without a mixture block
    takes the path and the launches it took before.

    KDE blocks: the list takes a ``KDEPrior`` wherever it takes a ``GaussianMixturePrior`` (block kind ``"kde"`` in the state;
    states without the kind still load), with the same limits: at most 8 blocks of all kinds, distinct columns, 157
    dimensions, one device.  ``kde_priors`` are the owned copies in list order, copied through their state.  The value is that
    of the same prior without its KDE blocks -- flow blocks, the table, Gaussian blocks, mixture blocks, in the order above
    -- THEN ``+ v`` for every KDE block in list order, ``v`` the block's own ``logpdf_device`` on its gathered columns: bit
    for bit that left-to-right float64 sum.  Each KDE block is one ``pmc_kde_logpdf`` launch that adds in place behind the
    launches that exist; where nothing precedes, the first KDE launch evaluates the table as well.  ``step_stage`` raises
    ``ValueError``.  A prior without a KDE block takes the path and the launches it took before.

    Out of scope: more than 8 blocks, a box around a mixture or a KDE, mixture blocks folded into the Gaussian launch, non-diagonal
    scalers, the stage on sharded walkers, singular Gaussian blocks, boxes that
    are not axis-aligned, and -- as for every ``DevicePrior`` -- lanes and graph capture."""

    MAX_DIM = FlowPrior.MAX_DIM
    MAX_BLOCKS = 8           # PMC_JOINT_BLOCKS_MAX
    _WORKSPACES = FlowPrior._WORKSPACES

    @staticmethod
    def layout(columns, flow_dim, rest_dim):
        """``(flow_cols, rest_cols)`` as int32 arrays: ``flow_cols`` is ``columns`` (``flow_dim`` distinct integers in
        ``[0, flow_dim + rest_dim)``), ``rest_cols`` the ``rest_dim`` other positions in increasing order.  ``ValueError`` for
        duplicates, for entries out of range or not integers and for a wrong count.  Pure numpy."""
        flow_dim, rest_dim = int(flow_dim), int(rest_dim)
        if flow_dim < 0 or rest_dim < 0:
            raise ValueError(f"JointPrior.layout: negative dimension (flow_dim = {flow_dim}, rest_dim = {rest_dim})")
        try:
            cols = np.asarray(columns)
        except (TypeError, ValueError):
            cols = np.asarray(columns, dtype=object)
        if cols.size == 0:
            cols = cols.astype(np.int64)
        if cols.ndim != 1 or cols.dtype == np.bool_ or not np.issubdtype(cols.dtype, np.integer):
            raise ValueError(f"JointPrior.layout: columns must be a sequence of integers, got {columns!r}")
        if len(cols) != flow_dim:
            raise ValueError(f"JointPrior.layout: {len(cols)} columns for a flow prior of {flow_dim} dimensions")
        D = flow_dim + rest_dim
        if ((cols < 0) | (cols >= D)).any():
            raise ValueError(f"JointPrior.layout: columns must lie in [0, {D}), got {cols.tolist()}")
        if len(np.unique(cols)) != len(cols):
            raise ValueError(f"JointPrior.layout: columns are not distinct: {cols.tolist()}")
        rest_cols = np.setdiff1d(np.arange(D), cols)
        return cols.astype(np.int32), rest_cols.astype(np.int32)

    @staticmethod
    def layout_blocks(columns, flow_dims, rest_dim):
        """``(block_cols, rest_cols)``: ``block_cols[b]`` is ``columns[b]`` as an int32 array (``flow_dims[b]`` integers in
        ``[0, sum(flow_dims) + rest_dim)``, distinct within the block and across blocks), ``rest_cols`` the ``rest_dim``
        other positions in increasing order.  ``ValueError`` for a number of column lists that is not the number of blocks,
        a wrong count in a block, entries out of range or not integers, duplicates within a block and an overlap between two
        blocks (both are named).  Pure numpy."""
        flow_dims = [int(d) for d in flow_dims]
        rest_dim = int(rest_dim)
        if rest_dim < 0 or any(d < 0 for d in flow_dims):
            raise ValueError(f"JointPrior.layout_blocks: negative dimension (flow_dims = {flow_dims}, rest_dim = {rest_dim})")
        try:
            lists = list(columns)
        except TypeError:
            raise ValueError(f"JointPrior.layout_blocks: columns must be a sequence of column lists, got {columns!r}") from None
        if len(lists) != len(flow_dims):
            raise ValueError(f"JointPrior.layout_blocks: {len(lists)} column lists for {len(flow_dims)} blocks")
        D = sum(flow_dims) + rest_dim
        maps, owner = [], {}
        for b, (cols_in, Df) in enumerate(zip(lists, flow_dims)):
            try:
                cols = np.asarray(cols_in)
            except (TypeError, ValueError):
                cols = np.asarray(cols_in, dtype=object)
            if cols.size == 0:
                cols = cols.astype(np.int64)
            if cols.ndim != 1 or cols.dtype == np.bool_ or not np.issubdtype(cols.dtype, np.integer):
                raise ValueError(f"JointPrior.layout_blocks: block {b}: columns must be a sequence of integers, got {cols_in!r}")
            if len(cols) != Df:
                raise ValueError(f"JointPrior.layout_blocks: block {b}: {len(cols)} columns for a flow prior of {Df} dimensions")
            if ((cols < 0) | (cols >= D)).any():
                raise ValueError(f"JointPrior.layout_blocks: block {b}: columns must lie in [0, {D}), got {cols.tolist()}")
            if len(np.unique(cols)) != len(cols):
                raise ValueError(f"JointPrior.layout_blocks: block {b}: columns are not distinct: {cols.tolist()}")
            for c in cols.tolist():
                if c in owner:
                    raise ValueError(f"JointPrior.layout_blocks: blocks {owner[c]} and {b} overlap (column {c})")
                owner[c] = b
            maps.append(cols.astype(np.int32))
        rest_cols = np.setdiff1d(np.arange(D), np.fromiter(owner, dtype=np.int64, count=len(owner)))
        return maps, rest_cols.astype(np.int32)

    def __init__(self, flow_prior, columns, rest=None):
        if isinstance(flow_prior, (list, tuple)):
            self._init_blocks(flow_prior, columns, rest)
            return
        if not isinstance(flow_prior, FlowPrior):
            raise ValueError(f"JointPrior: flow_prior must be a pocomc_amd.FlowPrior, got {type(flow_prior).__name__}")
        if not isinstance(rest, Prior):
            raise ValueError(f"JointPrior: rest must be a pocomc_amd.Prior, got {type(rest).__name__}")
        if rest.dists is None or rest.dim < 1:
            raise ValueError("JointPrior: rest needs at least one factor")
        if rest.device_table() is None:
            raise ValueError("JointPrior: the device must evaluate rest: build it as Prior(dists, device=True)")
        if flow_prior.dim + rest.dim > self.MAX_DIM:
            raise ValueError(f"JointPrior: n_dim = {flow_prior.dim} + {rest.dim} is too large (n_dim <= {self.MAX_DIM})")
        flow_cols, _ = self.layout(columns, flow_prior.dim, rest.dim)
        self._restore(flow_prior.__getstate__(), flow_cols.tolist(), rest, flow_prior.flow.device)

    # ----------------------------------------------------------------- state
    def _restore(self, flow_prior_state, columns, rest, device=None):
        import copy
        import torch
        from . import _lib
        self.flow_prior = FlowPrior.__new__(FlowPrior)
        self.flow_prior._restore(flow_prior_state["flow"], flow_prior_state["scaler"], device)
        self.rest = copy.deepcopy(rest)
        self._flow_cols, self._rest_cols = self.layout(columns, self.flow_prior.dim, self.rest.dim)
        tab = self.rest.device_table()
        dev = self.flow_prior.flow.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        n_ext = int((tab["family"] > 2).sum())
        # (the descriptor points into these tensors: they live as long as it does)
        self._dev = dict(family=up(tab["family"]), loc=up(tab["loc"]), scale=up(tab["scale"]),
                         par=up(tab["par"]) if n_ext else None, flow_cols=up(self._flow_cols), rest_cols=up(self._rest_cols))
        self._rdesc = _lib.pmc_prior_t(family=self._dev["family"].data_ptr(), loc=self._dev["loc"].data_ptr(),
                                       scale=self._dev["scale"].data_ptr(), D=len(tab["family"]), reserved=0,
                                       par=self._dev["par"].data_ptr() if n_ext else None, n_extended=n_ext, reserved2=0)
        self._ws = {}

    def __getstate__(self):
        if self.blocks:
            st = {"flow_priors": [p.__getstate__() for p in self._parts],
                  "columns": [c.tolist() for c in self._block_cols], "rest": self.rest}
            if self.gaussian_priors or self.mixture_priors or self.kde_priors:
                # (the blocks in list order: a flow's state, a Gaussian's, a mixture's, a KDE's)
                st["kinds"] = list(self._kinds)
            return st
        return {"flow_prior": self.flow_prior.__getstate__(), "columns": self._flow_cols.tolist(), "rest": self.rest}

    def __setstate__(self, st):
        if "flow_priors" in st:
            self._restore_blocks(st["flow_priors"], st["columns"], st["rest"], kinds=st.get("kinds"))
        else:
            self._restore(st["flow_prior"], st["columns"], st["rest"])

    # ----------------------------------------------------------------- the blocks form
    blocks = 0                    # the number of flow blocks in the blocks form; 0: the single form (``flow_prior``)

    def _init_blocks(self, flow_priors, columns, rest):
        B = len(flow_priors)
        for b, fp in enumerate(flow_priors):
            if not isinstance(fp, (FlowPrior, GaussianPrior, GaussianMixturePrior, KDEPrior)):
                raise ValueError(f"JointPrior: block {b} must be a pocomc_amd.FlowPrior or GaussianPrior or "
                                 f"GaussianMixturePrior, got {type(fp).__name__} (a KDEPrior is taken as well)")
        kinds = ["flow" if isinstance(fp, FlowPrior) else "gmix" if isinstance(fp, GaussianMixturePrior) else
                 "kde" if isinstance(fp, KDEPrior) else
                 "gauss_box" if isinstance(fp, TruncatedGaussianPrior) else "gauss" for fp in flow_priors]
        if not 1 <= B <= self.MAX_BLOCKS:
            n_flow, n_mix, n_kde = kinds.count("flow"), kinds.count("gmix"), kinds.count("kde")
            raise ValueError(f"JointPrior: {B} blocks ({n_flow} flow blocks, {B - n_flow - n_mix - n_kde} Gaussian blocks"
                             + (f", {n_mix} mixture blocks" if n_mix else "") + (f", {n_kde} KDE blocks" if n_kde else "")
                             + f"; 1 <= blocks <= {self.MAX_BLOCKS})")
        import torch
        # (a Gaussian block that has not been on a device yet goes where the others are)
        devs = [torch.device(fp.flow.device) if k == "flow" else None if fp._dev is None else fp._dev["device"]
                for k, fp in zip(kinds, flow_priors)]
        known = [b for b in range(B) if devs[b] is not None]
        for b in known[1:]:
            if devs[b] != devs[known[0]]:
                raise ValueError(f"JointPrior: blocks {known[0]} and {b} are on different devices ({devs[known[0]]}, {devs[b]})")
        if rest is not None:
            if not isinstance(rest, Prior):
                raise ValueError(f"JointPrior: rest must be a pocomc_amd.Prior or None, got {type(rest).__name__}")
            if rest.dists is None or rest.dim < 1:
                raise ValueError("JointPrior: rest needs at least one factor (rest=None: the blocks cover every column)")
            if rest.device_table() is None:
                raise ValueError("JointPrior: the device must evaluate rest: build it as Prior(dists, device=True)")
        dims, Dr = [fp.dim for fp in flow_priors], 0 if rest is None else rest.dim      # (blocks of both kinds)
        if sum(dims) + Dr > self.MAX_DIM:
            raise ValueError(f"JointPrior: n_dim = {' + '.join(str(d) for d in dims + [Dr])} is too large "
                             f"(n_dim <= {self.MAX_DIM})")
        maps, _ = self.layout_blocks(columns, dims, Dr)
        self._restore_blocks([fp.__getstate__() for fp in flow_priors], [m.tolist() for m in maps], rest,
                             devs[known[0]] if known else None, kinds)

    def _restore_blocks(self, states, columns, rest, device=None, kinds=None):
        """``states``, ``columns``, ``kinds`` (``"flow"`` / ``"gauss"`` / ``"gauss_box"``, a truncated Gaussian / ``"gmix"``, a
        mixture / ``"kde"``, a kernel density estimate; None: every block a flow): the blocks in list order."""
        import copy
        import ctypes as C
        import torch
        from . import _lib
        kinds = ["flow"] * len(states) if kinds is None else list(kinds)
        parts = []
        for kind, st in zip(kinds, states):
            if kind == "flow":
                fp = FlowPrior.__new__(FlowPrior)
                fp._restore(st["flow"], st["scaler"], device)
                device = fp.flow.device                            # (an unpickled prior: every block where the first one went)
            else:
                cls = {"gauss": GaussianPrior, "gauss_box": TruncatedGaussianPrior, "gmix": GaussianMixturePrior,
                       "kde": KDEPrior}[kind]
                fp = cls.__new__(cls)
                fp.__setstate__(copy.deepcopy(st))
            parts.append(fp)
        fps = [p for k, p in zip(kinds, parts) if k == "flow"]
        gps = [p for k, p in zip(kinds, parts) if k in ("gauss", "gauss_box")]      # (both Gaussian kinds, in list order)
        mps = [p for k, p in zip(kinds, parts) if k == "gmix"]
        kps = [p for k, p in zip(kinds, parts) if k == "kde"]
        self._kinds, self._parts = tuple(kinds), tuple(parts)
        self.flow_priors, self.gaussian_priors, self.mixture_priors = tuple(fps), tuple(gps), tuple(mps)
        self.kde_priors = tuple(kps)
        self.blocks = len(parts)
        self.rest = copy.deepcopy(rest)
        Dr = 0 if self.rest is None else self.rest.dim
        self._block_cols, self._rest_cols = self.layout_blocks(columns, [p.dim for p in parts], Dr)
        self._dim = sum(p.dim for p in parts) + Dr
        dev = torch.device(fps[0].flow.device if fps else device if device is not None else _lib.require_gpu())
        self._device = dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        flow_cols = [c for k, c in zip(kinds, self._block_cols) if k == "flow"]
        gauss_cols = [c for k, c in zip(kinds, self._block_cols) if k in ("gauss", "gauss_box")]
        mix_cols = [c for k, c in zip(kinds, self._block_cols) if k == "gmix"]
        kde_cols = [c for k, c in zip(kinds, self._block_cols) if k == "kde"]
        # (the descriptors point into these tensors: they live as long as the descriptors do)
        self._dev = dict(cols=[up(c) for c in flow_cols], gauss_cols=[up(c) for c in gauss_cols],
                         mix_cols=[up(c) for c in mix_cols], kde_cols=[up(c) for c in kde_cols],
                         rest_cols=up(self._rest_cols) if Dr else None)
        self._rdesc = None
        if Dr:
            tab = self.rest.device_table()
            n_ext = int((tab["family"] > 2).sum())
            self._dev.update(family=up(tab["family"]), loc=up(tab["loc"]), scale=up(tab["scale"]),
                             par=up(tab["par"]) if n_ext else None)
            self._rdesc = _lib.pmc_prior_t(family=self._dev["family"].data_ptr(), loc=self._dev["loc"].data_ptr(),
                                           scale=self._dev["scale"].data_ptr(), D=Dr, reserved=0,
                                           par=self._dev["par"].data_ptr() if n_ext else None, n_extended=n_ext, reserved2=0)
        rest_ptr = C.cast(C.pointer(self._rdesc), C.c_void_p) if Dr else None
        rest_cols_ptr = self._dev["rest_cols"].data_ptr() if Dr else None
        self._jdesc = None
        if fps:
            # (D: x has the Gaussian, mixture and KDE blocks' columns as well; 0 where the flow blocks and the table cover
            # every column)
            j = _lib.pmc_joint_blocks_t(n_blocks=len(fps), D=self._dim if gps or mps or kps else 0, rest=rest_ptr,
                                        rest_cols=rest_cols_ptr)
            for b, fp in enumerate(fps):
                j.scaler[b] = C.cast(C.pointer(fp._sdesc), C.c_void_p)
                j.cols[b] = self._dev["cols"][b].data_ptr()
            self._jdesc = j
        self._gdesc = self._gbox = None
        if gps:
            # (the table goes through this launch only where no flow launch has taken it)
            g = _lib.pmc_gauss_blocks_t(n_blocks=len(gps), D=self._dim, rest=None if fps else rest_ptr,
                                        rest_cols=None if fps else rest_cols_ptr)
            for b, gp in enumerate(gps):
                d = gp._device(dev)
                g.dim[b], g.logc[b] = gp.dim, gp._logc_device
                g.cols[b] = self._dev["gauss_cols"][b].data_ptr()
                g.mean[b], g.linv[b] = d["mean"].data_ptr(), d["linv"].data_ptr()
            self._gdesc = g
            if "gauss_box" in kinds:
                # (one truncated block sends the launch through pmc_gauss_box_logpdf; a plain block is a NULL pair)
                box = _lib.pmc_gauss_box_t()
                for b, gp in enumerate(gps):
                    if isinstance(gp, TruncatedGaussianPrior):
                        d = gp._device(dev)
                        box.lo[b], box.hi[b] = d["lo"].data_ptr(), d["hi"].data_ptr()
                self._gbox = box
        # one descriptor per mixture block, in list order; the table goes through the first one only where neither a flow
        # launch nor the Gaussian launch has taken it
        self._mdescs = []
        for b, mp in enumerate(mps):
            first = b == 0 and not fps and not gps
            self._mdescs.append(mp._descriptor(mp._device(dev), self._dev["mix_cols"][b], self._dim,
                                               rest_ptr if first else None, rest_cols_ptr if first else None))
        # and one per KDE block, likewise: the table goes through the first one only where nothing at all precedes
        self._kdescs = []
        for b, kp in enumerate(kps):
            first = b == 0 and not fps and not gps and not mps
            self._kdescs.append(kp._descriptor(kp._device(dev), self._dev["kde_cols"][b], self._dim,
                                               rest_ptr if first else None, rest_cols_ptr if first else None))
        self._offsets = np.concatenate([[0], np.cumsum([fp.dim for fp in fps])]).astype(np.int64)
        self._ws = {}

    def _workspace_blocks(self, n):
        import torch
        ws = self._ws.get(n)
        if ws is None:
            dev, off = self.flow_priors[0].flow.device, self._offsets
            u32 = torch.empty(n * int(off[-1]), dtype=torch.float32, device=dev)
            z = torch.empty(n * max(fp.dim for fp in self.flow_priors), dtype=torch.float32, device=dev)
            ws = (u32,
                  # block b's [n][Df_b] piece of u32, and the one z every flow writes in turn (not used)
                  [u32[n * int(off[b]):n * int(off[b + 1])].view(n, fp.dim) for b, fp in enumerate(self.flow_priors)],
                  [z[:n * fp.dim].view(n, fp.dim) for fp in self.flow_priors],
                  torch.empty(len(self.flow_priors), n, dtype=torch.float32, device=dev),      # the flows' log_prob
                  torch.empty(len(self.flow_priors), n, dtype=torch.float64, device=dev),      # the scalers' log-determinants
                  torch.empty(n, dtype=torch.float64, device=dev) if self._rdesc is not None else None,
                  torch.empty(n, dtype=torch.int32, device=dev))                     # inside the support (one flag per row)
            while len(self._ws) >= self._WORKSPACES:
                self._ws.pop(next(iter(self._ws)))
            self._ws[n] = ws
        return ws

    def _logpdf_device_blocks(self, x):
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        D, flow0 = self.dim, self.flow_priors[0].flow
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"JointPrior.logpdf_device: expected an (n, {D}) float64 tensor, got {what}")
        _on_device(x, flow0.device, "JointPrior.logpdf_device")
        n = x.shape[0]
        out = torch.empty(n, dtype=torch.float64, device=flow0.device)
        if n == 0:
            return out
        # the two layouts the kernel reads with coalesced loads; everything else is copied once
        if x.is_contiguous():
            strides = (D, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (D, 1)
        u32, u32_b, z_b, lp32, ldj, rest_logp, inside = self._workspace_blocks(n)
        lib = flow0.lib
        with torch.cuda.device(flow0.device):
            _lib.check(lib.pmc_joint_blocks_pre(C.byref(self._jdesc), C.c_void_p(x.data_ptr()), strides[0], strides[1], n,
                                                _lib.ptr(u32), _lib.ptr(ldj), _lib.ptr(rest_logp), _lib.ptr(inside),
                                                _lib.stream_handle()), "pmc_joint_blocks_pre")
            for b, fp in enumerate(self.flow_priors):
                fp.flow._forward_call(u32_b[b], z_b[b], None, lp32[b], n)
            _lib.check(lib.pmc_joint_blocks_post(len(self.flow_priors), _lib.ptr(lp32), _lib.ptr(ldj), _lib.ptr(rest_logp),
                                                 _lib.ptr(inside), _lib.ptr(out), n, _lib.stream_handle()),
                       "pmc_joint_blocks_post")
        return out

    def _step_stage_blocks(self, n, device):
        """``pmc_prior_blocks_stage_t`` for the ``n`` rows of one step engine: this prior's ``pmc_joint_blocks_t``, every
        block's flow (a bf16 block: its image) and one workspace set of its own, laid out as ``logpdf_device``'s.  The
        descriptor keeps what it points into alive, like ``pmc_prior_stage_t``'s."""
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device, _pinned_take
        n = int(n)
        if n < 1:
            raise ValueError(f"JointPrior.step_stage: n must be at least 1, got {n}")
        dev = torch.device(self.flow_priors[0].flow.device)
        if device is not None:
            _on_device(torch.empty(0, device=dev), device, "JointPrior.step_stage")
        with torch.cuda.device(dev):
            ws = dict(u32=torch.empty(n * int(self._offsets[-1]), dtype=torch.float32, device=dev),
                      z=torch.empty(n * max(fp.dim for fp in self.flow_priors), dtype=torch.float32, device=dev),
                      lp32=torch.empty(len(self.flow_priors), n, dtype=torch.float32, device=dev),
                      ldj=torch.empty(len(self.flow_priors), n, dtype=torch.float64, device=dev),
                      rest_logp=torch.empty(n, dtype=torch.float64, device=dev) if self._rdesc is not None else None,
                      inside=torch.empty(n, dtype=torch.int32, device=dev),
                      count=torch.zeros(2, dtype=torch.int64, device=dev))
            images = [fp.flow._bf16_image()[1:] if fp.flow.precision == "bf16" else None for fp in self.flow_priors]
        h_count = _pinned_take((2,), torch.int64)
        h_count.zero_()
        desc = _lib.pmc_prior_blocks_stage_t(
            u32=ws["u32"].data_ptr(), z=ws["z"].data_ptr(), lp32=ws["lp32"].data_ptr(), ldj=ws["ldj"].data_ptr(),
            rest_logp=ws["rest_logp"].data_ptr() if ws["rest_logp"] is not None else None, inside=ws["inside"].data_ptr(),
            count=ws["count"].data_ptr(), h_count=h_count.data_ptr())
        C.memmove(C.byref(desc.blocks), C.byref(self._jdesc), C.sizeof(_lib.pmc_joint_blocks_t))
        for b, fp in enumerate(self.flow_priors):
            desc.maf[b] = C.cast(C.pointer(fp.flow._desc), C.c_void_p)
            if images[b] is not None:
                desc.image16[b] = images[b][0].data_ptr()
                desc.image_per_transform[b] = int(images[b][1])
        desc._keep = (self, ws, images)
        desc.counts = h_count             # (the pinned words: the engine reads them, and recycles the tensor with its own)
        return desc

    def _rvs_blocks(self, size):
        x = np.empty((size, self.dim), dtype=np.float64)
        for cols, fp in zip(self._block_cols, self._parts):               # block 0, block 1, ..., then the rest
            x[:, cols] = fp.rvs(size)
        if self.rest is not None:
            glob = np.random.mtrand._rand                                 # (numpy's global generator, named: see rvs)
            x[:, self._rest_cols] = np.transpose([d.rvs(size=size, random_state=glob) for d in self.rest.dists])
        return x

    # ----------------------------------------------------------------- density
    def _workspace(self, n):
        import torch
        ws = self._ws.get(n)
        if ws is None:
            dev, Df = self.flow_prior.flow.device, self.flow_prior.dim
            ws = (torch.empty(n, Df, dtype=torch.float32, device=dev),           # u32
                  torch.empty(n, Df, dtype=torch.float32, device=dev),           # z (the flow writes it; not used)
                  torch.empty(n, dtype=torch.float32, device=dev),               # the flow's log_prob
                  torch.empty(n, dtype=torch.float64, device=dev),               # the scaler's log-determinant
                  torch.empty(n, dtype=torch.float64, device=dev),               # the table factors' sum
                  torch.empty(n, dtype=torch.int32, device=dev))                 # inside the support
            while len(self._ws) >= self._WORKSPACES:
                self._ws.pop(next(iter(self._ws)))
            self._ws[n] = ws
        return ws

    def _logpdf_device_gauss(self, x):
        """The blocks form with Gaussian blocks: the flow blocks' launches with the table as ``_logpdf_device_blocks`` makes
        them, then one ``pmc_gauss_blocks_logpdf`` launch that adds the Gaussian blocks in place; without a flow block that one
        launch alone, the table in it."""
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        D, dev = self.dim, self._device
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"JointPrior.logpdf_device: expected an (n, {D}) float64 tensor, got {what}")
        _on_device(x, dev, "JointPrior.logpdf_device")
        n = x.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.float64, device=dev)
        # the two layouts the kernels read with coalesced loads; everything else is copied once, for both
        if x.is_contiguous():
            strides = (D, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (D, 1)
        out = self._logpdf_device_blocks(x) if self.flow_priors else torch.empty(n, dtype=torch.float64, device=dev)
        base = _lib.ptr(out) if self.flow_priors else None
        with torch.cuda.device(dev):
            if self._gbox is not None:
                _lib.check(_lib.load().pmc_gauss_box_logpdf(C.byref(self._gdesc), C.byref(self._gbox), C.c_void_p(x.data_ptr()),
                                                            strides[0], strides[1], n, base, _lib.ptr(out),
                                                            _lib.stream_handle()), "pmc_gauss_box_logpdf")
            else:
                _lib.check(_lib.load().pmc_gauss_blocks_logpdf(C.byref(self._gdesc), C.c_void_p(x.data_ptr()), strides[0],
                                                               strides[1], n, base, _lib.ptr(out), _lib.stream_handle()),
                           "pmc_gauss_blocks_logpdf")
        return out

    def _logpdf_device_mix(self, x):
        """The blocks form with mixture blocks: the launches of the same prior without them (``_logpdf_device_gauss`` or
        ``_logpdf_device_blocks``), then one ``pmc_gauss_mix_logpdf`` launch per mixture block in list order, each adding its
        block in place; where nothing precedes, the first launch starts the value, with the table in it."""
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        D, dev = self.dim, self._device
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"JointPrior.logpdf_device: expected an (n, {D}) float64 tensor, got {what}")
        _on_device(x, dev, "JointPrior.logpdf_device")
        n = x.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.float64, device=dev)
        # the two layouts the kernels read with coalesced loads; everything else is copied once, for all of them
        if x.is_contiguous():
            strides = (D, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (D, 1)
        if self.gaussian_priors:
            out = self._logpdf_device_gauss(x)
        elif self.flow_priors:
            out = self._logpdf_device_blocks(x)
        else:
            out = None
        base = None if out is None else _lib.ptr(out)
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            for desc in self._mdescs:
                _lib.check(_lib.load().pmc_gauss_mix_logpdf(C.byref(desc), C.c_void_p(x.data_ptr()), strides[0], strides[1], n,
                                                            base, _lib.ptr(out), _lib.stream_handle()), "pmc_gauss_mix_logpdf")
                base = _lib.ptr(out)
        return out

    def _logpdf_device_kde(self, x):
        """The blocks form with KDE blocks: the launches of the same prior without them (``_logpdf_device_mix``,
        ``_logpdf_device_gauss`` or ``_logpdf_device_blocks``), then one ``pmc_kde_logpdf`` launch per KDE block in list
        order, each adding its block in place; where nothing precedes, the first launch starts the value, with the table in
        it."""
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        D, dev = self.dim, self._device
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"JointPrior.logpdf_device: expected an (n, {D}) float64 tensor, got {what}")
        _on_device(x, dev, "JointPrior.logpdf_device")
        n = x.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.float64, device=dev)
        # the two layouts the kernels read with coalesced loads; everything else is copied once, for all of them
        if x.is_contiguous():
            strides = (D, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (D, 1)
        if self.mixture_priors:
            out = self._logpdf_device_mix(x)
        elif self.gaussian_priors:
            out = self._logpdf_device_gauss(x)
        elif self.flow_priors:
            out = self._logpdf_device_blocks(x)
        else:
            out = None
        base = None if out is None else _lib.ptr(out)
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            for desc in self._kdescs:
                _lib.check(_lib.load().pmc_kde_logpdf(C.byref(desc), C.c_void_p(x.data_ptr()), strides[0], strides[1], n,
                                                      base, _lib.ptr(out), _lib.stream_handle()), "pmc_kde_logpdf")
                base = _lib.ptr(out)
        return out

    gaussian_priors = ()          # the owned copies of the Gaussian blocks, in list order (the blocks form)
    mixture_priors = ()           # the owned copies of the mixture blocks, in list order (the blocks form)
    kde_priors = ()               # the owned copies of the KDE blocks, in list order (the blocks form)

    def logpdf_device(self, x):
        if self.kde_priors:
            return self._logpdf_device_kde(x)
        if self.mixture_priors:
            return self._logpdf_device_mix(x)
        if self.gaussian_priors:
            return self._logpdf_device_gauss(x)
        if self.blocks:
            return self._logpdf_device_blocks(x)
        import ctypes as C
        import torch
        from . import _lib
        from .mcmc import _on_device
        D, flow = self.dim, self.flow_prior.flow
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != D:
            what = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"JointPrior.logpdf_device: expected an (n, {D}) float64 tensor, got {what}")
        _on_device(x, flow.device, "JointPrior.logpdf_device")
        n = x.shape[0]
        out = torch.empty(n, dtype=torch.float64, device=flow.device)
        if n == 0:
            return out
        # the two layouts the kernel reads with coalesced loads; everything else is copied once
        if x.is_contiguous():
            strides = (D, 1)
        elif x.t().is_contiguous():
            strides = (1, n)
        else:
            x, strides = x.contiguous(), (D, 1)
        u32, z, lp32, ldj, rest_logp, inside = self._workspace(n)
        lib = flow.lib
        with torch.cuda.device(flow.device):
            _lib.check(lib.pmc_joint_prior_pre(C.byref(self.flow_prior._sdesc), _lib.ptr(self._dev["flow_cols"]),
                                               C.byref(self._rdesc), _lib.ptr(self._dev["rest_cols"]),
                                               C.c_void_p(x.data_ptr()), strides[0], strides[1], n, _lib.ptr(u32),
                                               _lib.ptr(ldj), _lib.ptr(rest_logp), _lib.ptr(inside), _lib.stream_handle()),
                       "pmc_joint_prior_pre")
            flow._forward_call(u32, z, None, lp32, n)
            _lib.check(lib.pmc_joint_prior_post(_lib.ptr(lp32), _lib.ptr(ldj), _lib.ptr(rest_logp), _lib.ptr(inside),
                                                _lib.ptr(out), n, _lib.stream_handle()), "pmc_joint_prior_post")
        return out

    def logpdf(self, x):
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"JointPrior.logpdf: expected shape (n, {self.dim}), got {x.shape}")
        dev = self._device if self.blocks else self.flow_prior.flow.device
        return self.logpdf_device(torch.from_numpy(x).to(dev)).cpu().numpy()

    def step_stage(self, n, device=None):
        """``FlowPrior.step_stage`` for the joint prior: the descriptor carries the column maps and the table as well."""
        if self.kde_priors:
            raise ValueError("JointPrior.step_stage: a prior with a KDE block is not evaluated inside the step of a host "
                             "likelihood (step_prior); use logpdf, or device_prior=True with a device likelihood")
        if self.mixture_priors:
            raise ValueError("JointPrior.step_stage: a prior with a mixture block is not evaluated inside the step of a host "
                             "likelihood (step_prior); use logpdf, or device_prior=True with a device likelihood")
        if self.gaussian_priors:
            raise ValueError("JointPrior.step_stage: a prior with a Gaussian block is not evaluated inside the step of a host "
                             "likelihood (step_prior); use logpdf, or device_prior=True with a device likelihood")
        if self.blocks:
            return self._step_stage_blocks(n, device)
        return _step_stage(self, self.flow_prior, n, device,
                           joint=(self._dev["flow_cols"], self._rdesc, self._dev["rest_cols"]))

    # ----------------------------------------------------------------- draws
    def rvs(self, size=1):
        size = int(size)
        if self.blocks:
            return self._rvs_blocks(size)
        x = np.empty((size, self.dim), dtype=np.float64)
        x[:, self._flow_cols] = self.flow_prior.rvs(size)
        # rest.rvs with numpy's global generator named: this prior's copy of the factors (a deep copy, or an unpickled one)
        # carries a private copy of that generator's state, which np.random.seed -- the Sampler's random_state -- never reaches
        glob = np.random.mtrand._rand
        x[:, self._rest_cols] = np.transpose([d.rvs(size=size, random_state=glob) for d in self.rest.dists])
        return x

    @property
    def bounds(self):
        b = np.empty((self.dim, 2), dtype=np.float64)
        if self.blocks:
            for cols, fp in zip(self._block_cols, self._parts):
                b[cols] = fp.bounds
            if self.rest is not None:
                b[self._rest_cols] = self.rest.bounds
            return b
        b[self._flow_cols] = self.flow_prior.bounds
        b[self._rest_cols] = self.rest.bounds
        return b

    @property
    def dim(self):
        if self.blocks:
            return self._dim
        return self.flow_prior.dim + self.rest.dim
