"""The flow prior restated in numpy (test infrastructure): the density ``pocomc_amd.FlowPrior`` evaluates on the device,

    ``log p(x) = flow.log_prob(u(x)) - log|dx/du|``,   ``u = scaler.forward(x)``,

from the oracle's parts -- ``oracle.scaler.Reparameterize.forward`` (float64), the log-determinant its ``inverse`` returns for
that ``u``, ``OracleMAF.log_prob`` on ``u`` rounded to float32 (what the flow kernels are given) -- with -inf for rows outside
the support: a NaN or an inf among the ``x_j``, a bounded ``x_j`` on or beyond a bound, a ``u_j`` that is not finite."""
import numpy as np

from oracle.scaler import Reparameterize


def oracle_scaler(bounds, transform, fit_rows=None):
    """The oracle's diagonal scaler on ``bounds`` (``(D, 2)``, +-inf: unbounded on that side), fitted on ``fit_rows``."""
    bounds = np.asarray(bounds, dtype=np.float64)
    s = Reparameterize(len(bounds), bounds=bounds, transform=transform)
    if fit_rows is not None:
        s.fit(np.asarray(fit_rows, dtype=np.float64))
    return s


def support(scaler, x):
    """Rows whose every ``x_j`` is finite and strictly inside the bounds."""
    lo = np.where(np.isfinite(scaler.low), scaler.low, -np.inf)
    hi = np.where(np.isfinite(scaler.high), scaler.high, np.inf)
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(x) & (x > lo) & (x < hi), axis=1)


def flow_prior_model(scaler, maf, x):
    """``(logp, ldj, inside)`` of the rows of ``x`` (float64 ``(n, D)``): ``logp`` float64 with -inf outside the support and
    wherever the value is not finite, ``ldj`` the scaler's log-determinant (NaN outside), ``inside`` the support mask."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    logp = np.full(n, -np.inf)
    ldj = np.full(n, np.nan)
    inside = support(scaler, x)
    if inside.any():
        with np.errstate(all="ignore"):
            u = scaler.forward(x[inside], check_input=False)
            ok = np.isfinite(u.astype(np.float32)).all(axis=1)
            u = u[ok]
            l = scaler.inverse(u)[1]
            v = maf.log_prob(u.astype(np.float32)).astype(np.float64) - l
        rows = np.flatnonzero(inside)[ok]
        inside = np.zeros(n, dtype=bool)
        inside[rows] = True
        ldj[rows] = l
        logp[rows] = np.where(np.isfinite(v), v, -np.inf)
    return logp, ldj, inside


# ---------------------------------------------------------------------------------------------------------------------
# the normalisation problem shared by the CPU and the GPU test: D = 2, a scaler fitted on beta(2, 3) draws
# ---------------------------------------------------------------------------------------------------------------------
NORM_BOUNDS = np.array([[-1.0, 2.0], [0.0, 5.0]])
NORM_GRID = 600
NORM_BOUND = 5e-3


def norm_fit_rows():
    rng = np.random.default_rng(0)
    return NORM_BOUNDS[:, 0] + (NORM_BOUNDS[:, 1] - NORM_BOUNDS[:, 0]) * rng.beta(2.0, 3.0, size=(500, 2))


def norm_grid():
    """Midpoints of a NORM_GRID x NORM_GRID grid on the box, ``(rows (G * G, 2), cell area)``."""
    w = NORM_BOUNDS[:, 1] - NORM_BOUNDS[:, 0]
    mid = (np.arange(NORM_GRID) + 0.5) / NORM_GRID
    a, b = np.meshgrid(NORM_BOUNDS[0, 0] + w[0] * mid, NORM_BOUNDS[1, 0] + w[1] * mid, indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1), float(w[0] * w[1]) / NORM_GRID ** 2


def integral(logp, cell):
    return float(np.exp(logp).sum() * cell)
