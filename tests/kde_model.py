"""The statement of a row of ``csrc/kde_prior.hip`` (``pmc_kde_logpdf``, include/pocomc_amd.h), written once in numpy: float64,
every product and every sum a numpy operation of its own (numpy contracts nothing into an FMA), in the order the header fixes.

    d_j = x[cols[j]] - center_j
    y_i = ((0.0 + Linv[i,0] d_0) + Linv[i,1] d_1) + ...          (GaussianPrior's y, the same order)
    q_m = ((0.0 + (y_0 - t_m0)^2) + (y_1 - t_m1)^2) + ...        in j order
    e_m = -0.5 q_m + logw_m
    mx  = max_m e_m        (-inf: the row is -inf, no difference is formed)
    s   = sum_m exp(e_m - mx)                                    here: sequentially, m = 0, 1, ...
    v   = (mx + log s) - logc ;   logp[r] = start + v

The kernel's ``y_i`` and ``e_m`` are this statement's bits; its ``exp`` and ``log`` are the device library's and it adds the M
terms of ``s`` in eight slices, so the values agree to ``tolerance(M, v, logc)`` and not bit for bit -- except with one sample
and ``logw = 0.0``, where ``t_0 = 0``, ``exp(0) = 1`` and ``log(1) = 0`` are exact on both sides and the value is
``gauss_prior_model.gauss_block_model``'s.  The sample sets the KDE tests share are here too."""
import numpy as np


def whiten(xb, center, linv_packed):
    """``y`` ``(n, k)`` of the block's gathered columns ``xb`` ``(n, k)``."""
    xb = np.asarray(xb, dtype=np.float64)
    n, k = xb.shape
    assert len(center) == k and len(linv_packed) == k * (k + 1) // 2
    y = np.empty((n, k))
    with np.errstate(all="ignore"):
        d = [xb[:, j] - center[j] for j in range(k)]
        for i in range(k):
            row = linv_packed[i * (i + 1) // 2:]
            acc = np.zeros(n)
            for j in range(i + 1):
                acc = acc + row[j] * d[j]
            y[:, i] = acc
    return y


def kde_e_model(xb, center, linv_packed, t, logw):
    """``e`` ``(n, M)``: every kernel's ``-0.5 q_m + logw_m`` for every row."""
    y = whiten(xb, center, linv_packed)
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = np.zeros((len(y), len(t)))
        for j in range(y.shape[1]):
            df = y[:, j, None] - t[None, :, j]
            q = q + df * df
        return -0.5 * q + np.asarray(logw)[None, :]


def kde_model(xb, center, linv_packed, t, logw, logc, start=None, chunks=1):
    """``start + v`` of every row (``start=None``: ``v``); -inf for a row with an x that is not finite, with ``mx = -inf`` (an
    ``e_m`` that is NaN counts as -inf) or with a value that is not finite.  ``chunks``: the sum of the exps in that many
    contiguous slices of ``ceil(M / chunks)``, each in m order, the partial sums added in slice order (1: sequentially)."""
    xb = np.asarray(xb, dtype=np.float64)
    e = kde_e_model(xb, center, linv_packed, t, logw)
    e = np.where(np.isnan(e), -np.inf, e)
    mx = e.max(axis=1)
    dead = np.isneginf(mx)
    ref = np.where(dead, 0.0, mx)                                         # (no difference is formed for a dead row)
    M = e.shape[1]
    step = -(-M // chunks)
    with np.errstate(all="ignore"):
        terms = np.exp(e - ref[:, None])
        s = None
        for lo in range(0, M, step):
            part = np.add.accumulate(terms[:, lo:lo + step], axis=1)[:, -1]      # (accumulate adds in m order)
            s = part if s is None else s + part
        v = np.where(dead, -np.inf, (ref + np.log(s)) - logc)
        if start is not None:
            v = np.asarray(start, dtype=np.float64) + v
    bad = ~np.isfinite(xb).all(axis=1) | ~np.isfinite(v)
    return np.where(bad, -np.inf, v)


def block_model(prior, xb, start=None, chunks=1):
    """``kde_model`` on a ``KDEPrior``'s ``device_block()``."""
    blk = prior.device_block()
    return kde_model(xb, blk["center"], blk["linv_packed"], blk["t"], blk["logw"], float(blk["logc"]), start, chunks)


def tolerance(M, v, logc):
    """``(M + 8) 2^-52 + 2^-50 (|v| + |logc|)``, derived and not measured: the terms of ``s`` lie in (0, 1] and ``s >= 1``; a
    1-ulp ``exp`` on each side moves ``s`` by at most 2 * 2^-52 relative; any order of the M additions by at most
    (M - 1) 2^-53 on each side; a 1-ulp ``log`` and the two closing additions round on values of the size of ``|mx|``,
    ``|log s|`` and ``|logc|``."""
    return (M + 8) * 2.0 ** -52 + 2.0 ** -50 * (np.abs(v) + abs(float(logc)))


# ------------------------------------------------------------------------------------------------------------------
# sample sets
# ------------------------------------------------------------------------------------------------------------------
def banana(M, k, seed):
    """``(M, k)`` rows of a banana in the first two columns (the second bent by the first's square), further columns
    correlated normals of unequal widths."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(M, k))
    s = np.array(z)
    s[:, 0] = 2.0 * z[:, 0]
    if k > 1:
        s[:, 1] = 0.5 * z[:, 1] + 0.25 * s[:, 0] ** 2 - 1.0
    for j in range(2, k):
        s[:, j] = (0.3 + 0.2 * j) * z[:, j] + 0.4 * s[:, j - 1]
    return s


def bimodal(M, k, seed, at=70.0):
    """Two clusters 6 apart in every column, centred near ``at``: far from the origin, so that the centring matters."""
    rng = np.random.default_rng(seed)
    side = np.where(rng.random(M) < 0.35, -3.0, 3.0)
    return at + side[:, None] + rng.normal(size=(M, k)) * np.linspace(0.5, 1.5, k)


def log_weights(M, seed, wmin=1e-12):
    """Weights from 1 down to ``wmin``, log-spaced, in a random order."""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.logspace(0.0, np.log10(wmin), M)) if M > 1 else np.ones(1)


def scipy_kde(samples, weights, bandwidth):
    """``scipy.stats.gaussian_kde`` of the same samples (its ``dataset`` is ``(k, M)``)."""
    from scipy.stats import gaussian_kde
    return gaussian_kde(np.asarray(samples).T, bw_method=bandwidth, weights=weights)
