"""The arithmetic of ``csrc/gauss_mix_prior.hip`` (``pmc_gauss_mix_logpdf``, include/pocomc_amd.h), stated in numpy on top of
``gauss_prior_model.gauss_block_model``: float64, every product and every sum a numpy operation of its own in the order the
header fixes.

    g_c = gauss_block_model(x, mean_c, linv_c, logc_c)
    t_c = g_c + logw_c                          (-inf where g_c is NaN or -inf)
    m   = max_c t_c
    s   = ((0.0 + exp(t_0 - m)) + exp(t_1 - m)) + ...      in c order
    v   = m + log(s);   -inf where every t_c is -inf (the differences are never formed) or v is not finite

The kernel's ``t_c`` are this statement's bits; its ``exp`` and ``log`` are the device library's, numpy's are the host's, so
the two values agree to ``tolerance(C, v)`` and not bit for bit -- except with one component and ``logw = 0.0``, where
``exp(0) = 1`` and ``log(1) = 0`` are exact on both sides.  The fixtures the mixture tests share are here too."""
import numpy as np

import gauss_prior_model as gpm


def mix_t_model(xb, logw, mean, linv_packed, logc):
    """``t`` ``(C, n)``: every component's ``g_c + logw_c`` on the block's gathered columns ``xb`` ``(n, k)``."""
    xb = np.asarray(xb, dtype=np.float64)
    t = np.empty((len(logw), len(xb)))
    with np.errstate(all="ignore"):
        for c in range(len(logw)):
            g = gpm.gauss_block_model(xb, mean[c], linv_packed[c], float(logc[c]))      # (-inf for NaN and for bad rows)
            t[c] = np.where(np.isneginf(g), -np.inf, g + logw[c])
    return t


def gauss_mix_model(xb, logw, mean, linv_packed, logc, start=None):
    """``start + v`` of every row (``start=None``: ``v``); -inf where it is not finite."""
    t = mix_t_model(xb, logw, mean, linv_packed, logc)
    m = t[0].copy()
    for c in range(1, len(t)):
        m = np.where(t[c] > m, t[c], m)
    dead = np.isneginf(m)
    ms = np.where(dead, 0.0, m)                                           # (no difference is formed for a dead row)
    with np.errstate(all="ignore"):
        s = np.zeros(t.shape[1])
        for c in range(len(t)):
            s = s + np.exp(t[c] - ms)
        v = np.where(dead, -np.inf, ms + np.log(s))
        if start is not None:
            v = np.asarray(start, dtype=np.float64) + v
    return np.where(np.isfinite(v), v, -np.inf)


def block_model(prior, xb, start=None):
    """``gauss_mix_model`` on a ``GaussianMixturePrior``'s ``device_block()``."""
    blk = prior.device_block()
    return gauss_mix_model(xb, blk["logw"], blk["mean"], blk["linv_packed"], blk["logc"], start)


def tolerance(C, model):
    """``(C + 8) 2^-52 + 2^-52 |model|``: the ``t_c`` are the model's bits; a 1-ulp float64 ``exp`` moves each of the C terms,
    all at most 1, by 2^-52 at most, the C additions round once each, a 1-ulp ``log`` and the final sum once more on a value
    of the size of the result.  The header states the same bound."""
    return (C + 8) * 2.0 ** -52 + 2.0 ** -52 * np.abs(model)


# ------------------------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------------------------
def random_mixture(C, k, seed, spread=1.0, cond=100.0, wmin=1e-12):
    """``(weights, means, covs)``: C components in k dimensions whose means are ``spread`` apart in units of their widths
    (1: overlapping, 30: well separated), weights log-spaced from 1 down to ``wmin`` in a random order."""
    rng = np.random.default_rng(seed)
    means = rng.normal(size=(C, k)) * spread
    covs = np.stack([gpm.random_cov(k, cond, rng) * rng.uniform(0.5, 2.0) for _ in range(C)])
    weights = rng.permutation(np.logspace(0.0, np.log10(wmin), C)) if C > 1 else np.ones(1)
    return weights, means, covs


def mixture_draws(weights, means, covs, n, width, rng):
    """``n`` rows, each from a component chosen by ``rng`` uniformly (so that the light components have rows too), at
    ``width`` times its spread."""
    comp = rng.integers(len(weights), size=n)
    L = np.linalg.cholesky(covs)
    z = rng.normal(size=(n, means.shape[1]))
    return means[comp] + width * np.einsum("rj,rij->ri", z, L[comp])


def em_case(seed=3, n=4000):
    """The issue's EM case: two components in 3-D, means (-4, 0, 0) and (4, 1, -1), covariances ``A A^T + 0.5 I``, weights
    0.3 / 0.7.  ``(rows, weights, means, covs)``."""
    rng = np.random.default_rng(seed)
    weights = np.array([0.3, 0.7])
    means = np.array([[-4.0, 0.0, 0.0], [4.0, 1.0, -1.0]])
    covs = []
    for _ in range(2):
        A = rng.normal(size=(3, 3))
        covs.append(A @ A.T + 0.5 * np.eye(3))
    covs = np.stack(covs)
    comp = (rng.random(n) < weights[1]).astype(np.int64)
    L = np.linalg.cholesky(covs)
    x = means[comp] + np.einsum("rj,rij->ri", rng.normal(size=(n, 3)), L[comp])
    return x, weights, means, covs


def scipy_logpdf(x, weights, means, covs):
    """``logsumexp_c(log w_c + multivariate_normal(mean_c, cov_c).logpdf(x))``, the weights normalised."""
    from scipy.special import logsumexp
    from scipy.stats import multivariate_normal
    w = np.asarray(weights, dtype=np.float64)
    w = w / w.sum()
    parts = [np.log(w[c]) + np.atleast_1d(multivariate_normal(means[c], covs[c]).logpdf(x)) for c in range(len(w))]
    return logsumexp(np.stack(parts), axis=0)
