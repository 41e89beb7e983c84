"""Log-weight vectors in the regimes an SMC run produces, sizes on the kernels' own boundaries, references in exact or
extended arithmetic, and the criterion the bookkeeping kernels (``csrc/trim.hip``, ``csrc/pool.hip``, the tail of
``csrc/mcmc_kernels.hip``) are held to there (``tests/test_pool_regimes_cpu.py``, ``tests/test_gpu_pool_regimes.py``).

Why: every older test of these kernels feeds them log-weights that are a Gaussian of width 2-4.  A run also produces
exactly equal weights (beta = 0), nearly equal ones (a small beta step), spreads of hundreds of nats (most
``exp(logw - max)`` underflow to 0.0), a single survivor, ties (resampled duplicates) and holes (``logl = -inf``).

* reference: the quantity evaluated on the same float64 numbers in 50-digit arithmetic (``mpmath``) up to
  ``MP_MAX`` elements, in x87 extended precision (64-bit mantissa, error ~1e-19: three decades below float64's) above
  it; ``tests/test_pool_regimes_cpu.py`` pins the two against each other.  Trimming: the exact ESS ratio of every
  percentile bin from integer arithmetic on the float64 weights (``fractions.Fraction``).
* envelope: the largest deviation from that reference among ``N_PERTURB`` float64 evaluations of the ORACLE on the same
  numbers in permuted particle order -- a reordering is exactly what a parallel reduction does to a sum;
* criterion for a device value: ``err <= max(bound, C * envelope)``; ``bound`` is the one ``tests/test_gpu_tools.py``
  already uses for that quantity, ``C`` the constant of ``tests/flow_regimes.py``.
* knife edge of a trim case: some bin's exact ratio ``r_i`` lies within ``C * max(envelope of r_i, k_i)`` of ``ess``,
  ``k_i = (tot1 / s1_i + tot2 / s2_i) * ceil(log2 P) * 2^-53`` being the rounding a suffix sum formed as total minus
  prefix can carry relative to itself (``trim_search_kernel``: a scan's prefix is off by about ``log2 P`` roundings of
  the TOTAL, which the subtraction turns into ``tot / s`` roundings of the suffix).  There the summation order decides
  the bin, and no implementation can promise the reference's.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

from oracle import tools as otools

C = 16.0                     # tests/flow_regimes.py
N_PERTURB = 8
MP_MAX = 4097                # 50-digit arithmetic up to here, extended precision above
U = 2.0 ** -53
ONE_BELOW = 1.0 - 2.0 ** -53

# tests/test_gpu_tools.py: ESS / logZ / logw rtol 1e-12, USS 1e-11, sums 1e-13, scatter matrix 1e-10
BOUND = {"ess": 1e-12, "logz": 1e-12, "logw": 1e-12, "uss": 1e-11, "sum": 1e-13, "scatter": 1e-10, "mean": 1e-12}

REGIMES = ("equal", "near_equal", "gauss", "wide", "very_wide", "holes", "one_hot", "ties", "shifted_up", "shifted_down")
# 256-thread blocks, the 4096-element chunk of serial_cumsum_kernel, the grid caps of the reductions (256 blocks in
# pmc_logw_stats, 1024 / 2048 in the element-wise kernels)
# (2048 * 256 + 1 was dropped from the top of this list and USS stops at 1e5 to keep the GPU file under a tenth of
#  the suite's run time, profiles/pool_regimes.md)
SIZES = (1, 2, 3, 17, 255, 256, 257, 1000, 4095, 4096, 4097, 8193, 65537, 100_000, 2048 * 256 - 1)
USS_SIZES = SIZES[:-1]
SORT_SIZES = (1, 2, 3, 17, 100, 255, 256, 257, 1000, 4095, 4096, 4097, 8193, 100_000, 500_000)   # sorts and scans
RESAMPLE_SIZES = (1, 2, 4095, 4096, 4097, 8192, 8193, 100_000)
NO_KNIFE_EDGE = ("gauss", "wide", "very_wide", "holes", "ties", "one_hot", "equal")
HISTORY_T = (1, 2, 9, 40)


def logw(regime, P, seed=0):
    """The log-weight vector of ``regime`` at length ``P`` (fixed seed)."""
    rng = np.random.default_rng([seed, P, REGIMES.index(regime)])
    z = rng.normal(size=P)
    if regime == "equal":
        return np.zeros(P)
    if regime == "near_equal":
        return 1e-9 * z
    if regime == "gauss":
        return 2.5 * z
    if regime == "wide":
        return 30.0 * z
    if regime == "very_wide":
        return 300.0 * z
    if regime == "holes":
        v = 2.5 * z
        v[rng.choice(P, P // 10, replace=False)] = -np.inf
        return v
    if regime == "one_hot":
        v = np.full(P, -np.inf)
        v[rng.integers(P)] = 0.0
        return v
    if regime == "ties":
        return np.round(2.0 * z)
    if regime == "shifted_up":
        return 2.5 * z + 700.0
    if regime == "shifted_down":
        return 2.5 * z - 700.0
    raise KeyError(regime)


def weights(regime, P, seed=0):
    """``exp(logw - max)`` of the regime, unnormalised like the Sampler's (sampler.py:779-781 before the division)."""
    lw = logw(regime, P, seed)
    return np.exp(lw - lw.max())


def history(T, N, width, seed=0, holes=False):
    """A persistent-sampling history for ``pmc_logw``: ``logl (T, N)`` of the given width, ``beta[0] = 0`` ascending,
    ``logz`` a random walk."""
    rng = np.random.default_rng([seed, T, N, int(width)])
    logl = rng.normal(size=(T, N)) * width - 30.0
    if holes:
        logl.reshape(-1)[rng.choice(T * N, max(T * N // 10, 1), replace=False)] = -np.inf
    beta = np.sort(rng.uniform(0, 1, size=T))
    beta[0] = 0.0
    logz = np.cumsum(rng.normal(size=T))
    return logl, beta, logz


@functools.lru_cache(maxsize=4)
def permutations(n, seed=0):
    rng = np.random.default_rng([seed, n, 77])
    return [rng.permutation(n) for _ in range(N_PERTURB)]


# ------------------------------------------------------------------------------------------------ exact statistics
def _mpf(x):
    """An extended-precision number as a 50-digit one (exactly)."""
    hi = float(x)
    with mpmath.workdps(50):
        return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))


def _sums_mp(lw):
    mx = max(lw)
    s1 = s2 = mpmath.mpf(0)
    m = mpmath.mpf(float(mx))
    for v in lw:
        d = mpmath.mpf(float(v)) - m
        if d > -300:                       # below: less than 1e-130 of the sum (which is >= 1), far past 50 digits
            s1 += mpmath.exp(d)
            s2 += mpmath.exp(2 * d)
    return s1, s2


def _sums_ld(lw):
    assert np.finfo(np.longdouble).eps < 2e-19, "needs a 64-bit mantissa long double (x86)"
    d = lw.astype(np.longdouble) - np.longdouble(lw.max())
    e = np.sort(np.exp(d[d > -300]))
    return _mpf(np.sum(e)), _mpf(np.sum(e * e))


def exact_stats(lw, force=None):
    """``max, s1 = sum exp(logw - max), s2 = sum exp(2 (logw - max))`` and what the run derives from them
    (``ess = s1^2 / s2``, ``compute_ess = ess / P``, ``logz = max + log s1``) as 50-digit numbers."""
    with mpmath.workdps(50):
        mx = float(np.max(lw))
        s1, s2 = (_sums_mp if (force or ("mp" if len(lw) <= MP_MAX else "ld")) == "mp" else _sums_ld)(lw)
        ess = s1 * s1 / s2
        return {"max": mx, "s1": s1, "s2": s2, "ess": ess, "compute_ess": ess / len(lw),
                "logz": mpmath.mpf(mx) + mpmath.log(s1)}


def oracle_stats(lw):
    """The same quantities as the float64 oracle computes them (``oracle/tools.py``)."""
    w = np.exp(lw - np.max(lw))
    return {"s1": np.sum(w), "s2": np.sum(w * w), "ess": otools.effective_sample_size(w.copy()),
            "compute_ess": otools.compute_ess(lw), "logz": otools.increment_logz(lw)}


def err(got, exact):
    """|got - exact| as a float (exact: 50-digit number or float)."""
    with mpmath.workdps(50):
        return float(abs(mpmath.mpf(float(got)) - exact))


def stats_envelope(lw, exact, seed=0):
    """Per quantity: the largest deviation of the oracle from ``exact`` over ``N_PERTURB`` particle orders."""
    env = dict.fromkeys(("s1", "s2", "ess", "compute_ess", "logz"), 0.0)
    for p in permutations(len(lw), seed):
        o = oracle_stats(lw[p])
        for k in env:
            env[k] = max(env[k], err(o[k], exact[k]))
    return env


STAT_BOUND = {"s1": "sum", "s2": "sum", "ess": "ess", "compute_ess": "ess", "logz": "logz"}


def allowed(quantity, exact, envelope):
    """``max(bound, C * envelope)`` of the criterion; ``bound`` is relative to the exact value like the ``rtol`` of
    ``tests/test_gpu_tools.py`` (log quantities: ``rtol`` and ``atol`` both, as ``test_logw_logz`` has them)."""
    scale = abs(float(exact))
    if quantity in ("logz", "logw"):
        scale += 1.0
    return max(BOUND[quantity] * scale, C * envelope)


@functools.lru_cache(maxsize=None)
def stats_case(regime, P):
    """(logw, exact statistics, envelope) of one regime x size; cached: every test of the case shares it."""
    lw = logw(regime, P)
    ex = exact_stats(lw)
    return lw, ex, stats_envelope(lw, ex)


def uss_reference(w, k, seed=0):
    """``unique_sample_size`` as the reference DEFINES it in float64 (``sum 1 - (1 - w)^k``: ``1 - w`` rounds to 1 below
    2^-53 in the reference too), its envelope over particle orders, and the exact value (reported only)."""
    ref = float(otools.unique_sample_size(w.copy(), k))
    env = max(abs(float(otools.unique_sample_size(w[p].copy(), k)) - ref) for p in permutations(len(w), seed))
    wl = w.astype(np.longdouble) / np.sum(np.sort(w).astype(np.longdouble))
    exact = float(np.sum(np.sort(-np.expm1(np.longdouble(k) * np.log1p(-wl[wl < 1])))) + np.count_nonzero(wl >= 1))
    return ref, env, exact


# -------------------------------------------------------------------------------- mixture log-weights (pmc_logw)
def exact_mixture(logl, beta, logz, beta_final):
    """``particles.py:215-231`` without the normalisation, in extended precision: ``logl beta_final - (log sum_t
    exp(logl beta_t - logz_t) - log T)`` per element (flattened), NaN where ``logl = -inf`` (``-inf * beta[0]``)."""
    L = np.asarray(logl, np.longdouble)
    with np.errstate(invalid="ignore"):
        b = L[None] * np.asarray(beta, np.longdouble)[:, None, None] - np.asarray(logz, np.longdouble)[:, None, None]
        m = b.max(axis=0)
        B = m + np.log(np.sum(np.exp(b - m), axis=0)) - np.log(np.longdouble(len(beta)))
        return (L * np.longdouble(beta_final) - B).reshape(-1)


def mixture_mp(l, beta, logz, beta_final):
    """One element of :func:`exact_mixture` in 50-digit arithmetic."""
    with mpmath.workdps(50):
        t = [mpmath.mpf(float(l)) * mpmath.mpf(float(b)) - mpmath.mpf(float(z)) for b, z in zip(beta, logz)]
        m = max(t)
        B = m + mpmath.log(mpmath.fsum(mpmath.exp(v - m) for v in t)) - mpmath.log(len(beta))
        return mpmath.mpf(float(l)) * mpmath.mpf(float(beta_final)) - B


def mixture_envelope(logl, beta, logz, beta_final, exact, seed=0):
    """Element-wise: the oracle with the history's iterations in ``N_PERTURB`` orders (the order of its logaddexp)."""
    T = len(beta)
    rng = np.random.default_rng([seed, T, 5])
    env = np.zeros(exact.shape)
    for _ in range(N_PERTURB):
        p = rng.permutation(T)
        # (beta and logz move together: every particle's log-weight is the same number, its terms added in another order)
        with np.errstate(invalid="ignore"):
            lw, _ = otools.compute_logw_and_logz(logl, beta[p], logz[p], beta_final, normalize=False)
        with np.errstate(invalid="ignore"):
            env = np.fmax(env, np.abs((lw.astype(np.longdouble) - exact).astype(np.float64)))
    return env


# --------------------------------------------------------------------------------------------------------- trimming
def _exact_ints(a):
    """float64 array -> Python integers ``a * 2^1074`` (exact: every finite double is a multiple of 2^-1074)."""
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64).astype(object)
    sh = (e.astype(np.int64) - 53 + 1074).astype(object)
    return np.array([x << s if s >= 0 else x >> -s for x, s in zip(mi, sh)], dtype=object)


def percentile_levels(bins):
    return np.linspace(0, 99, bins)


def trim_exact(w, ess=0.99, bins=1000, near=1e-6, seed=0):
    """The trim decision of ``pocomc/tools.py:10-53`` on normalised float64 weights ``w`` in exact arithmetic.

    Returns a dict: ``thr[i]`` the float64 threshold ``np.percentile`` returns for bin i, ``delta[i]`` the ESS ratio of the
    set ``w >= thr[i]`` minus ``ess`` (within ``near`` of 0 from integer arithmetic, exact to 2^-80; farther away from
    extended precision, good to 1e-11), ``bin`` the highest bin
    with ``ratio >= ess`` (what the reference's downward scan accepts in exact arithmetic), ``band[i]`` the knife-edge
    half-width of the bins within ``near`` of ``ess`` (the others are 1e4 bands away: ``k_i <= 200 * 20 * 2^-53``
    because the top percent of the particles holds at least a percent of either sum), ``knife`` the bins inside
    their band, and ``valid`` the bins an implementation may stop at: the highest bin that is acceptable beyond its
    band, and every knife-edge bin above it."""
    P = len(w)
    pct = percentile_levels(bins)
    thr = np.percentile(w, pct)
    srt = np.sort(w)
    cut = np.searchsorted(srt, thr, side="left")                 # kept: srt[cut:]
    # every bin in extended precision first: a sequential 64-bit-mantissa sum of P terms is off by at most P * 2^-64
    # of the total, so a ratio by at most 4 * 100 * P * 2^-64 < 1e-11 for P <= 5e5 -- bins farther than ``near`` from
    # ``ess`` are decided; the others are redone in integers below
    L = srt.astype(np.longdouble)
    l1, l2 = np.concatenate([[0], np.cumsum(L)]), np.concatenate([[0], np.cumsum(L * L)])
    q1, q2 = l1[-1] - l1[cut], l2[-1] - l2[cut]
    delta = ((q1 * q1 / q2) / (l1[-1] * l1[-1] / l2[-1]) - np.longdouble(float(ess))).astype(np.float64)
    accept = delta >= 0
    close = np.nonzero(np.abs(delta) <= near)[0]
    ess_f = Fraction(float(ess))
    en, ed = ess_f.numerator, ess_f.denominator
    if close.size:
        ints = _exact_ints(srt)
        c1 = np.concatenate([[0], np.cumsum(ints)])              # Python integers: exact
        c2 = np.concatenate([[0], np.cumsum(ints * ints)])
        tot1, tot2 = c1[-1], c2[-1]
    for i in close:                                              # delta[i] = ratio_i - ess, exact to 2^-80
        s1, s2 = tot1 - c1[cut[i]], tot2 - c2[cut[i]]
        num, den = s1 * s1 * tot2, s2 * tot1 * tot1             # ratio_i = num / den
        diff = num * ed - en * den
        accept[i] = diff >= 0
        delta[i] = float((diff << 80) // (den * ed)) / 2.0 ** 80
    band, knife = {}, []
    perms = None
    for i in close:
        i = int(i)
        s1, s2 = tot1 - c1[cut[i]], tot2 - c2[cut[i]]
        ratio = Fraction(s1 * s1 * tot2, s2 * tot1 * tot1)
        k = (float(Fraction(tot1, s1)) + float(Fraction(tot2, s2))) * math.ceil(math.log2(max(P, 2))) * U
        perms = perms if perms is not None else permutations(P, seed)
        env = 0.0
        for p in perms:
            wp = w[p]
            kept = wp[wp >= thr[i]]
            kept = kept / np.sum(kept)
            r = (1.0 / np.sum(kept ** 2.0)) / (1.0 / np.sum(wp ** 2.0))
            env = max(env, abs(float(Fraction(r) - ratio)))
        band[i] = C * max(env, k)
        if abs(delta[i]) <= band[i]:
            knife.append(i)
    sure = [i for i in range(bins) if accept[i] and i not in knife]
    floor = max(sure) if sure else 0                             # (the reference's scan always stops at bin 0)
    return {"thr": thr, "cut": cut, "delta": delta, "accept": accept, "bin": int(np.max(np.nonzero(accept)[0])) if accept.any() else 0,
            "band": band, "knife": knife, "valid": [floor] + [i for i in knife if i > floor]}


def oracle_trim_bin(w, ess=0.99, bins=1000):
    """The bin at which the loop of ``oracle.tools.trim_weights`` stops (its own statements, the index returned)."""
    w = w / np.sum(w)
    ess_total = 1.0 / np.sum(w ** 2.0)
    percentiles = np.linspace(0, 99, bins)
    i = bins - 1
    while True:
        threshold = np.percentile(w, percentiles[i])
        wt = w[w >= threshold]
        wt /= np.sum(wt)
        if (1.0 / np.sum(wt ** 2.0)) / ess_total >= ess:
            return i
        i -= 1


# ------------------------------------------------------------------------------------------------------- resampling
def systematic_reference(size, w, offset):
    """``oracle.tools.systematic_resample`` without its Python loop: its running sum IS ``np.cumsum`` (sequential), its
    ``while positions[i] > cumulative_sum`` the first j with ``cdf[j] >= position``.  Returns ``(idx, overrun)``:
    where a position lies above the last cdf entry the oracle raises IndexError; ``idx`` holds ``len(w)`` there."""
    if abs(np.sum(w) - 1.) > otools.SQRTEPS:
        w = np.array(w) / np.sum(w)
    cdf = np.cumsum(w)
    pos = (offset + np.arange(size)) / size
    idx = np.searchsorted(cdf, pos, side="left")
    return idx, idx >= len(w)


# ---------------------------------------------------------------------------------------------------------- moments
def exact_moments(x, w=None):
    """Weighted mean and scatter matrix ``sum w (x - mean)(x - mean)^T`` of float rows in extended precision."""
    X = np.asarray(x).astype(np.longdouble)
    W = np.ones(len(X), np.longdouble) if w is None else np.asarray(w).astype(np.longdouble)
    v1 = np.sum(W)
    mean = (W[:, None] * X).sum(axis=0) / v1
    c = X - mean
    S = np.einsum("ri,rj->ij", c * W[:, None], c)
    return mean, S, v1, np.sum(W * W)


def oracle_moments(x, w=None):
    """numpy's own route (``np.average`` / the centred product of ``np.cov``) in float64."""
    x64 = np.asarray(x, np.float64)
    w = np.ones(len(x64)) if w is None else w
    mean = np.average(x64, axis=0, weights=w)
    c = x64 - mean
    return mean, (c * w[:, None]).T @ c


def moments_envelope(x, w, exact_mean, exact_S, seed=0):
    em = es = 0.0
    for p in permutations(len(x), seed):
        m, S = oracle_moments(x[p], None if w is None else w[p])
        em = np.maximum(em, np.abs((m - exact_mean).astype(np.float64)))
        es = np.maximum(es, np.abs((S - exact_S).astype(np.float64)))
    return em, es


# --------------------------------------------------------------------------------------------------------- bootstrap
def exact_bootstrap(lw, draws):
    """``logsumexp(logw[draws[b]]) - log n`` per replicate, 50-digit; ``-inf`` where every draw is ``-inf``."""
    out = []
    with mpmath.workdps(50):
        for d in draws:
            v = lw[d]
            if np.isneginf(v).all():
                out.append(-mpmath.inf)
                continue
            m = mpmath.mpf(float(v.max()))
            s = mpmath.fsum(mpmath.exp(mpmath.mpf(float(t)) - m) for t in v if t - v.max() > -300)
            out.append(m + mpmath.log(s) - mpmath.log(len(v)))
    return out
