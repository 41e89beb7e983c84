"""The SMC bookkeeping kernels (``pmc_logw``, ``pmc_logw_stats``, ``pmc_weights_from_logw``, ``pmc_trim_threshold``,
``pmc_trim_select``, ``pmc_sum_f64``, ``pmc_resample_*``, ``pmc_moments``, ``pmc_column_medians``,
``pmc_bootstrap_logz_replay``) in the weight regimes a run produces and at sizes on their own boundaries, against the
exact references and the criterion of ``tests/pool_regimes.py`` (pinned without a GPU by
``tests/test_pool_regimes_cpu.py``).  ``-s`` prints, per quantity and regime, the largest ``err / envelope`` of the device
next to the float64 oracle's, and the knife-edge trim cases with both bins."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import pool_regimes as pr
from oracle import tools as otools

pytestmark = pytest.mark.gpu

MEASURED = {}          # (quantity, regime) -> [largest err / envelope on the device, same for the float64 oracle]
KNIFE = []


def note(quantity, regime, e_dev, e_or, env, scale):
    floor = max(env, 2.0 ** -53 * scale, np.finfo(float).tiny)       # an envelope of 0 (exact sums): one rounding
    m = MEASURED.setdefault((quantity, regime), [0.0, 0.0])
    m[0], m[1] = max(m[0], e_dev / floor), max(m[1], e_or / floor)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nquantity regime: largest err/envelope, device | float64 oracle")
    for (q, r), (d, o) in sorted(MEASURED.items()):
        print(f"  {q:12s} {r:13s} {d:10.3g} | {o:10.3g}")
    print("knife-edge trim cases (regime, P, ess, bins): device bin | oracle bin | bins on the edge")
    for c in KNIFE:
        print("  ", c)


def up(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def dev_stats(lw, k=0):
    from pocomc_amd import tools
    with np.errstate(invalid="ignore"):
        return tools.logw_stats(up(lw), k)


def dev_weights(lw):
    """``pmc_logw_stats`` + ``pmc_weights_from_logw`` as ``Particles.select`` chains them."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    d = up(lw)
    P = d.numel()
    st = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.pmc_reduce_workspace_bytes(P)), dtype=torch.uint8, device="cuda")
    w = torch.empty(P, dtype=torch.float64, device="cuda")
    _lib.check(lib.pmc_logw_stats(_lib.ptr(d), P, 0, _lib.ptr(st), _lib.ptr(ws), _lib.stream_handle()))
    _lib.check(lib.pmc_weights_from_logw(_lib.ptr(d), P, _lib.ptr(st), _lib.ptr(w), _lib.stream_handle()))
    return w.cpu().numpy()


def dev_trim(w, ess, bins):
    """``pmc_trim_threshold`` + ``pmc_trim_select``: (threshold, bin, kept indices, renormalised weights)."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    wd = up(w)
    P = wd.numel()
    nb1, nb2 = int(lib.pmc_trim_workspace_bytes(P)), int(lib.pmc_trim_select_workspace_bytes(P))
    ws = torch.empty(max(nb1, nb2), dtype=torch.uint8, device="cuda")
    res = torch.zeros(2, dtype=torch.float64, device="cuda")
    idx = torch.full((P,), -1, dtype=torch.int64, device="cuda")
    wt = torch.zeros(P, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = _lib.stream_handle()
    _lib.check(lib.pmc_trim_threshold(_lib.ptr(wd), P, float(ess), int(bins), _lib.ptr(res), _lib.ptr(ws), nb1, st))
    _lib.check(lib.pmc_trim_select(_lib.ptr(wd), P, _lib.ptr(res), _lib.ptr(idx), _lib.ptr(wt), _lib.ptr(cnt), _lib.ptr(ws), nb2, st))
    r, m = res.cpu().numpy(), int(cnt.item())
    return float(r[0]), int(r[1]), idx.cpu().numpy()[:m], wt.cpu().numpy()[:m]


# ------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_statistics(regime):
    """max, sum w, sum w^2, ESS, compute_ess, increment_logz through every public entry point, the normalised
    weights of ``pmc_weights_from_logw`` and the ordered sum ``pmc_sum_f64``."""
    from pocomc_amd import tools
    for P in pr.SIZES:
        lw, ex, env = pr.stats_case(regime, P)
        with np.errstate(invalid="ignore"):
            o = pr.oracle_stats(lw)
        st = dev_stats(lw)
        assert st[0] == ex["max"]
        w = np.exp(lw - lw.max())
        with np.errstate(invalid="ignore"):
            got = {"s1": [st[1]], "s2": [st[2]], "ess": [st[1] * st[1] / st[2], tools.effective_sample_size(w.copy())],
                   "compute_ess": [tools.compute_ess(lw)], "logz": [tools.increment_logz(lw)]}
        for k, q in pr.STAT_BOUND.items():
            for g in got[k]:
                e = pr.err(g, ex[k])
                note(k, regime, e, pr.err(o[k], ex[k]), env[k], abs(float(ex[k])))
                assert e <= pr.allowed(q, ex[k], env[k]), (regime, P, k, g, float(ex[k]), e, env[k])
        if regime == "one_hot":
            assert got["ess"] == [1.0, 1.0] and got["logz"] == [0.0] and got["compute_ess"] == [1.0 / P]
        if regime == "equal":
            assert st[1] == P == st[2]
        # normalised weights: -inf gives exactly 0.0, never NaN; they sum to 1
        wn = dev_weights(lw)
        assert not np.isnan(wn).any() and (wn[np.isneginf(lw)] == 0.0).all() and (wn >= 0).all()
        s_env = max(abs(float(np.sum(wn[p])) - math.fsum(wn)) for p in pr.permutations(P))
        assert abs(math.fsum(wn) - 1.0) <= max(pr.BOUND["sum"], pr.C * s_env), (regime, P, math.fsum(wn))
        np.testing.assert_allclose(wn, w / float(ex["s1"]), rtol=1e-12, atol=0)
        # pmc_sum_f64 (the ordered sum the resamplers normalise by)
        e = abs(tools.device_sum(up(wn)) - math.fsum(wn))
        note("sum_f64", regime, e, abs(float(np.sum(wn)) - math.fsum(wn)), s_env, 1.0)
        assert e <= max(pr.BOUND["sum"], pr.C * s_env), (regime, P, e, s_env)
    # one element past the 2048-block grid cap of weights_kernel (the exact statistics stop below it, pool_regimes.SIZES)
    lw = pr.logw(regime, 2048 * 256 + 1)
    w, wn = np.exp(lw - lw.max()), dev_weights(lw)
    assert (wn[np.isneginf(lw)] == 0.0).all() and abs(math.fsum(wn) - 1.0) <= pr.BOUND["sum"]
    np.testing.assert_allclose(wn, w / math.fsum(w), rtol=1e-12, atol=0)


@pytest.mark.parametrize("regime", pr.REGIMES)
def test_unique_sample_size(regime):
    """USS as the reference defines it in float64 (``sum 1 - (1 - w)^k``), k in {1, 64, P, 10 P}."""
    from pocomc_amd import tools
    for P in pr.USS_SIZES:
        w = pr.weights(regime, P)
        for k in (1, 64, P, 10 * P):
            ref, env, exact = pr.uss_reference(w, k)
            got = tools.unique_sample_size(w.copy(), k)
            note("uss", regime, abs(got - ref), abs(ref - exact), env, abs(ref))
            assert abs(got - ref) <= max(pr.BOUND["uss"] * abs(ref), pr.C * env), (regime, P, k, got, ref, exact, env)


def test_statistics_of_degenerate_vectors():
    """All ``-inf``: the oracle's max is ``-inf`` and everything derived from it NaN; so is the device's.  A NaN entry:
    ``np.max`` propagates it, the kernel's ``fmax`` does not -- ``stats[0]`` is the largest non-NaN entry -- but every sum
    is NaN, so ESS and logZ are NaN like the oracle's."""
    from pocomc_amd import tools
    for P in (1, 257, 70_000):
        lw = np.full(P, -np.inf)
        st = dev_stats(lw)
        with np.errstate(invalid="ignore"):
            assert st[0] == np.max(lw) == -np.inf and np.isnan(otools.increment_logz(lw)) and np.isnan(otools.compute_ess(lw))
            assert np.isnan(st[1]) and np.isnan(st[2]) and np.isnan(tools.increment_logz(lw)) and np.isnan(tools.compute_ess(lw))
        lw = pr.logw("gauss", P)
        lw[P // 2] = np.nan
        st = dev_stats(lw)
        assert np.isnan(otools.increment_logz(lw)) and np.isnan(otools.compute_ess(lw))
        assert st[0] == (np.nanmax(lw) if P > 1 else -np.inf) and np.isnan(st[1]) and np.isnan(st[2])
        assert np.isnan(tools.increment_logz(lw)) and np.isnan(tools.compute_ess(lw))
        assert np.isnan(dev_weights(lw)).all()                       # as exp(logw - nan) / nan is in the reference


# --------------------------------------------------------------------------------------------------------- pmc_logw
@pytest.mark.parametrize("T", pr.HISTORY_T)
@pytest.mark.parametrize("width", [4, 300])
def test_mixture_log_weights(T, width):
    """``pmc_logw`` (``particles.py:215-231``) against the extended-precision mixture, through ``compute_logw_and_logz``,
    ``PoolWeights`` and ``Particles.logw_stats``; rows with ``logl = -inf`` carry the oracle's NaN."""
    from pocomc_amd import tools
    from pocomc_amd.particles import Particles
    for N in (1, 300):
        for holes in (False, True):
            logl, beta, logz = pr.history(T, N, width, holes=holes)
            pool = tools.PoolWeights(logl, beta, logz)
            for bf in (0.0, 0.41, 1.0):
                ex = pr.exact_mixture(logl, beta, logz, bf)
                with np.errstate(invalid="ignore"):
                    olw, _ = otools.compute_logw_and_logz(logl, beta, logz, bf, normalize=False)
                    lw, lz = tools.compute_logw_and_logz(logl, beta, logz, bf, normalize=False)
                assert np.array_equal(np.isnan(lw), np.isnan(olw)) and np.array_equal(np.isnan(lw), np.isneginf(logl.reshape(-1)))
                ok = ~np.isnan(olw)
                env = pr.mixture_envelope(logl, beta, logz, bf, ex)[ok]
                exf = ex[ok].astype(np.float64)
                e = np.abs((lw.astype(np.longdouble) - ex).astype(np.float64))[ok]
                eo = np.abs((olw.astype(np.longdouble) - ex).astype(np.float64))[ok]
                lim = np.maximum(pr.BOUND["logw"] * (1 + np.abs(exf)), pr.C * env)
                if ok.any():
                    fl = np.maximum(env, 2.0 ** -53 * (1 + np.abs(exf)))
                    m = MEASURED.setdefault(("logw", f"T{T}_width{width}"), [0.0, 0.0])
                    m[0], m[1] = max(m[0], float((e / fl).max())), max(m[1], float((eo / fl).max()))
                assert (e <= lim).all(), (T, N, width, bf, float((e / lim).max()))
                with np.errstate(invalid="ignore"):
                    lw2, lz2 = pool.logw_and_logz(bf, normalize=False)
                assert np.array_equal(lw, lw2, equal_nan=True) and (lz == lz2 or (np.isnan(lz) and np.isnan(lz2)))
                if holes:
                    assert np.isnan(lz)                                # a NaN log-weight makes the evidence NaN, as in the reference
                    continue
                # ESS and logZ of the trial from the device's own log-weights, against their exact statistics
                exs = pr.exact_stats(lw)
                envs = pr.stats_envelope(lw, exs)
                ess = pool.ess(bf)
                assert pr.err(ess, exs["ess"]) <= pr.allowed("ess", exs["ess"], envs["ess"]), (T, N, width, bf)
                exz = exs["logz"] - math.log(T * N)
                assert pr.err(lz, exz) <= pr.allowed("logz", exz, envs["logz"]), (T, N, width, bf)
    # Particles.logw_stats: the same kernels on the resident pool
    logl, beta, logz = pr.history(T, 257, width)
    Pt = Particles(257, 1)
    z = np.zeros(257)
    for t in range(T):
        Pt.update(dict(u=z[:, None], x=z[:, None], logdetj=z, logp=z, logl=logl[t], beta=beta[t], logz=logz[t], iter=t,
                       calls=0, steps=1, efficiency=1.0, ess=1.0, accept=1.0))
    pool = tools.PoolWeights(logl, beta, logz)
    for bf in (0.0, 0.41, 1.0):
        np.testing.assert_array_equal(Pt.logw_stats(bf, k=T * 257), pool.stats(bf, k=T * 257))


# --------------------------------------------------------------------------------------------------------- trimming
def check_trim(regime, w, ess, bins, oracle_up_to=8193):
    P = len(w)
    tr = pr.trim_exact(w, ess, bins)
    thr, b, idx, wt = dev_trim(w, ess, bins)
    assert b in tr["valid"], (regime, P, ess, bins, b, tr["valid"], tr["knife"])
    if tr["knife"]:
        KNIFE.append((regime, P, ess, bins, b, pr.oracle_trim_bin(w, ess, bins), tr["knife"]))
    else:
        assert b == tr["bin"], (regime, P, ess, bins, b, tr["bin"])
        if P <= oracle_up_to:                                     # the oracle itself (its bin is pinned on the CPU above that)
            i_or, w_or = otools.trim_weights(np.arange(P), w.copy(), ess, bins)
            np.testing.assert_array_equal(idx, i_or)
            np.testing.assert_allclose(wt, w_or, rtol=1e-13)
    assert thr == tr["thr"][b], (regime, P, ess, bins, thr, tr["thr"][b])
    np.testing.assert_array_equal(idx, np.nonzero(w >= thr)[0])         # exactly {i : w_i >= threshold}, in index order
    kept = w[idx]
    s_env = max(abs(float(np.sum((kept / np.sum(kept))[p])) - 1.0) for p in pr.permutations(len(kept)))
    assert abs(math.fsum(wt) - 1.0) <= max(pr.BOUND["sum"], pr.C * s_env), (regime, P, math.fsum(wt))
    np.testing.assert_allclose(wt, kept / math.fsum(kept), rtol=1e-13, atol=0)
    if regime == "equal" or thr == 0.0:
        assert len(idx) == P
    return b


@pytest.mark.parametrize("regime", pr.REGIMES)
def test_trimming(regime):
    """``pmc_trim_threshold`` / ``pmc_trim_select`` and ``tools.trim_weights``: away from a knife edge bin, threshold and
    kept indices equal the reference's exactly; on one the bin is the reference's or one whose exact ratio is inside
    the band."""
    from pocomc_amd import tools
    for P in pr.SORT_SIZES:
        w = pr.weights(regime, P)
        w /= np.sum(w)
        check_trim(regime, w, 0.99, 1000)
        thr, b, idx, wt = dev_trim(w, 0.99, 1000)
        i2, w2 = tools.trim_weights(np.arange(P), w.copy())
        np.testing.assert_array_equal(i2, idx)
        np.testing.assert_allclose(w2, wt, rtol=1e-13)
    for P in (17, 1000):
        w = pr.weights(regime, P)
        w /= np.sum(w)
        for ess in (0.9, 0.99, 0.999):
            for bins in (2, 10, 1000, 65536):
                if bins == 65536 and (P != 1000 or ess != 0.99):
                    continue                                             # (the exact ratios of 65536 bins: once per regime)
                check_trim(regime, w, ess, bins)


def test_pool_select_in_the_regimes():
    """``Particles.select`` on a resident pool: its weights and trim against the exact decision on those weights."""
    from pocomc_amd.particles import Particles
    for T, width in ((9, 4), (40, 300), (1, 4)):
        logl, beta, logz = pr.history(T, 257, width)
        Pt = Particles(257, 1)
        z = np.zeros(257)
        for t in range(T):
            Pt.update(dict(u=z[:, None], x=z[:, None], logdetj=z, logp=z, logl=logl[t], beta=beta[t], logz=logz[t],
                           iter=t, calls=0, steps=1, efficiency=1.0, ess=1.0, accept=1.0))
        for bf in (0.0, 0.41, 1.0):
            Pt.logw_stats(bf)
            w, idx, wt = Pt.select(ess=0.99, bins=1000)
            w, idx, wt = w.cpu().numpy(), idx.cpu().numpy(), wt.cpu().numpy()
            tr = pr.trim_exact(w)
            thr = [t for i, t in enumerate(tr["thr"]) if i in tr["valid"] and np.array_equal(np.nonzero(w >= t)[0], idx)]
            assert thr, (T, width, bf, tr["valid"])
            if not tr["knife"]:
                i_or, w_or = otools.trim_weights(np.arange(len(w)), w.copy())
                np.testing.assert_array_equal(idx, i_or)
                np.testing.assert_allclose(wt, w_or, rtol=1e-13)


# ------------------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("regime", pr.REGIMES)
def test_resampling(regime):
    """Systematic and multinomial indices equal the reference's sequential implementations bit for bit.  Where the
    reference raises (a systematic position above a cdf that rounds below 1) the device clamps to ``P - 1``: the
    documented contract of ``pmc_resample_systematic``."""
    from pocomc_amd import tools
    rng = np.random.default_rng(5)
    clamped = 0
    for P in pr.RESAMPLE_SIZES:
        w = pr.weights(regime, P)
        w = w / np.sum(w)
        cdf = np.cumsum(w)
        cdf /= cdf[-1]
        for n_out in sorted({1, max(P // 3, 1), P, 4 * P}):
            for off in (0.0, 0.37, pr.ONE_BELOW):
                ref, over = pr.systematic_reference(n_out, w, off)
                clamped += int(over.sum())
                got = tools.systematic_resample(n_out, w.copy(), offset=off)
                np.testing.assert_array_equal(got, np.minimum(ref, P - 1), err_msg=f"{regime} P={P} n_out={n_out} offset={off}")
            u = rng.random(n_out)
            u[0] = 0.0
            u[-1:] = pr.ONE_BELOW if n_out > 1 else 0.0
            if n_out > 8:                                            # uniforms that EQUAL a cdf entry: side='right' decides
                u[1:7] = cdf[rng.integers(0, P, 6)]
                u[1:7] = np.minimum(u[1:7], pr.ONE_BELOW)
            got = tools.multinomial_resample(n_out, w, uniforms=u)
            np.testing.assert_array_equal(got, otools.multinomial_resample(n_out, w, uniforms=u),
                                          err_msg=f"{regime} P={P} n_out={n_out}")
            assert (w[got] > 0.0).all()                              # a particle of weight 0.0 is never drawn
    print(f"{regime}: {clamped} systematic positions above the cdf's last entry (clamped to P - 1)")


# ---------------------------------------------------------------------------------------------- moments and medians
MOMENT_SHAPES = [(1, 1), (2, 15), (63, 16), (64, 17), (65, 128), (1023, 16), (1025, 128), (1025, 17), (20000, 15), (20000, 17)]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n,D", MOMENT_SHAPES)
def test_moments_in_the_regimes(n, D, f32):
    """``pmc_moments`` with weights from the regimes (zeros, one-hot) on data with a large offset (mean 1e8, spread 1 in
    float64; 1e4 in float32, whose spacing at 1e8 is 8), with and without ``idx``."""
    import torch
    from pocomc_amd.geometry import moments
    rng = np.random.default_rng(n * 131 + D)
    x = ((1e4 if f32 else 1e8) + rng.normal(size=(n, D))).astype(np.float32 if f32 else np.float64)
    xd = torch.from_numpy(x).cuda()
    idx = rng.integers(0, n, size=max(n // 2, 1))
    cases = [(r, pr.weights(r, n), None) for r in ("gauss", "very_wide", "one_hot", "equal")] + [("none", None, None), ("idx", None, idx)]
    for name, w, ix in cases:
        xs = x if ix is None else x[ix]
        mean, S, v1, v2 = moments(xd, None if ix is None else torch.from_numpy(ix).cuda(), None if w is None else up(w))
        em, eS, e1, e2 = pr.exact_moments(xs, w)
        om, oS = pr.oracle_moments(xs, w)
        envm, envS = pr.moments_envelope(xs, w, em, eS)
        d = lambda a, b: np.abs((a - b).astype(np.float64))
        m64, S64 = em.astype(np.float64), eS.astype(np.float64)
        lim_m = np.maximum(pr.BOUND["mean"] * np.abs(m64) + 1e-13, pr.C * envm)
        lim_S = np.maximum(pr.BOUND["scatter"] * np.abs(S64) + 1e-10, pr.C * envS)
        for q, e, eo, env, sc in (("mean", d(mean, em), d(om, em), envm, np.abs(m64)), ("scatter", d(S, eS), d(oS, eS), envS, np.abs(S64).max())):
            fl = np.maximum(env, 2.0 ** -53 * np.maximum(sc, 1e-300))
            m = MEASURED.setdefault((q, name), [0.0, 0.0])
            m[0], m[1] = max(m[0], float((e / fl).max())), max(m[1], float((eo / fl).max()))
        assert (d(mean, em) <= lim_m).all(), (name, n, D, f32, float((d(mean, em) / lim_m).max()))
        assert (d(S, eS) <= lim_S).all(), (name, n, D, f32, float((d(S, eS) / lim_S).max()))
        assert abs(v1 - float(e1)) <= 1e-13 * float(e1) and abs(v2 - float(e2)) <= 1e-13 * float(e2)
        np.testing.assert_array_equal(S, S.T)
        if name == "one_hot":
            k = int(np.argmax(w))
            assert (S == 0.0).all() and np.array_equal(mean, x[k].astype(np.float64)) and v1 == 1.0 == v2


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1025, 20000])
def test_medians_of_awkward_columns(n, f32):
    """``pmc_column_medians`` against ``np.median``: ties, +-0.0, +-inf, even n in float32 (the mean of the two middle
    elements is a float32), and NaN (of either sign) in a column, where ``np.median`` is NaN."""
    import torch
    from pocomc_amd.geometry import column_medians
    rng = np.random.default_rng(n)
    dt = np.float32 if f32 else np.float64
    x = rng.normal(size=(n, 17)).astype(dt)
    x[:, 0] = np.round(2 * x[:, 0])                                       # ties
    x[:, 1] = np.where(rng.random(n) < 0.5, dt(0.0), dt(-0.0))            # +-0.0 only
    x[:, 2] = np.where(rng.random(n) < 0.3, dt(0.0), np.where(rng.random(n) < 0.5, dt(-0.0), x[:, 2]))
    x[rng.random(n) < 0.2, 3] = np.inf
    x[rng.random(n) < 0.2, 4] = -np.inf
    x[:, 5] = np.where(rng.random(n) < 0.5, np.inf, -np.inf)
    x[:, 6] = 1e8 + x[:, 6]
    x[rng.integers(n), 7] = np.nan
    x[rng.integers(n), 8] = -np.nan
    x[rng.integers(n), 9] = np.copysign(np.nan, -1.0)
    x[rng.integers(n), 10] = np.nan
    x[rng.integers(n), 10] = np.copysign(np.nan, -1.0)
    x[:, 11] = np.nan
    assert np.signbit(x[:, 9]).any() or n == 0
    idx = rng.integers(0, n, size=max(n // 2, 1))
    xd = torch.from_numpy(x).cuda()
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        ref, ref_i = np.median(x, axis=0), np.median(x[idx], axis=0)
    got, got_i = column_medians(xd), column_medians(xd, torch.from_numpy(idx).cuda())
    assert got.dtype == dt and np.isnan(ref[7:12]).all()
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got_i, ref_i)


# --------------------------------------------------------------------------------------------------------- bootstrap
@pytest.mark.parametrize("regime", ["very_wide", "holes", "gauss"])
def test_bootstrap_replay(regime):
    """``pmc_bootstrap_logz_replay`` on recorded draws against the 50-digit log-sum-exp; a replicate that draws only
    ``-inf`` entries is ``-inf``, not NaN."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    for n in (1, 255, 513, 1000):
        lw = pr.logw(regime, n)
        B = 6
        draws = rng.integers(0, n, size=(B, n))
        holes = np.nonzero(np.isneginf(lw))[0]
        if len(holes):
            draws[2] = np.resize(holes, n)
        ex = pr.exact_bootstrap(lw, draws)
        lwd, dd = up(lw), up(draws, np.int64)
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        ws = torch.empty(int(lib.pmc_reduce_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        out = torch.empty(B, dtype=torch.float64, device="cuda")
        st = _lib.stream_handle()
        _lib.check(lib.pmc_logw_stats(_lib.ptr(lwd), n, 0, _lib.ptr(stats), _lib.ptr(ws), st))
        _lib.check(lib.pmc_bootstrap_logz_replay(_lib.ptr(lwd), n, _lib.ptr(stats), B, _lib.ptr(dd), _lib.ptr(out), st))
        got = out.cpu().numpy()
        for b in range(B):
            if ex[b] == -pr.mpmath.inf:
                assert got[b] == -np.inf, (regime, n, b, got[b])
                continue
            with np.errstate(divide="ignore"):
                orc = [np.logaddexp.reduce(lw[draws[b][p]]) - np.log(n) for p in pr.permutations(n)]
                o = np.logaddexp.reduce(lw[draws[b]]) - np.log(n)
            env = max(pr.err(v, ex[b]) for v in orc)
            e = pr.err(got[b], ex[b])
            note("bootstrap", regime, e, pr.err(o, ex[b]), env, 1 + abs(float(ex[b])))
            assert e <= pr.allowed("logz", ex[b], env), (regime, n, b, got[b], float(ex[b]), env)
