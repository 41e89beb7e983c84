"""Every kernel that draws from ``csrc/philox.h`` against the host model of ``tests/philox_model.py`` (judged without a
GPU by ``tests/test_philox_model_cpu.py``): the *values* a (seed, step, particle, stream, draw) yields, not their law.

``pmc_rng_fill`` equals the inline draws of the proposal kernels bit for bit (``test_proposal_in_every_width_class``,
``test_fused_proposal_and_inverse_equal_the_two_launches``, ``test_variates_drawn_ahead_equal_inline_draws``), so
holding it to the model pins those too; the fit noise (``pmc_add_noise_rows_f32``) and the bootstrap
(``pmc_bootstrap_logz``) are compared directly.

Exact here: the uniforms, the bootstrap's indices and its sum, the float32 noise arithmetic.  Within a bound: the
normals and the gamma value (the device's ``log``, ``sqrt``, ``sincospi``, ``pow``) against the longdouble yardstick,
bound = 4 x the float64 twin's own largest error, in ulps of the value (``philox_model.bound_ulps``).  ``-s`` prints
the bound and the largest device error / bound per family (recorded in ``profiles/philox_model.txt``)."""
import ctypes as C

import numpy as np
import pytest

import philox_model as pm
import pool_regimes as pr

pytestmark = pytest.mark.gpu

MEASURED = {}          # family -> largest device error / bound
GUARD = 16             # elements past the end of an output that must stay untouched


def note(family, ratio):
    MEASURED[family] = max(MEASURED.get(family, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    e = pm.twin_error()
    print(f"\ntwin vs yardstick: normals {e.normal:.3f} ulps, pow {e.pow:.3f} ulps; bound {pm.bound_ulps():.3f} ulps")
    print("family: largest device error / bound")
    for k, v in sorted(MEASURED.items()):
        print(f"  {k:28s} {v:8.4f}")


def guarded(n_elem, dtype):
    """A device buffer of ``n_elem`` elements followed by ``GUARD`` NaNs: ``(whole, view of the first n_elem)``."""
    import torch
    whole = torch.full((n_elem + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return whole, whole[:n_elem]


def untouched(whole):
    return bool(whole[-GUARD:].isnan().all().item())


def fill(seed, step, offset, n, D, gamma_shape=0.0, normal=True, uniform=True):
    """``pmc_rng_fill``: ``(normal (n, D) | None, gamma (n) | None, uniform (n) | None)`` as numpy arrays."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    r = _lib.pmc_rng_t(gamma=None, normal=None, uniform=None, seed=seed, step=step, offset=offset)
    zw, z = guarded(n * D, torch.float64) if normal else (None, None)
    gw, g = guarded(n, torch.float64) if gamma_shape > 0 else (None, None)
    uw, u = guarded(n, torch.float64) if uniform else (None, None)
    _lib.check(lib.pmc_rng_fill(C.byref(r), float(gamma_shape), _lib.ptr(z), _lib.ptr(g), _lib.ptr(u), n, D,
                                _lib.stream_handle()), "pmc_rng_fill")
    torch.cuda.synchronize()
    for w in (zw, gw, uw):
        assert w is None or untouched(w)
    host = lambda t: None if t is None else t.cpu().numpy()
    return (None if z is None else host(z).reshape(n, D)), host(g), host(u)


def check_normals(z, yard, u1, family):
    """Device normals within the bound of the yardstick; every complete pair returns the model's first uniform."""
    bound = pm.bound_ulps()
    assert np.isfinite(z).all()
    e = pm.ulps(z, yard)
    note(family, e.max() / bound)
    assert e.max() <= bound, (family, float(e.max()), bound, np.unravel_index(e.argmax(), e.shape))
    full = z.shape[1] // 2
    if full:
        r2 = z[:, 0:2 * full:2] ** 2 + z[:, 1:2 * full:2] ** 2
        np.testing.assert_allclose(np.exp(-0.5 * r2), u1[:, :full], rtol=1e-12, atol=0)


def check_gamma(g, model, family):
    """Device gamma within its row bound of the yardstick's value AT THE MODEL'S CANDIDATE: a device that accepted
    another candidate returns an unrelated number.  No row is left out (margins: the CPU file)."""
    assert (model.margin >= pm.MARGIN_MIN).all()
    assert np.isfinite(g).all() and (g > 0).all()
    ratio = pm.ulps(g, model.yard) / (model.factor * pm.bound_ulps())
    note(family, ratio.max())
    worst = int(ratio.argmax())
    assert ratio.max() <= 1.0, (family, worst, g[worst], float(model.yard[worst]), int(model.candidate[worst]))


# ------------------------------------------------------------------------------------------------- pmc_rng_fill
@pytest.mark.parametrize("D", pm.FILL_D)
@pytest.mark.parametrize("n", pm.FILL_N)
def test_rng_fill_equals_the_model(n, D):
    """Odd ``D`` (the last pair's second normal is dropped), ``D = 1``, more pairs than a wave has lanes, one row and
    rows across several workgroups."""
    m = pm.fill_case(pm.SEED, pm.STEP, 0, max(pm.FILL_N), D, pm.FILL_SHAPE)
    z, g, u = fill(pm.SEED, pm.STEP, 0, n, D, pm.FILL_SHAPE)
    assert np.array_equal(u, m.uniform[:n])                                  # bit for bit
    check_normals(z, m.normal_yard[:n], m.u1[:n], "normal")
    check_gamma(g, pm.first_rows(m.gamma, n), "gamma 18.5")


@pytest.mark.parametrize("shape", pm.GAMMA_SHAPES)
def test_gamma_equals_the_model(shape):
    """The scale draw alone (no normal, no uniform buffer) at every shape class: the boost branch below one, the
    Student-t EM fit's ends, the bench's, the clamped nu."""
    m = pm.gamma_case(shape)
    if shape in (0.5, 1.05):
        # rows that accept at the second candidate and in the second round trip: the draw index moves on correctly
        assert (m.candidate == 1).any() and (m.candidate >= 2).any()
    _, g, _ = fill(pm.SEED, pm.STEP, 0, pm.GAMMA_N, 2, shape, normal=False, uniform=False)
    check_gamma(g, m, f"gamma {shape:g}")
    late = m.candidate >= 1
    if late.any():
        note(f"gamma {shape:g} late rows", (pm.ulps(g, m.yard) / (m.factor * pm.bound_ulps()))[late].max())


@pytest.mark.parametrize("offset", pm.EDGE_OFFSETS)
@pytest.mark.parametrize("seed", pm.EDGE_SEEDS)
def test_keys_and_counters_at_their_edges(seed, offset):
    """Seeds with a non-zero upper key word (``mcmc.py`` / ``sampler.py`` draw up to 2^62), steps from 2^32 on (the
    fold), and 64 rows that straddle the 32-bit boundary of the particle word or lie beyond it."""
    n, D = pm.EDGE_N, pm.EDGE_D
    for step in pm.EDGE_STEPS:
        m = pm.fill_case(seed, step, offset, n, D)
        for i, shape in enumerate(pm.EDGE_SHAPES):
            z, g, u = fill(seed, step, offset, n, D, shape, normal=i == 0, uniform=i == 0)
            if i == 0:
                assert np.array_equal(u, m.uniform), (seed, step, offset)
                check_normals(z, m.normal_yard, m.u1, "normal, edge keys")
            check_gamma(g, pm.gamma_case(shape, seed, step, offset, n), "gamma, edge keys")


# ---------------------------------------------------------------------------------------------------- fit noise
def add_noise(x, scale, seed, pass_, row0=None):
    """``pmc_add_noise_rows_f32`` (``row0=None``: ``pmc_add_noise_f32``) on a host float32 array; numpy (n, D)."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    n, D = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    whole, out = guarded(n * D, torch.float32)
    st = _lib.stream_handle()
    if row0 is None:
        _lib.check(lib.pmc_add_noise_f32(_lib.ptr(xd), n, D, scale, seed, pass_, _lib.ptr(out), st), "pmc_add_noise_f32")
    else:
        _lib.check(lib.pmc_add_noise_rows_f32(_lib.ptr(xd), n, D, scale, seed, pass_, row0, _lib.ptr(out), st),
                   "pmc_add_noise_rows_f32")
    torch.cuda.synchronize()
    assert untouched(whole)
    return out.cpu().numpy().reshape(n, D)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_noise(got, yard):
    """Bit-equal to ``float32`` of the model wherever the bound decides the rounding (everywhere: the CPU file)."""
    want, decided = pm.float32_of(yard, pm.bound_ulps())
    assert decided.all()
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


@pytest.mark.parametrize("D", pm.NOISE_D)
@pytest.mark.parametrize("n", pm.NOISE_N)
def test_fit_noise_is_float32_of_the_model(n, D):
    _, yard = pm.noise_case(max(pm.NOISE_N), D)
    got = add_noise(np.zeros((n, D), np.float32), 1.0, pm.NOISE_SEED, pm.NOISE_PASS, 0)
    check_noise(got, yard[:n])


def test_fit_noise_past_the_grid_cap():
    """``n * ceil(D / 2) > 4096 * 256``: the elements past the capped grid are reached through the stride loop."""
    n, D = pm.NOISE_LARGE
    assert n * ((D + 1) // 2) > 4096 * 256
    got = add_noise(np.zeros((n, D), np.float32), 1.0, pm.NOISE_SEED, pm.NOISE_PASS, 0)
    check_noise(got, pm.noise_case(n, D)[1])


@pytest.mark.parametrize("n, D", [(300, 33), (5000, 3)])
def test_fit_noise_arithmetic_shards_and_passes(n, D):
    """``out = x + scale * noise`` as float32 multiply then add (no FMA); ``row0 = k`` returns rows ``k..`` of the whole
    set; the one-shard entry point is ``row0 = 0``; every pass has the model's own noise."""
    zero = np.zeros((n, D), np.float32)
    noise = add_noise(zero, 1.0, pm.NOISE_SEED, pm.NOISE_PASS, 0)
    x = np.random.default_rng(n).normal(size=(n, D)).astype(np.float32) * np.float32(3.0)
    for scale in (0.37, 1e-3, 25.0):
        got = add_noise(x, scale, pm.NOISE_SEED, pm.NOISE_PASS, 0)
        want = x + np.float32(scale) * noise
        assert want.dtype == np.float32 and np.array_equal(bits(got), bits(want)), scale
    assert np.array_equal(bits(add_noise(x, 0.37, pm.NOISE_SEED, pm.NOISE_PASS)),
                          bits(add_noise(x, 0.37, pm.NOISE_SEED, pm.NOISE_PASS, 0)))
    for k in (1, n // 3, n - 1):                           # a rank's shard: rank * rows
        assert np.array_equal(bits(add_noise(zero[k:], 1.0, pm.NOISE_SEED, pm.NOISE_PASS, k)), bits(noise[k:])), k
    for p in (pm.NOISE_PASS + 1, 2 ** 32 + 1):
        got = add_noise(zero[:300], 1.0, pm.NOISE_SEED, p, 0)
        check_noise(got, pm.noise_case(300, D, pass_=p)[1])
        assert not np.array_equal(got, noise[:300])
    # a seed with an upper key word, rows beyond the 32-bit boundary of the particle word
    got = add_noise(zero[:300], 1.0, 2 ** 62 - 1, pm.NOISE_PASS, 0)
    check_noise(got, pm.noise_case(300, D, seed=2 ** 62 - 1)[1])
    row0 = 2 ** 32 - 8
    got = add_noise(zero[:64], 1.0, pm.NOISE_SEED, pm.NOISE_PASS, row0)
    check_noise(got, pm.fit_noise(pm.NOISE_SEED, pm.NOISE_PASS, row0, 64, D)[1])


@pytest.mark.parametrize("n", [2, 1023, 1024, 1025, 3000])
def test_mean_distance(n):
    """``pmc_mean_distance_f32`` (the quantity the noise scale is built from) around its 1024 threads, for the first,
    a middle and the last row, against float64."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    D = 6
    x = np.random.default_rng(n).normal(size=(n, D)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    for row in (0, n // 2, n - 1):
        md = torch.full((1 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.pmc_mean_distance_f32(_lib.ptr(xd), n, D, row, _lib.ptr(md), _lib.stream_handle()))
        torch.cuda.synchronize()
        assert untouched(md)
        x64 = x.astype(np.float64)
        ref = np.sqrt(((x64[row] - x64) ** 2).sum(axis=1)).mean()
        np.testing.assert_allclose(md[0].item(), ref, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------- bootstrap
@pytest.mark.parametrize("seed", [12345, 2 ** 32 + 12345, 2 ** 62 - 1])
@pytest.mark.parametrize("n", [1, 2, 255, 511, 512, 513, 1025])
def test_bootstrap_draws_the_models_indices(n, seed):
    """``pmc_bootstrap_logz(seed)`` is bit-equal to ``pmc_bootstrap_logz_replay`` fed with the model's indices: the same
    kernel and the same arithmetic, only the source of the indices differs.  Sizes around the 512 elements one sweep
    of a workgroup covers, odd ones (the tail takes the first index of its pair only), log-weights 30 nats wide."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    B = 8
    lw = pr.logw("wide", n)
    idx = pm.bootstrap_indices(seed, B, n)
    assert idx.shape == (B, n) and idx.min() >= 0 and idx.max() < n          # what the replay kernel will index with
    lwd = torch.from_numpy(lw).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.pmc_reduce_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    ow, out = guarded(B, torch.float64)
    rw, rep = guarded(B, torch.float64)
    st = _lib.stream_handle()
    _lib.check(lib.pmc_logw_stats(_lib.ptr(lwd), n, 0, _lib.ptr(stats), _lib.ptr(ws), st))
    _lib.check(lib.pmc_bootstrap_logz(_lib.ptr(lwd), n, _lib.ptr(stats), B, seed, _lib.ptr(out), st), "pmc_bootstrap_logz")
    _lib.check(lib.pmc_bootstrap_logz_replay(_lib.ptr(lwd), n, _lib.ptr(stats), B, _lib.ptr(dd), _lib.ptr(rep), st))
    torch.cuda.synchronize()
    assert untouched(ow) and untouched(rw)
    got, want = out.cpu().numpy(), rep.cpu().numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, seed, got, want)
    if n > 2:
        assert len(np.unique(got)) > 1                                          # replicates differ: the step word counts
    # and the replay is the log-sum-exp of those draws (float64, order aside)
    ref = np.array([np.logaddexp.reduce(lw[i]) - np.log(n) for i in idx])
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
