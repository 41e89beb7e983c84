"""``pmc_student_em_weighted`` (``csrc/student.hip``), ``Geometry(student="em_weighted")`` and
``Sampler(student_fit="em_weighted")`` against the float64 numpy / scipy restatement of ``tests/student_em_weighted.py``.

Bound (``mu`` relative to ``max|mu|``, ``Sigma`` to ``max|Sigma|``, ``nu`` to itself): ``se.tolerances`` of the restatement's
own reordering noise on the case -- 1e-9 where that noise is below 2e-12, 500 times the noise recorded in ``sw.NOISE`` on the
few cases where it is not (``tests/test_student_em_weighted_cpu.py`` re-measures every one).  ``-s`` prints the measured maxima
(``profiles/student_em_weighted.txt``).

A fit that is run to the end stops at the first iteration whose ``|delta nu|`` is at most ``tol``.  The device's ``nu`` is held
to the restatement's within the bound only, so where a step of the restatement lies within twice that bound (times ``nu``)
of ``tol`` the two may stop an iteration apart; the device is then compared with the restatement at the device's own length,
and its length must be one the restatement's steps allow."""
import ctypes as C
import functools

import numpy as np
import pytest

import student_em as se
import student_em_weighted as sw

pytestmark = pytest.mark.gpu

MEASURED = {}          # test group -> largest relative deviation of (mu, Sigma, nu) and of deviation / bound


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nweighted student EM, device against the restatement: largest relative deviation of mu | Sigma | nu | deviation / bound")
    for k, (a, b, c, d) in sorted(MEASURED.items()):
        print(f"  {k:28s} {a:9.2e} | {b:9.2e} | {c:9.2e} | {d:9.2e}")


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def within(group, mu, sigma, nu, ref, tol=(1e-9, 1e-9, 1e-9)):
    """Records the deviations of a device result from ``ref`` and returns whether each is below its bound
    ``tol = (nu, mu, Sigma)``."""
    e_mu = np.abs(mu - ref["mu"]).max() / np.abs(ref["mu"]).max()
    e_s = np.abs(sigma - ref["sigma"]).max() / np.abs(ref["sigma"]).max()
    e_nu = abs(nu - ref["nu"]) / ref["nu"] if np.isfinite(ref["nu"]) else float(nu != ref["nu"])
    ratio = max(e_nu / tol[0], e_mu / tol[1], e_s / tol[2])
    m = MEASURED.setdefault(group, [0.0, 0.0, 0.0, 0.0])
    m[:] = max(m[0], e_mu), max(m[1], e_s), max(m[2], e_nu), max(m[3], ratio)
    print(f"{group}: mu {e_mu:.2e} Sigma {e_s:.2e} nu {e_nu:.2e} (bounds nu {tol[0]:.1e} mu {tol[1]:.1e} Sigma {tol[2]:.1e})")
    return ratio < 1.0


# --------------------------------------------------------------------------------------------------------- 1. parity
@functools.lru_cache(maxsize=None)
def case(n, D, f32, regime):
    """``(rows, w, start)`` of a parity case; the references below are computed once each."""
    x = sw.case_rows(n, D, f32)
    w = sw.case_weights(n, D, regime)
    return x, w, sw.start_values(x, w)


@functools.lru_cache(maxsize=None)
def reference(n, D, f32, regime, tol, max_iter):
    x, w, start = case(n, D, f32, regime)
    return sw.fit(x, w, *start, tol=tol, max_iter=max_iter)


@pytest.mark.parametrize("regime", sw.REGIMES)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,D", sw.SHAPES)
def test_parity(n, D, f32, regime):
    from pocomc_amd.geometry import student_em_weighted
    x, w, start = case(n, D, f32, regime)
    dx, dw = up(x), up(w)
    for k, (tol, max_iter) in enumerate(sw.LENGTHS):
        bound = sw.tolerances(n, D, regime, k)
        ref = reference(n, D, f32, regime, tol, max_iter)
        mu, sigma, info = student_em_weighted(dx, dw, *start, tol=tol, max_iter=max_iter)
        print(f"{n}x{D} {regime} tol {tol:g} max_iter {max_iter}: device {info['status']} after {info['iterations']}, restatement "
              f"{ref['status']} after {ref['iterations']}, nu {ref['nu']:.6g}")
        assert info["host_reads"] == 1 + (info["iterations"] + 7) // 8
        assert info["rows_positive"] == ref["rows_positive"] == int((w > 0).sum())
        assert abs(info["ess"] - ref["ess"]) <= 1e-12 * ref["ess"]
        if tol > 0.0 and info["iterations"] != ref["iterations"]:
            # the stop rule within the precision of the comparison (module docstring)
            it = info["iterations"]
            ref = reference(n, D, f32, regime, 0.0, it)
            slack = 2.0 * bound[0] * ref["nu"]
            assert ref["iterations"] == it and info["status"] == "converged"
            assert ref["steps"][it - 1] <= tol + slack and all(s > tol - slack for s in ref["steps"][:it - 1])
        else:
            assert info["status"] == ref["status"] and info["iterations"] == ref["iterations"]
        assert within(f"parity {n}x{D}", mu, sigma, info["nu"], ref, bound), (regime, tol, max_iter)


# ---------------------------------------------------------------------- 2. integer weights against the existing entry
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("seed,n,D", [(1, 300, 6), (2, 517, 33), (3, 400, 128)])
def test_integer_weights_give_the_fit_of_the_repeated_rows(seed, n, D, f32):
    """``student_em`` on an ``idx`` that holds row ``r`` ``k_r`` times against ``student_em_weighted`` with ``w = k``: the new
    sums against the old ones, on the device."""
    from pocomc_amd.geometry import student_em, student_em_weighted
    x = se.mvt_rows(seed, n, D, 5.0, dtype=np.float32 if f32 else np.float64)
    k = np.random.default_rng(seed).integers(0, 4, size=n)
    start = sw.start_values(x, k.astype(np.float64))
    dx, idx, dw = up(x), up(np.repeat(np.arange(n), k)), up(k.astype(np.float64))
    for kw in (dict(tol=0.0, max_iter=10), dict()):
        a = student_em_weighted(dx, dw, *start, **kw)
        b = student_em(dx, idx, *start, **kw)
        assert a[2]["status"] == b[2]["status"] and a[2]["iterations"] == b[2]["iterations"] > 1
        assert a[2]["rows_positive"] == int((k > 0).sum()) and abs(a[2]["ess"] - sw.ess(k.astype(np.float64))) < 1e-9
        assert within("integer weights", a[0], a[1], a[2]["nu"], dict(mu=b[0], sigma=b[1], nu=b[2]["nu"]))


# ------------------------------------------------------------------------------------------- 3. rows of weight zero
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("where", ["first", "last", "chunk"])
def test_a_row_of_weight_zero_is_not_read(where, bad, f32):
    """130 rows are 64 chunks of 3 rows (the last ones empty): row 3 opens the second chunk.  The row holds NaN / inf in
    every column; the fit is the fit with zeros in that row, bit for bit."""
    from pocomc_amd.geometry import student_em_weighted
    n, D = 130, 17
    x = sw.case_rows(n, D, f32)
    r = dict(first=0, last=n - 1, chunk=3)[where]
    w = sw.weights("lognormal1", n, seed=5)
    w[r] = 0.0
    clean = x.copy()
    clean[r] = 0.0
    dirty = x.copy()
    dirty[r] = bad
    dirty[r, ::2] = -bad if np.isinf(bad) else bad
    start = sw.start_values(clean, w)
    a = student_em_weighted(up(dirty), up(w), *start)
    b = student_em_weighted(up(clean), up(w), *start)
    assert a[2]["iterations"] > 8 and a[2]["rows_positive"] == n - 1
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()


# ------------------------------------------------------------------------------------------ 4. scale and determinism
@pytest.mark.parametrize("n,D,regime", [(130, 17, "lognormal1"), (300, 64, "integer"), (220, 157, "uniform")])
def test_the_scale_of_the_weights_does_not_matter(n, D, regime):
    from pocomc_amd.geometry import student_em_weighted
    x, w, start = case(n, D, False, regime)
    ref = reference(n, D, False, regime, 0.0, 10)
    mu, sigma, info = student_em_weighted(up(x), up(7.3 * w), *start, tol=0.0, max_iter=10)
    assert info["status"] == ref["status"] and info["iterations"] == ref["iterations"]
    assert abs(info["ess"] - ref["ess"]) <= 1e-12 * ref["ess"]
    assert within("weights x 7.3", mu, sigma, info["nu"], ref, sw.tolerances(n, D, regime, 2))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,D", [(130, 17), (220, 157)])
def test_same_bits_on_every_call(n, D, f32):
    from pocomc_amd.geometry import student_em_weighted
    x, w, start = case(n, D, f32, "zeros5")
    a = student_em_weighted(up(x), up(w), *start, max_iter=12)
    b = student_em_weighted(up(x), up(w), *start, max_iter=12)
    assert a[2]["iterations"] >= 4
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# -------------------------------------------------------------------------------------------------- 5. what it refuses
@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf, -np.inf, -0.5e-300])
def test_bad_weights_raise_and_leave_the_start_values(bad):
    """Through the library itself: the call fails before any EM kernel runs, ``mu_io`` / ``sigma_io`` keep their bits."""
    import torch
    from pocomc_amd import _lib
    from pocomc_amd.geometry import student_em_weighted
    n, D = 130, 5
    x = sw.case_rows(n, D)
    w = sw.weights("lognormal1", n, seed=1)
    w[77] = bad
    start = sw.start_values(x, np.abs(np.nan_to_num(w, nan=1.0, posinf=1.0, neginf=1.0)))
    keep = [s.copy() for s in start]
    with pytest.raises(ValueError, match="weights must be finite and non-negative"):
        student_em_weighted(up(x), up(w), *start)
    assert np.array_equal(start[0], keep[0]) and np.array_equal(start[1], keep[1])
    lib = _lib.load()
    io = up(np.concatenate([start[0], start[1].ravel()]))
    before = io.clone()
    dx, dw = up(x), up(w)
    nbytes = int(lib.pmc_student_em_weighted_workspace_bytes(n, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res = (C.c_double * 6)(*([-7.0] * 6))
    rc = lib.pmc_student_em_weighted(_lib.ptr(dx), None, _lib.ptr(dw), n, D, _lib.ptr(io), C.c_void_p(io.data_ptr() + 8 * D),
                                     1e-6, 100, res, _lib.ptr(ws), nbytes, _lib.stream_handle())
    torch.cuda.synchronize()
    assert rc != 0 and b"weights must be finite and non-negative" in lib.pmc_last_error()
    assert torch.equal(io, before) and list(res) == [-7.0] * 6


def test_rows_of_positive_weight_must_outnumber_the_dimensions():
    """|P| = D: ValueError.  |P| = D + 1 with equal weights: every distance is D, the rows are Gaussian to the fit, which
    leaves at its first iteration with the start values."""
    from pocomc_amd.geometry import student_em_weighted
    n, D = 40, 6
    x = sw.case_rows(n, D)
    rows = np.random.default_rng(0).permutation(n)
    for count in (D, D + 1):
        w = np.zeros(n)
        w[rows[:count]] = 2.5
        start = sw.start_values(x, w)
        if count == D:
            with pytest.raises(ValueError, match="needs more rows of positive weight than dimensions"):
                student_em_weighted(up(x), up(w), *start)
            continue
        ref = sw.fit(x, w, *start)
        assert ref["status"] == "nu_inf" and ref["iterations"] == 1
        mu, sigma, info = student_em_weighted(up(x), up(w), *start)
        assert info["status"] == "nu_inf" and info["iterations"] == 1 and info["nu"] == np.inf and info["host_reads"] == 2
        assert info["rows_positive"] == D + 1 and abs(info["ess"] - (D + 1)) < 1e-12
        assert np.array_equal(mu, start[0]) and np.array_equal(sigma, start[1])
    with pytest.raises(ValueError):
        student_em_weighted(up(x[:D]), up(np.ones(D)), *sw.start_values(x, np.ones(n)))       # n <= D: before any launch


def test_the_width_limit():
    from pocomc_amd import _lib
    from pocomc_amd.geometry import Geometry, student_em_weighted
    x = se.mvt_rows(1, 400, 158, 4.0)
    w = np.ones(400)
    with pytest.raises(ValueError, match="157"):
        student_em_weighted(up(x), up(w), *sw.start_values(x, w))
    g = Geometry(student="em_weighted")
    with pytest.raises(ValueError, match="157"):
        g.fit(x, w)
    assert g.t_mean is None and g.normal_mean is None
    lib = _lib.load()                                                         # the library's own refusal: nothing is launched
    res = (C.c_double * 6)()
    dx, dw = up(x), up(w)
    io = up(np.zeros(158 + 158 * 158))
    rc = lib.pmc_student_em_weighted(_lib.ptr(dx), None, _lib.ptr(dw), 400, 158, _lib.ptr(io), C.c_void_p(io.data_ptr() + 8 * 158),
                                     1e-6, 100, res, _lib.ptr(io), 1 << 40, _lib.stream_handle())
    assert rc != 0 and b"D > 157" in lib.pmc_last_error()


# ------------------------------------------------------------------------------------------------------- 6. Geometry
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_geometry_fits_on_the_weights(weighted, f32):
    """``normal_mean`` / ``normal_cov`` are the ``"em"`` mode's bit for bit; the t-fit is the restatement's from the
    weighted mean and the weighted scatter ``S / V1``; ``weights=None`` means ones."""
    from pocomc_amd.geometry import Geometry
    n, D = 2049, 6
    x = se.mvt_rows(13, n, D, 4.0, dtype=np.float32 if f32 else np.float64)
    w = sw.weights("zeros5", n, seed=2) if weighted else None
    wr = w if weighted else np.ones(n)
    ref = sw.fit(x, wr, *sw.start_values(x, wr))
    assert ref["status"] == "converged" and all(not (0.99e-6 <= s <= 1.01e-6) for s in ref["steps"][-2:])
    g, old = Geometry(student="em_weighted"), Geometry(student="em")
    g.fit(x, w)
    old.fit(x, w)
    assert np.array_equal(g.normal_mean, old.normal_mean) and np.array_equal(g.normal_cov, old.normal_cov)
    info = g.student_info
    print(f"Geometry em_weighted: {info}; em: {old.student_info}")
    assert set(info) == {"iterations", "status", "nu", "rows_positive", "ess"}
    assert info["status"] == "converged" and info["iterations"] == ref["iterations"] and g.t_nu == info["nu"]
    assert info["rows_positive"] == int((wr > 0).sum()) and abs(info["ess"] - sw.ess(wr)) < 1e-9 * n
    assert within("geometry", g.t_mean, g.t_cov, g.t_nu, ref)


def test_geometry_draws_no_random_number():
    import torch
    from pocomc_amd.geometry import Geometry
    n, D = 1024, 5
    x = se.mvt_rows(4, n, D, 4.0)
    w = sw.weights("lognormal1", n, seed=4)
    fits = {}
    for mode in ("em_weighted", "em"):
        for seed in (5, 6):
            np.random.seed(seed)
            torch.manual_seed(seed)
            s0, t0 = np.random.get_state(), torch.get_rng_state()
            g = Geometry(student=mode)
            g.fit(x, w)
            s1 = np.random.get_state()
            same = s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
            assert same == (mode == "em_weighted")
            assert torch.equal(torch.get_rng_state(), t0)
            fits[mode, seed] = (g.t_mean, g.t_cov, g.t_nu)
    a, b = fits["em_weighted", 5], fits["em_weighted", 6]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    a, b = fits["em", 5], fits["em", 6]
    print(f"nu: em_weighted {fits['em_weighted', 5][2]:.6f}; em under two seeds {a[2]:.6f}, {b[2]:.6f}")
    assert not np.array_equal(a[1], b[1]) and a[2] != b[2]


def test_geometry_refuses_what_both_other_modes_refuse():
    from pocomc_amd.geometry import Geometry
    g = Geometry(student="em_weighted")
    with pytest.raises(ValueError):
        g.fit(se.mvt_rows(1, 6, 6, 4.0))                                 # n <= D
    x = se.mvt_rows(1, 300, 6, 4.0)
    w = np.zeros(300)
    w[:6] = 1.0
    with pytest.raises(ValueError, match="rows of positive weight"):
        g.fit(x, w)                                                      # |P| = D
    w = np.ones(300)
    w[5] = -1.0
    with pytest.raises(ValueError):
        g.fit(x, w)
    bad = x.copy()
    bad[17, 3] = np.nan
    with pytest.raises(ValueError):
        g.fit(bad)
    with pytest.raises(np.linalg.LinAlgError):
        g.fit(se.collinear_rows())                                       # rank 2 in 8 dimensions: no factor of the scatter matrix
    assert g.t_mean is None and g.normal_mean is None and g.student_info is None
    g.fit(se.mvt_rows(3, 2048, 6, np.inf))                               # Gaussian rows: nu = inf -> 1e6
    assert g.t_nu == 1e6 and g.student_info["status"] == "nu_inf" and g.student_info["nu"] == np.inf


# -------------------------------------------------------------------------------------------------------- 7. Sampler
def test_sampler_run_on_the_pool_weights():
    """The Sampler run of ``tests/test_gpu_student_em.py`` in both EM modes; the resample-based mode's own deviation of logZ
    is the yardstick."""
    from test_gpu_student_em import run_sampler
    exact = -4 * np.log(40.0)
    out = {}
    for mode in ("em", "em_weighted"):
        s = run_sampler(mode)
        logz, _ = s.evidence()
        print(f"student_fit={mode!r}: u_geometry.t_nu {s.u_geometry.t_nu} {s.u_geometry.student_info} logZ {logz} "
              f"(deviation {logz - exact:+.4f})")
        out[mode] = (s, abs(logz - exact))
    s, dev = out["em_weighted"]
    assert s.student_fit == "em_weighted" and s.u_geometry.t_nu < 100
    assert {"rows_positive", "ess"} <= set(s.u_geometry.student_info)
    assert s.u_geometry.student_info["rows_positive"] > 4 and s.u_geometry.student_info["ess"] > 4
    assert dev <= max(0.75, 1.25 * out["em"][1])


# --------------------------------------------------------------------------------------- 8. a width the old mode refuses
def test_a_fit_at_d140_feeds_the_step():
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from test_gpu_mcmc import product_case
    D = 140
    x = se.mvt_rows(9, 400, D, 5.0)
    with pytest.raises(ValueError):
        Geometry(student="em").fit(x)
    g = Geometry(student="em_weighted")
    g.fit(x, np.random.default_rng(9).uniform(0.5, 1.5, size=400))
    print(f"D = 140: {g.student_info}")
    assert g.student_info["status"] in ("converged", "max_iter") and 2.0 < g.t_nu < 10.0      # (the restatement: 4.564)
    assert np.linalg.eigvalsh(g.t_cov).min() > 0
    state, funcs, opts, _ = product_case("pcn_d140", dict(kind="pcn", N=80, D=D, T=3, beta=0.5, nu=None, prior="mixed",
                                                          target="gauss", seed=301, n_max=2, geometry=g))
    np.random.seed(301)
    got = pmcmc.pcn(state, funcs, opts)
    assert got["steps"] == 2
    assert all(np.isfinite(got[k]).all() for k in ("u", "x", "logdetj", "logl", "logp"))
