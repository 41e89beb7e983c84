"""``pmc_student_em`` (``csrc/student.hip``), ``Geometry(student="em")`` and ``Sampler(student_fit="em")`` against the
float64 numpy / scipy restatement of ``tests/student_em.py``.

Tolerance ``TOL = 1e-9`` (``mu`` relative to ``max|mu|``, ``Sigma`` to ``max|Sigma|``, ``nu`` to itself): the restatement
against itself with the rows permuted and its root tolerance loosened to 1e-11 moves by at most 1.8e-12 after 10
iterations on inputs of this kind, so 1e-9 leaves a factor of about 500 over the reference's own reordering noise and is
far below any algorithmic error.  ``-s`` prints the measured maxima (``profiles/student_em.txt``)."""
import functools

import numpy as np
import pytest

import student_em as se
from oracle import tools as otools

pytestmark = pytest.mark.gpu

TOL = 1e-9
MEASURED = {}          # test group -> largest relative deviation of (mu, Sigma, nu)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nstudent EM, device against the restatement: largest relative deviation of mu | Sigma | nu")
    for k, (a, b, c) in sorted(MEASURED.items()):
        print(f"  {k:28s} {a:9.2e} | {b:9.2e} | {c:9.2e}")


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def deviation(group, mu, sigma, nu, ref):
    e_mu = np.abs(mu - ref["mu"]).max() / np.abs(ref["mu"]).max()
    e_s = np.abs(sigma - ref["sigma"]).max() / np.abs(ref["sigma"]).max()
    e_nu = abs(nu - ref["nu"]) / ref["nu"] if np.isfinite(ref["nu"]) else float(nu != ref["nu"])
    m = MEASURED.setdefault(group, [0.0, 0.0, 0.0])
    m[:] = max(m[0], e_mu), max(m[1], e_s), max(m[2], e_nu)
    print(f"{group}: mu {e_mu:.2e} Sigma {e_s:.2e} nu {e_nu:.2e}")
    return max(e_mu, e_s, e_nu)


# ------------------------------------------------------------------------------------------ 1. fixed-length parity
# less than one wavefront; a row count that crosses the 64-row and 256-thread blocks by one; D off the 16-wide tiles;
# the LDS limit
SHAPES = [(37, 2), (300, 6), (2049, 33), (517, 64), (1000, 128)]


@functools.lru_cache(maxsize=None)
def parity_input(n, D, f32, indexed):
    """``(x, idx, rows)``: the pool, the selection (None: all rows) and the selected rows as the restatement sees them."""
    x = se.mvt_rows(100 + D, n + (11 if indexed else 0), D, 5.0, dtype=np.float32 if f32 else np.float64)
    if not indexed:
        return x, None, x
    idx = np.random.default_rng(n).integers(0, x.shape[0], size=n)       # repeats, out of order
    return x, idx, x[idx]


@functools.lru_cache(maxsize=None)
def parity_reference(n, D, f32, indexed, max_iter):
    rows = parity_input(n, D, f32, indexed)[2]
    start = se.start_values(rows)
    return start, se.fit(rows, *start, tol=0.0, max_iter=max_iter)


@pytest.mark.parametrize("max_iter", [1, 3, 10])
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "idx"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,D", SHAPES)
def test_fixed_length_parity(n, D, f32, indexed, max_iter):
    from pocomc_amd.geometry import student_em
    x, idx, _ = parity_input(n, D, f32, indexed)
    start, ref = parity_reference(n, D, f32, indexed, max_iter)
    assert ref["iterations"] == max_iter and ref["status"] == "max_iter"       # (the restatement: a condition on the input)
    mu, sigma, info = student_em(up(x), None if idx is None else up(idx), *start, tol=0.0, max_iter=max_iter)
    assert info["iterations"] == max_iter and info["status"] == "max_iter"
    assert info["host_reads"] == (max_iter + 7) // 8
    assert deviation(f"parity {n}x{D}", mu, sigma, info["nu"], ref) < TOL


# ------------------------------------------------------------------------------------------------ 2. converged fits
@pytest.mark.parametrize("seed,n,D,nu", [(21, 300, 2, 2.5), (12, 517, 10, 30.0), (13, 2049, 6, 4.0)])
def test_converged_fit_through_geometry(seed, n, D, nu):
    from pocomc_amd.geometry import Geometry
    x = se.mvt_rows(seed, n, D, nu)
    ref = se.fit(x, *se.start_values(x))
    print(f"restatement: nu {ref['nu']:.6f}, {ref['iterations']} iterations, last steps {ref['steps'][-2:]}")
    assert ref["status"] == "converged"
    # rounding cannot move the stopping iteration: the last two |delta nu| are clear of the tolerance
    assert all(not (0.99e-6 <= s <= 1.01e-6) for s in ref["steps"][-2:])
    g = Geometry(student="em")
    g.fit(x)
    assert g.student_info["status"] == "converged" and g.student_info["iterations"] == ref["iterations"]
    assert g.t_nu == g.student_info["nu"]
    assert deviation("converged", g.t_mean, g.t_cov, g.t_nu, ref) < TOL


# ------------------------------------------------------------------------------------------------- 3. Gaussian rows
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("seed,n,D", [(3, 2048, 6), (7, 64, 2)])
def test_gaussian_rows_give_the_reference_geometry(seed, n, D, f32, weighted):
    from pocomc_amd.geometry import Geometry
    x = se.mvt_rows(seed, n, D, np.inf, dtype=np.float32 if f32 else np.float64)
    w = None
    rows = x
    if weighted:
        w = np.random.default_rng(seed).uniform(0.5, 1.5, size=n)
        w /= w.sum()
        np.random.seed(5)
        rows = x[otools.systematic_resample(n, w)]
    r = se.fit(rows, *se.start_values(rows))
    assert r["status"] == "nu_inf" and r["iterations"] == 1             # (the restatement: a condition on the input)
    out = []
    for mode in ("reference", "em"):
        g = Geometry(student=mode)
        np.random.seed(5)
        g.fit(x, w)
        out.append(g)
        assert g.t_nu == 1e6
    ref, em = out
    assert em.student_info == dict(iterations=1, status="nu_inf", nu=np.inf) and ref.student_info is None
    assert np.array_equal(em.t_mean, ref.t_mean) and np.array_equal(em.t_cov, ref.t_cov)
    assert np.array_equal(em.normal_mean, ref.normal_mean) and np.array_equal(em.normal_cov, ref.normal_cov)


# --------------------------------------------------------------------------------------------------- 4. status paths
def test_max_iter_status():
    from pocomc_amd.geometry import student_em
    x = se.mvt_rows(13, 2049, 6, 4.0)
    start = se.start_values(x)
    ref = se.fit(x, *start, max_iter=5)
    assert ref["status"] == "max_iter" and ref["iterations"] == 5
    mu, sigma, info = student_em(up(x), None, *start, max_iter=5)
    assert info["status"] == "max_iter" and info["iterations"] == 5 and info["host_reads"] == 1
    assert deviation("max_iter", mu, sigma, info["nu"], ref) < TOL


def test_lower_clamp_status():
    from pocomc_amd.geometry import Geometry
    x = se.mvt_rows(5, 1024, 2, 0.05)
    ref = se.fit(x, *se.start_values(x))
    assert ref["status"] == "lower_clamp" and ref["nu"] == se.NU_LO      # (every Cholesky of the restatement succeeded)
    g = Geometry(student="em")
    g.fit(x)
    assert g.student_info["status"] == "lower_clamp" and g.student_info["iterations"] == ref["iterations"]
    assert g.t_nu == se.NU_LO
    assert deviation("lower clamp", g.t_mean, g.t_cov, g.t_nu, ref) < TOL


def test_bad_input_raises():
    from pocomc_amd.geometry import Geometry
    g = Geometry(student="em")
    with pytest.raises(ValueError):
        g.fit(se.mvt_rows(1, 6, 6, 4.0))                                 # n <= D
    with pytest.raises(ValueError):
        g.fit(se.mvt_rows(1, 400, 129, 4.0))                             # D above the LDS limit
    x = se.mvt_rows(1, 300, 6, 4.0)
    x[17, 3] = np.nan
    with pytest.raises(ValueError):
        g.fit(x)                                                         # the check in front of both modes
    assert g.t_mean is None


# ----------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_same_bits_on_every_call_and_through_idx(f32):
    from pocomc_amd.geometry import student_em
    x, idx, rows = parity_input(2049, 33, f32, True)
    start = se.start_values(rows)
    a = student_em(up(x), up(idx), *start)
    b = student_em(up(x), up(idx), *start)
    c = student_em(up(rows), None, *start)
    assert a[2]["status"] == "converged" and a[2]["iterations"] > 8
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2] == other[2]


# ------------------------------------------------------------------------------------------------------- 6. Sampler
def t3_loglike(x):
    """Log-density of a standard 4-variate t with 3 degrees of freedom, row-wise."""
    from scipy.special import gammaln
    nu, D = 3.0, 4
    c = gammaln((nu + D) / 2) - gammaln(nu / 2) - 0.5 * D * np.log(nu * np.pi)
    return c - 0.5 * (nu + D) * np.log1p(np.sum(x * x, axis=1) / nu)


def run_sampler(student_fit):
    from scipy.stats import uniform
    import pocomc_amd as pc
    prior = pc.Prior(4 * [uniform(-20.0, 40.0)])
    s = pc.Sampler(prior=prior, likelihood=t3_loglike, vectorize=True, precondition=False, sample="tpcn",
                   student_fit=student_fit, n_effective=256, n_active=128, random_state=0)
    s.run(n_total=512, n_evidence=0)
    return s


def test_sampler_run_uses_a_finite_nu():
    s = run_sampler("em")
    logz, _ = s.evidence()
    print("student_fit='em': u_geometry.t_nu", s.u_geometry.t_nu, s.u_geometry.student_info, "logZ", logz)
    assert s.u_geometry.t_nu < 100
    # the likelihood is normalised and all but 2e-4 of its mass lies in the box: logZ = -log(40^4)
    assert abs(logz - (-4 * np.log(40.0))) < 0.75


def test_sampler_reference_mode_keeps_the_gaussian_step():
    s = run_sampler("reference")
    assert s.u_geometry.t_nu == 1e6 and s.u_geometry.student_info is None


def test_sampler_rejects_an_unknown_mode():
    from scipy.stats import uniform
    import pocomc_amd as pc
    with pytest.raises(ValueError):
        pc.Sampler(prior=pc.Prior(4 * [uniform(-20.0, 40.0)]), likelihood=t3_loglike, vectorize=True, student_fit="x")
