"""``pmc_student_em`` (``csrc/student.hip``) where ``tests/test_gpu_student_em.py`` does not go: D = 1 and D across the 16-wide
tiles, fewer rows than one wavefront, ``n = D + 1``, first roots of f(nu) in every decade of [0.1, 1e4], fits that end above
nu = 300 or below 1, and every status the fit can end with -- ``not_pd`` and ``nonfinite`` through ``student_em`` itself,
which hands back what ``Geometry.fit`` turns into an exception.

The reference is the float64 numpy / scipy restatement (``tests/student_em.py``); ``tests/test_student_em_cpu.py`` holds the
conditions on every input with it.  Tolerances: ``TOL = 1e-9`` as in ``tests/test_gpu_student_em.py``, except where the
restatement itself moves by more than 1e-9 / 500 when its rows come in another order (``student_em.reorder_noise``, measured
on the CPU and recorded next to the input in ``student_em.NU_AXIS`` / ``LARGE_NU``): there it is 500 times that figure, per
input and per quantity.  Above nu of a few hundred the restatement is the noisy side: it forms ``log(nu/2) - psi(nu/2)``
from two numbers near 6, the device sums the difference directly.  ``-s`` prints the measured maxima per group
(``profiles/student_em.txt``)."""
import functools

import numpy as np
import pytest

import student_em as se
from test_gpu_student_em import MEASURED, TOL, deviation, report, up      # noqa: F401  (report: the module's -s table)

pytestmark = pytest.mark.gpu


def within(group, mu, sigma, nu, ref, d):
    """The measured-noise rule: nu, mu and Sigma each inside ``max(1e-9, 500 d)`` of the restatement."""
    deviation(group, mu, sigma, nu, ref)
    t_nu, t_mu, t_s = se.tolerances(d)
    e_nu = abs(nu - ref["nu"]) / ref["nu"]
    e_mu = np.abs(mu - ref["mu"]).max() / np.abs(ref["mu"]).max()
    e_s = np.abs(sigma - ref["sigma"]).max() / np.abs(ref["sigma"]).max()
    print(f"{group}: bounds nu {t_nu:.1e} mu {t_mu:.1e} Sigma {t_s:.1e}")
    return e_nu < t_nu and e_mu < t_mu and e_s < t_s


# ------------------------------------------------------------------------------------- a. tile and block edges
@functools.lru_cache(maxsize=None)
def edge_input(n, D, f32, indexed):
    return se.edge_rows(n, D, f32, indexed)


@functools.lru_cache(maxsize=None)
def edge_reference(n, D, f32, indexed, max_iter):
    rows = edge_input(n, D, f32, indexed)[2]
    start = se.start_values(rows)
    return start, se.fit(rows, *start, tol=0.0, max_iter=max_iter)


@pytest.mark.parametrize("max_iter", [1, 4])
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "idx"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,D", se.EDGE_SHAPES)
def test_fixed_length_parity_at_tile_and_block_edges(n, D, f32, indexed, max_iter):
    from pocomc_amd.geometry import student_em
    x, idx, _ = edge_input(n, D, f32, indexed)
    start, ref = edge_reference(n, D, f32, indexed, max_iter)
    assert ref["iterations"] == max_iter and ref["status"] == "max_iter"       # (the restatement: a condition on the input)
    mu, sigma, info = student_em(up(x), None if idx is None else up(idx), *start, tol=0.0, max_iter=max_iter)
    assert info["iterations"] == max_iter and info["status"] == "max_iter"
    assert info["host_reads"] == (max_iter + 7) // 8
    assert deviation(f"edge {n}x{D}", mu, sigma, info["nu"], ref) < TOL


# --------------------------------------------------------------------------------------------------- b. n = D + 1
@pytest.mark.parametrize("args", [(1, 3, 2, 4), (1, 7, 6, 4), (3, 129, 128, 5)], ids=["3x2", "7x6", "129x128"])
def test_one_row_more_than_dimensions(args):
    from pocomc_amd.geometry import student_em
    x = se.mvt_rows(*args)
    mu0, s0 = se.start_values(x)
    ref = se.fit(x, mu0, s0)
    assert ref["status"] == "nu_inf" and ref["iterations"] == 1                # (the restatement: a condition on the input)
    mu, sigma, info = student_em(up(x), None, mu0, s0)
    assert info["status"] == "nu_inf" and info["iterations"] == 1 and info["nu"] == np.inf and info["host_reads"] == 1
    assert np.array_equal(mu, mu0) and np.array_equal(sigma, s0)               # "mu / Sigma as they are"


# ----------------------------------------------------------------------------------- c. the nu axis, one iteration
@functools.lru_cache(maxsize=None)
def axis_reference(k):
    args, c, _, _ = se.NU_AXIS[k]
    x = se.mvt_rows(*args)
    start = se.scaled_start(x, c)
    return x, start, se.fit(x, *start, tol=0.0, max_iter=1)


@pytest.mark.parametrize("k", range(len(se.NU_AXIS)), ids=[f"nu{r:g}" for _, _, r, _ in se.NU_AXIS])
def test_first_root_along_the_nu_axis(k):
    from pocomc_amd.geometry import student_em
    _, _, root, d = se.NU_AXIS[k]
    x, start, ref = axis_reference(k)
    assert ref["status"] == "max_iter" and abs(ref["nu"] - root) < 1e-5 * root  # (the restatement: a condition on the input)
    mu, sigma, info = student_em(up(x), None, *start, tol=0.0, max_iter=1)
    assert info["status"] == "max_iter" and info["iterations"] == 1 and info["host_reads"] == 1
    decade = int(np.floor(np.log10(root)))
    assert 10.0 ** decade <= info["nu"] <= 10.0 ** (decade + 1)                # (the device returned this decade)
    assert within(f"nu axis 1e{decade:+d}", mu, sigma, info["nu"], ref, d)


# ------------------------------------------------------------------------------------ d. large-nu fits to the end
@functools.lru_cache(maxsize=None)
def large_reference(k):
    x = se.mvt_rows(*se.LARGE_NU[k][0])
    start = se.start_values(x)
    return x, start, se.fit(x, *start)


@pytest.mark.parametrize("k", range(len(se.LARGE_NU)), ids=["s%d_t%g" % (a[0], a[3]) for a, _, _ in se.LARGE_NU])
def test_large_nu_fit_runs_to_the_end(k):
    """The VALUE of nu is compared, not the stopping iteration: above nu of about 1000 the last steps |delta nu| sit at the
    tolerance's size and rounding decides whether the loop stops at 22 or runs to 100 (the restatement itself does either,
    depending on the order of the rows)."""
    from pocomc_amd.geometry import student_em
    args, nu, d = se.LARGE_NU[k]
    x, start, ref = large_reference(k)
    assert ref["status"] in ("converged", "max_iter") and abs(ref["nu"] - nu) < 1e-5 * nu
    mu, sigma, info = student_em(up(x), None, *start)
    print(f"{args}: iterations device {info['iterations']} ({info['status']}), restatement {ref['iterations']} ({ref['status']}); "
          f"nu device {info['nu']:.10g}, restatement {ref['nu']:.10g}")
    assert info["status"] in ("converged", "max_iter")
    assert info["host_reads"] == -(-info["iterations"] // 8)
    assert within("large nu", mu, sigma, info["nu"], ref, d)


# -------------------------------------------------------------------------------------------------- e. heavy tails
@pytest.mark.parametrize("args", [(4, 1024, 3, 1), (3, 65, 1, 1)], ids=["1024x3", "65x1"])
def test_converged_fit_below_nu_one(args):
    from pocomc_amd.geometry import student_em
    x = se.mvt_rows(*args)
    start = se.start_values(x)
    ref = se.fit(x, *start)
    assert ref["status"] == "converged" and 0.8 < ref["nu"] < 1.0 and 68 <= ref["iterations"] <= 76
    # rounding cannot move the stopping iteration: the last two |delta nu| are clear of the tolerance
    assert all(not (0.99e-6 <= s <= 1.01e-6) for s in ref["steps"][-2:])
    mu, sigma, info = student_em(up(x), None, *start)
    assert info["status"] == "converged" and info["iterations"] == ref["iterations"]
    assert info["host_reads"] == -(-ref["iterations"] // 8) and info["host_reads"] in (9, 10)
    assert 0.1 <= info["nu"] < 1.0
    assert deviation("heavy tails", mu, sigma, info["nu"], ref) < TOL


def test_lower_clamp_at_the_second_iteration():
    from pocomc_amd.geometry import student_em
    x = se.mvt_rows(4, 1024, 3, 0.3)
    start = se.start_values(x)
    ref = se.fit(x, *start)
    assert ref["status"] == "lower_clamp" and ref["iterations"] == 2 and ref["nu"] == se.NU_LO
    mu, sigma, info = student_em(up(x), None, *start)
    assert info["status"] == "lower_clamp" and info["iterations"] == 2 and info["nu"] == se.NU_LO and info["host_reads"] == 1
    assert deviation("lower clamp at 2", mu, sigma, info["nu"], ref) < TOL


# ------------------------------------------------------------------------------------------------- f. status exits
def pd_start(D=4):
    x = se.mvt_rows(8, 120, D, 4.0)
    return (x,) + se.start_values(x)


def bad_sigmas():
    _, _, s0 = pd_start()
    out = {}
    for name, v in (("zero first pivot", 0.0), ("negative first pivot", -1.0)):
        s = s0.copy(); s[0, 0] = v
        out[name] = s
    # a non-positive LAST pivot: the diagonal's last element below what the first three pivots take from it
    s = s0.copy()
    schur = s0[3, 3] - s0[3, :3] @ np.linalg.solve(s0[:3, :3], s0[:3, 3])
    s[3, 3] = s0[3, 3] - 1.05 * schur                                          # (the pivot: -0.05 of the true one)
    out["negative last pivot"] = s
    for name, v in (("nan diagonal", np.nan), ("inf diagonal", np.inf)):
        s = s0.copy(); s[2, 2] = v
        out[name] = s
    return out


@pytest.mark.parametrize("which", ["zero first pivot", "negative first pivot", "negative last pivot", "nan diagonal", "inf diagonal"])
def test_not_pd_at_the_first_iteration_leaves_the_start_values(which):
    from pocomc_amd.geometry import student_em
    x, mu0, _ = pd_start()
    s = bad_sigmas()[which]
    if which == "negative last pivot":
        assert np.all(np.diag(s) > 0) and np.linalg.eigvalsh(s[:3, :3]).min() > 0
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(s)
    mu, sigma, info = student_em(up(x), None, mu0, s)
    assert info["status"] == "not_pd" and info["iterations"] == 1 and info["host_reads"] == 1
    assert np.array_equal(mu, mu0) and np.array_equal(sigma, s, equal_nan=True)


def test_not_pd_at_the_second_iteration_keeps_the_first_iterations_result():
    from pocomc_amd.geometry import student_em
    x = se.collinear_rows()
    mu0, s0 = se.start_values(x)
    s0 = s0 + np.eye(x.shape[1])
    ref = se.fit(x, mu0, s0)
    assert ref["status"] == "not_pd" and ref["iterations"] == 2                # (the restatement: a condition on the input)
    mu, sigma, info = student_em(up(x), None, mu0, s0)
    assert info["status"] == "not_pd" and info["iterations"] == 2 and info["host_reads"] == 1
    assert deviation("not_pd at 2", mu, sigma, info["nu"], ref) < TOL


def test_geometry_raises_on_the_collinear_rows():
    from pocomc_amd.geometry import Geometry
    x = se.collinear_rows()
    ref = se.fit(x, *se.start_values(x))
    assert ref["status"] == "not_pd" and ref["iterations"] == 2                # (from Geometry.fit's own start values)
    g = Geometry(student="em")
    with pytest.raises(np.linalg.LinAlgError, match="EM iteration 2"):
        g.fit(x)
    assert g.t_mean is None and g.t_cov is None and g.t_nu is None


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_nonfinite_row_ends_the_fit_and_an_unselected_one_does_not(bad):
    """65 rows: the bad value sits in the last one, alone in the second wavefront of ``em_delta_kernel``."""
    from pocomc_amd.geometry import student_em
    clean = se.mvt_rows(9, 65, 3, 4.0)
    mu0, s0 = se.start_values(clean)
    x = clean.copy()
    x[64, 1] = bad
    mu, sigma, info = student_em(up(x), None, mu0, s0)
    assert info["status"] == "nonfinite" and info["iterations"] == 1 and info["host_reads"] == 1
    assert np.array_equal(mu, mu0) and np.array_equal(sigma, s0)
    # the bad row of a larger pool reached through idx only: last of the 65 selected ...
    pool = np.vstack([clean[:64], se.mvt_rows(10, 5, 3, 4.0), x[64:]])          # rows 0..63 clean, 64..68 other, 69 bad
    sel = np.concatenate([np.arange(64), [69]])
    mu, sigma, info = student_em(up(pool), up(sel), mu0, s0)
    assert info["status"] == "nonfinite" and info["iterations"] == 1
    assert np.array_equal(mu, mu0) and np.array_equal(sigma, s0)
    # ... and present but not selected: the fit of the clean rows, bit for bit
    pool = np.vstack([clean[:30], x[64:], clean[30:]])                          # the bad row at 30
    sel = np.concatenate([np.arange(30), np.arange(31, 66)])
    a = student_em(up(pool), up(sel), mu0, s0)
    b = student_em(up(clean), None, mu0, s0)
    assert b[2]["status"] in ("converged", "max_iter") and b[2]["iterations"] > 1
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# -------------------------------------------------------------------------------------------------- g. determinism
def test_same_bits_on_every_call_at_large_nu_and_at_the_lds_limit():
    from pocomc_amd.geometry import student_em
    x, start, _ = large_reference(0)
    a, b = student_em(up(x), None, *start), student_em(up(x), None, *start)
    assert a[2]["iterations"] > 8
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    x, idx, _ = edge_input(200, 128, False, True)
    start, _ = edge_reference(200, 128, False, True, 4)
    a, b = (student_em(up(x), up(idx), *start, tol=0.0, max_iter=4) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
