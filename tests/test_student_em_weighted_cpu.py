"""The numpy / scipy restatement of the weighted Student-t EM fit (``tests/student_em_weighted.py``) against the unweighted
one on repeated rows, its own reordering noise on every case of ``tests/test_gpu_student_em_weighted.py``, the weighted
fit against the resample-based one, and the parts of the ``"em_weighted"`` option that need no GPU."""
import numpy as np
import pytest

import student_em as se
import student_em_weighted as sw


def deviation(a, b):
    return (abs(a["nu"] - b["nu"]) / b["nu"], np.abs(a["mu"] - b["mu"]).max() / np.abs(b["mu"]).max(),
            np.abs(a["sigma"] - b["sigma"]).max() / np.abs(b["sigma"]).max())


@pytest.mark.parametrize("seed,n,D,nu", [(1, 300, 6, 4.0), (2, 517, 33, 5.0), (3, 400, 128, 5.0)])
def test_integer_weights_are_repeated_rows(seed, n, D, nu):
    """``pi_r = k_r / sum k`` is what ``1 / n`` gives the row when it is there ``k_r`` times: the two restatements agree to
    rounding, with the same iteration count."""
    x = se.mvt_rows(seed, n, D, nu)
    k = np.random.default_rng(seed).integers(0, 4, size=n)
    start = sw.start_values(x, k.astype(np.float64))
    a = sw.fit(x, k.astype(np.float64), *start)
    b = se.fit(np.repeat(x, k, axis=0), *start)
    d = deviation(a, b)
    print(f"{n} x {D}: {a['status']} after {a['iterations']} | {b['iterations']} iterations, nu {a['nu']:.4f}; deviation nu "
          f"{d[0]:.1e} mu {d[1]:.1e} Sigma {d[2]:.1e}; {a['rows_positive']} rows of positive weight")
    assert a["rows_positive"] == int((k > 0).sum()) > D
    assert a["status"] == b["status"] and a["iterations"] == b["iterations"] > 1
    assert max(d) < 1e-12


@pytest.mark.parametrize("n,D", sw.SHAPES)
def test_the_restatement_is_quiet_on_every_case_of_the_device_tests(n, D):
    """``reorder_noise`` of every regime and length at this shape is below 2e-12 -- ``se.tolerances`` then gives the device
    tests the 1e-9 floor -- or is the figure recorded in ``sw.NOISE``, which gives them 500 times that.  Every case has more
    rows of positive weight than dimensions and runs at least one full iteration."""
    x = sw.case_rows(n, D)
    for regime in sw.REGIMES:
        w = sw.case_weights(n, D, regime)
        assert int((w > 0).sum()) > D and np.isfinite(w).all() and (w >= 0).all()
        start = sw.start_values(x, w)
        for k, (tol, max_iter) in enumerate(sw.LENGTHS):
            r = sw.fit(x, w, *start, tol=tol, max_iter=max_iter)
            assert r["status"] in ("converged", "max_iter", "lower_clamp") and r["iterations"] >= 1
            m = sw.reorder_noise(x, w, *start, tol=tol, max_iter=max_iter)
            rec = sw.NOISE.get((n, D, regime, k))
            print(f"{n} x {D} {regime:10s} {tol:g}/{max_iter}: {r['status']} after {r['iterations']}, nu {r['nu']:.4g}; reorder noise "
                  f"nu {m[0]:.2e} mu {m[1]:.2e} Sigma {m[2]:.2e}" + (f"; recorded {rec}" if rec else ""))
            if rec is None:
                assert max(m) < 2e-12, (regime, k, m)
            else:
                assert all(a <= b for a, b in zip(m, rec)), (regime, k, m, rec)       # (the recorded figures bound the measured)
                assert all(b <= 8.0 * a + 1e-15 for a, b in zip(m, rec)), (regime, k, m, rec)   # (and are no slack of their own)


def test_the_regimes_are_what_they_say():
    n = 640
    w = {r: sw.weights(r, n, seed=3) for r in sw.REGIMES}
    assert set(w) == set(sw.REGIMES) and all(v.shape == (n,) and (v >= 0).all() for v in w.values())
    assert np.all(w["uniform"] == 1.0)
    assert (w["zeros5"] == 0).sum() == n // 20
    assert abs(w["half_mass"].max() / w["half_mass"].sum() - 0.5) < 1e-12
    assert set(np.unique(w["integer"])) == {0.0, 1.0, 2.0, 3.0}
    zero = np.flatnonzero(w["chunk_zero"] == 0)
    assert len(zero) == n // 64 and zero[0] % (n // 64) == 0 and np.all(np.diff(zero) == 1)
    assert sw.ess(w["lognormal3"]) < 0.1 * sw.ess(w["lognormal1"]) < 0.1 * n


@pytest.mark.parametrize("args", sw.POOLS)
def test_the_weighted_nu_lies_among_the_resampled_ones(args):
    """The fit on the weights gives a nu inside the range of the fits on systematic resamples of the same weights over 16
    offsets: it is the quantity the resample-based mode estimates with one random draw."""
    x, w = sw.pool(*args)
    n = x.shape[0]
    a = sw.fit(x, w, *sw.start_values(x, w))
    nus = []
    for off in np.linspace(0.03, 0.97, 16):
        rows = x[sw.systematic_indices(n, w, off)]
        nus.append(se.fit(rows, *se.start_values(rows))["nu"])
    nus = np.array(nus)
    print(f"{args}: Kish ESS {sw.ess(w):.0f}, weighted nu {a['nu']:.4f} ({a['status']}, {a['iterations']} iterations); resampled nu "
          f"{nus.min():.3f} ... {nus.max():.3f}, standard deviation {nus.std():.3f}")
    assert a["status"] == "converged"
    assert nus.min() < a["nu"] < nus.max()


def test_the_option_is_accepted():
    """Fails on the parent commit, where ``"em_weighted"`` is an invalid value."""
    import torch
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import _lib
    from pocomc_amd.geometry import Geometry
    g = Geometry(student="em_weighted")
    assert g.student == "em_weighted" and g.student_info is None and g.t_mean is None
    with pytest.raises(ValueError):
        Geometry(student="em-weighted")
    kw = dict(prior=pc.Prior(4 * [uniform(-20.0, 40.0)]), likelihood=lambda x: -0.5 * np.sum(x * x, axis=1), vectorize=True,
              n_effective=64, n_active=32)
    with pytest.raises(ValueError):
        pc.Sampler(student_fit="em-weighted", **kw)
    try:
        s = pc.Sampler(student_fit="em_weighted", **kw)
    except _lib.PocomcAmdError:                        # past the check of the option: the constructor then asks for the GPU
        assert not torch.cuda.is_available()
    else:
        assert s.student_fit == "em_weighted" and s.u_geometry.student == s.theta_geometry.student == "em_weighted"


def test_the_library_exports_the_weighted_entry():
    """Fails on the parent commit: the symbol is absent."""
    from pocomc_amd import _lib
    lib = _lib.load()
    assert lib.pmc_student_em_weighted_workspace_bytes(1000, 157) == lib.pmc_student_em_workspace_bytes(1000, 157) > 0
    assert lib.pmc_student_em_weighted_workspace_bytes(0, 4) == 0
    assert hasattr(lib, "pmc_student_em_weighted")
