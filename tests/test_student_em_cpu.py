"""The numpy / scipy restatement of the Student-t EM fit (``tests/student_em.py``) on inputs with a known answer, and the
parts of ``Geometry(student=...)`` that need no GPU."""
import pickle

import numpy as np
import pytest

import student_em as se


@pytest.mark.parametrize("seed,n,D,nu", [(1, 2048, 6, 4.0), (2, 1000, 32, 8.0)])
def test_restatement_recovers_nu(seed, n, D, nu):
    x = se.mvt_rows(seed, n, D, nu)
    r = se.fit(x, *se.start_values(x))
    print(f"t_{nu:g} rows {n} x {D}: nu = {r['nu']:.4f} after {r['iterations']} iterations ({r['status']})")
    assert r["status"] == "converged" and r["iterations"] < 100
    assert abs(r["nu"] - nu) < 0.15 * nu
    assert np.isfinite(r["mu"]).all() and np.linalg.eigvalsh(r["sigma"]).min() > 0


def test_restatement_leaves_gaussian_rows_at_the_first_iteration():
    x = se.mvt_rows(3, 2048, 6, np.inf)
    mu0, s0 = se.start_values(x)
    r = se.fit(x, mu0, s0)
    assert r["status"] == "nu_inf" and r["iterations"] == 1 and r["nu"] == np.inf
    assert np.array_equal(r["mu"], mu0) and np.array_equal(r["sigma"], s0)


def test_geometry_rejects_an_unknown_student_mode():
    from pocomc_amd.geometry import Geometry
    with pytest.raises(ValueError):
        Geometry(student="bogus")
    assert Geometry().student == "reference" and Geometry(student="em").student == "em"


def test_geometry_from_an_older_checkpoint_is_in_reference_mode():
    """A ``Geometry`` pickled before the attribute existed has no ``student`` in its state."""
    from pocomc_amd.geometry import Geometry
    g = Geometry()
    state = dict(g.__dict__)
    del state["student"], state["student_info"]
    old = Geometry.__new__(Geometry)
    old.__dict__.update(state)
    back = pickle.loads(pickle.dumps(old))
    assert "student" not in back.__dict__
    assert back.student == "reference" and back.student_info is None
