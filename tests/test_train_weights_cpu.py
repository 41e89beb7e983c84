"""Which of a run's weight regimes a float32 trainer can be held to (``tests/train_weights.py``), without a GPU: for every
(fixture, regime) ``tests/test_gpu_train_weights.py`` keeps, the float64 autograd reference is finite and ``C e`` -- the
envelope of ``test_trainer_loss_and_gradient_per_block`` -- stays at or below 1e-3 in every parameter block.  The gain-4
fixtures are those of the GPU test; the flows ``Flow.fit`` trains there are stood in for by the torch twin's
(``flow_regimes.twin_trained``), and the GPU test asserts the same condition on the fitted flows themselves."""
import numpy as np
import pytest

import flow_regimes as fr
import pool_regimes as pr
import train_weights as tw
from pocomc_amd.maf_spec import MAFSpec

FIXTURES = {"maf3-d10-fit": "maf3-trained", "nsf6-d10-fit": "nsf6-trained", "maf3-d10-g4": "maf3-g4", "nsf6-d10-g4": "nsf6-g4"}


def fixture(name):
    if name.endswith("trained"):
        spec, flat = fr.twin_trained(name.split("-")[0])
        return spec, flat, fr.two_modes(10, 1000, 9)
    spec = MAFSpec(10, 3) if name.startswith("maf3") else MAFSpec(10, 6, univariate="rqs")
    return spec, fr.gain_params(spec, 4.0), fr.two_modes(10, 1000, 9) * np.float32(1.3)


@pytest.mark.parametrize("regime", tw.REGIMES)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_kept_regimes_have_a_finite_reference_and_a_small_envelope(name, regime):
    spec, flat, data = fixture(FIXTURES[name])
    got = tw.pick(spec, flat, data, regime)
    assert ((name, regime) in tw.DROPPED) == (got is None)
    if got is not None:
        seed, x, w = got
        finite, ce = tw.condition(spec, flat, x, w)
        print(f"{name} {regime}: seed {seed}, reference finite {finite}, C e {ce:.2e}")
        assert finite and ce <= tw.CE_MAX


def test_the_weights_are_a_runs():
    for regime in tw.REGIMES:
        w = tw.run_weights(regime)
        assert w.dtype == np.float32 and w.shape == (tw.N,) and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    assert (tw.run_weights("holes") == 0).sum() == tw.N // 10 and (tw.run_weights("one_hot") != 0).sum() == 1
    assert np.ptp(tw.run_weights("equal")) == 0
    w = tw.run_weights("wide")
    assert w[w > 0].min() < 1e-20 * w.max()
    x = np.arange(300, dtype=np.float32).reshape(100, 3)
    xs, ws, k = tw.zero_rows_last(x, tw.run_weights("holes"))
    assert k == 90 and (ws[:k] != 0).all() and not ws[k:].any() and (np.diff(xs[:k, 0]) > 0).all()


def test_the_validation_reference_and_its_bound():
    lp, w = -np.arange(1.0, 101.0), tw.run_weights("holes")
    tot, mag = tw.valid_reference(lp, w, [np.arange(0, 40), np.arange(40, 80), np.arange(80, 100)])
    assert np.isfinite(tot) and 0 < tot <= mag * (1 + 1e-12)
    assert np.isnan(tw.valid_reference(lp, tw.run_weights("one_hot"), [np.arange(0, 40), np.arange(40, 100)])[0])
    assert tw.valid_bound(40, 3) == (2 * 9 + 3 + 3) * 2.0 ** -24
