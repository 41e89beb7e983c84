"""The trainer and the validation pass on a run's weights (``tests/train_weights.py``): importance weights normalised to
sum 1 in float32 -- orders of magnitude apart, denormal, exactly 0, all but one 0 -- where every other weighted test of
the suite draws ``w ~ U(0.1, 1)``.

* ``pmc_maf_loss_grad`` against float64 autograd of ``torch_loss`` under the criterion of
  ``test_trainer_loss_and_gradient_per_block`` (its own function, not a restatement), on the rows and weights the CPU
  condition keeps (``train_weights.pick``: finite reference, ``C e <= 1e-3`` in every block);
* rows of weight 0 leave loss and gradient bit for bit those of the batch without them (the rows that count keep their
  order and their positions in the 16-row sets: the zero rows sit behind them);
* ``pmc_maf_valid_epoch`` (with and without a permutation, batches of 40 on 100 rows) and ``pmc_neg_weighted_sum`` against
  the float64 sum formed from the device's own log-densities, relative to ``sum |terms|`` (``train_weights.valid_bound``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_flow_regimes as gfr
import train_weights as tw

pytestmark = pytest.mark.gpu

FIXTURES = ["maf3-d10-fit", "nsf6-d10-fit", "maf3-d10-g4", "nsf6-d10-g4"]
RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIO):
        print(f"\ntrain weights, largest deviation / bound, {k}: {RATIO[k]:.3f}", end="")


def picked(name, regime):
    spec, flat, data = gfr.fixture(name)
    got = tw.pick(spec, flat, data, regime)
    assert ((name, regime) in tw.DROPPED) == (got is None), f"{name} {regime}: no seed meets the CPU condition"
    return spec, flat, got


@pytest.mark.parametrize("regime", tw.REGIMES)
@pytest.mark.parametrize("name", FIXTURES)
def test_trainer_on_a_runs_weights(name, regime):
    spec, flat, got = picked(name, regime)
    if got is None:
        return
    seed, x, w = got
    gfr._loss_and_gradient(spec, flat, gfr.flow(spec, flat), x, w, True, f"trainer, {name} {regime} weights (seed {seed})")


@pytest.mark.parametrize("regime", ["holes", "one_hot", "very_wide"])
@pytest.mark.parametrize("name", FIXTURES)
def test_rows_of_weight_zero_do_not_count(name, regime):
    from pocomc_amd.train import loss_and_grad, _train_state
    spec, flat, got = picked(name, regime)
    if got is None:
        return
    seed, x, w = got
    xs, ws, k = tw.zero_rows_last(x, w)
    assert 0 < k < tw.N and not ws[k:].any() and (ws[:k] != 0).all()
    f = gfr.flow(spec, flat)
    _train_state(f).repack(f)
    out = []
    for n in (tw.N, k):
        loss = loss_and_grad(f, torch.from_numpy(xs[:n].copy()).cuda(), torch.from_numpy(ws[:n].copy()).cuda())
        out.append((np.float32(loss.item()), f._train.grad.cpu().numpy().copy()))
    (la, ga), (lb, gb) = out
    assert np.isfinite(la) and np.isfinite(ga).all() and np.abs(ga).max() > 0
    assert la.view(np.uint32) == lb.view(np.uint32), f"{name} {regime}: loss {la!r} with the zero rows, {lb!r} without"
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), f"{name} {regime}: {k} rows count, the gradient differs in its bits"


@pytest.mark.parametrize("regime", tw.REGIMES)
@pytest.mark.parametrize("name", FIXTURES)
def test_validation_sums_on_a_runs_weights(name, regime):
    from pocomc_amd import _lib
    spec, flat, data = gfr.fixture(name)
    f = gfr.flow(spec, flat)
    n, bs = tw.N, 40
    x, w = tw.rows(data), tw.run_weights(regime)
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    scratch = torch.empty(n, dtype=torch.float32, device="cuda")
    acc = torch.zeros(1, dtype=torch.float32, device="cuda")
    starts = range(0, n, bs)
    for perm in (None, np.random.default_rng(4).permutation(n)):
        pd = None if perm is None else torch.from_numpy(perm).cuda()
        acc.zero_()
        _lib.check(f.lib.pmc_maf_valid_epoch(C.byref(f._desc), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(pd), n, bs, _lib.ptr(scratch),
                                             _lib.ptr(acc), _lib.stream_handle()), "pmc_maf_valid_epoch")
        lp = scratch.cpu().numpy()                                  # (in batch order: position i holds row perm[i])
        order = np.arange(n) if perm is None else perm
        assert np.isfinite(lp).all()
        ref, mag = tw.valid_reference(lp, w[order], [np.arange(b0, min(b0 + bs, n)) for b0 in starts])
        got = float(acc.item())
        tag = f"{name} {regime} perm={perm is not None}: device {got!r}, float64 {ref!r}, sum |terms| {mag!r}"
        print(tag)
        if not np.isfinite(ref):                                    # a batch of weight 0: 0 / 0 here as in the reference
            assert np.isnan(ref) and np.isnan(got), tag
            continue
        r = abs(got - ref) / (tw.valid_bound(bs, len(starts)) * mag)
        RATIO["validation epoch"] = max(RATIO.get("validation epoch", 0.0), r)
        assert r <= 1.0, tag
    # the per-batch path: pmc_sum_f32 + pmc_neg_weighted_sum over the 100 rows as one batch
    lp = f.log_prob(torch.from_numpy(x)).to(torch.float32).cuda().contiguous()
    ws, out = torch.zeros(1, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.float32, device="cuda")
    _lib.check(f.lib.pmc_sum_f32(_lib.ptr(wd), _lib.ptr(ws), n, _lib.stream_handle()), "pmc_sum_f32")
    _lib.check(f.lib.pmc_neg_weighted_sum(_lib.ptr(lp), _lib.ptr(wd), _lib.ptr(ws), 1000.0, _lib.ptr(out), n, _lib.stream_handle()),
               "pmc_neg_weighted_sum")
    ref, mag = tw.valid_reference(lp.cpu().numpy(), w, [np.arange(n)])
    r = abs(float(out.item()) - ref) / (tw.valid_bound(n, 1) * mag)
    RATIO["neg_weighted_sum"] = max(RATIO.get("neg_weighted_sum", 0.0), r)
    assert np.isfinite(ref) and r <= 1.0, f"{name} {regime}: pmc_neg_weighted_sum {out.item()!r} against {ref!r} (sum |terms| {mag!r})"
