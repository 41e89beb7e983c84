"""The weights a run hands ``Flow.fit``: importance weights normalised to sum 1 and cast to float32 (``Sampler._fit``), in
the regimes of ``tests/pool_regimes.py`` -- many orders of magnitude apart, denormal, exactly 0, all but one 0.  Shared by
``tests/test_train_weights_cpu.py`` (which regimes a float32 trainer can be held to) and ``tests/test_gpu_train_weights.py``."""
from __future__ import annotations

import numpy as np
import torch

import flow_regimes as fr
import pool_regimes as pr
from oracle.maf import torch_loss
from test_gpu_flow_regimes import _blocks as blocks          # the parameter blocks of the trainer's criterion

REGIMES = ("equal", "wide", "very_wide", "holes", "one_hot")
N = 100
CE_MAX = 1e-3               # a (fixture, regime) is kept where C e stays at or below this in every parameter block
# (fixture, regime) pairs no seed of which meets the condition (tests/test_train_weights_cpu.py keeps this table true).
# Seeds passed over on the CPU's fixtures, spline flows only (C e 1.1e-3 .. 2.4e-3 on rows next to a knot): nsf6 trained
# equal 0, holes 0, one_hot 0; nsf6 gain 4 equal 0-4, one_hot 0-1.
DROPPED = ()


def run_weights(regime, n=N, seed=0):
    """float32 ``w / sum(w)`` of the regime; zeros and denormals stay as they come."""
    w = pr.weights(regime, n, seed)
    return (w / w.sum()).astype(np.float32)


def rows(data, n=N, seed=0):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(data[rng.choice(len(data), n, replace=False)], np.float32)


def condition(spec, flat, x, w):
    """``(finite, C e)``: the float64 autograd reference of ``torch_loss`` is finite, and the float32 twin's error ``e``
    (per block, ``max |g32 - g64| / max |g64|``; the criterion of ``test_trainer_loss_and_gradient_per_block``) times
    ``C``, the largest over the blocks."""
    ref = {}
    for dt in (torch.float64, torch.float32):
        ft = torch.tensor(flat.astype(np.float64) if dt == torch.float64 else flat, dtype=dt, requires_grad=True)
        lo = torch_loss(spec, ft, torch.from_numpy(x).to(dt), torch.from_numpy(w).to(dt))
        lo.backward()
        ref[dt] = (float(lo.detach()), ft.grad.double().numpy())
    (l64, g64), (l32, g32) = ref[torch.float64], ref[torch.float32]
    finite = bool(np.isfinite(l64) and np.isfinite(g64).all())
    worst = 0.0
    if finite:
        for _, sl in blocks(spec):
            s = max(np.abs(g64[sl]).max(), fr.TINY)
            worst = max(worst, fr.C * float(np.abs(g32[sl] - g64[sl]).max() / s))
    return finite, worst


def pick(spec, flat, data, regime, seeds=range(6)):
    """``(seed, x, w)`` of the first seed whose rows and weights meet the condition (a finite float64 reference and
    ``C e <= CE_MAX`` in every block), or None: the seeds before it are dropped, never a kernel's result consulted."""
    for seed in seeds:
        x, w = rows(data, seed=seed), run_weights(regime, seed=seed)
        finite, ce = condition(spec, flat, x, w)
        if finite and ce <= CE_MAX:
            return seed, x, w
    return None


def zero_rows_last(x, w):
    """The batch with its rows of weight 0 moved behind the others (stable): the rows that count keep their order, and
    without the tail they keep their positions within their 16-row sets.  ``(x, w, rows that count)``."""
    order = np.argsort(w == 0, kind="stable")
    return np.ascontiguousarray(x[order]), np.ascontiguousarray(w[order]), int((w != 0).sum())


def valid_reference(lp, w, batches):
    """``sum over batches of -sum(lp w 1000 / sum w)`` in float64 from the device's log-densities, and ``sum |terms|``.
    ``batches``: index arrays into ``lp`` / ``w``.  A batch whose float32 weights are all 0 is 0 / 0 there, as in the
    reference's DataLoader loop: nan."""
    total, mag = 0.0, 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for idx in batches:
            wb = w[idx].astype(np.float64)
            terms = lp[idx].astype(np.float64) * (wb * (1000.0 / wb.sum()))
            total -= terms.sum()
            mag += np.abs(terms).sum()
    return total, mag


def valid_bound(nb, n_batches):
    """Roundings of ``epoch_nll_kernel`` relative to ``sum |terms|``: per batch the float32 weight sum (``nb / 256 + 8``:
    strided adds, six butterfly levels, two block sums), ONE division, two products per term, the terms' sum
    (``nb / 256 + 8`` again), and one addition per batch into the running total."""
    d = -(-nb // 256) + 8
    return (2 * d + 3 + n_batches) * 2.0 ** -24
