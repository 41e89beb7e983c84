"""Torch-autograd restatement of the bf16 spline trainer (``csrc/maf_train_bf16.hip``, ``train_engine="bf16_spline"``):
``oracle.maf.torch_log_prob`` / ``torch_loss`` for spline specs, rounding to bf16 exactly where the engine rounds
(``tests/test_bf16_spline_train_model_cpu.py``, ``tests/test_gpu_train_bf16_spline.py``).

Where the engine rounds -- its contract:

* masked weights ``rne(W * mask)``; the biases stay float32;
* ``x_t`` is rounded into layer 0 only; the spline reads the unrounded ``x_t``;
* ``h0``, ``h1``, ``h2`` are rounded when stored, and the residual reads the rounded value;
* phi, the spline, ladj, the loss, the spline's own ``dL/dx`` and ``dL/dx_t`` are never rounded;
* ``dphi``, ``da2``, ``da1``, ``da0`` are rounded when stored.

Three ``autograd.Function``s say that: ``RF`` (value rounded, gradient passed through: ``W * mask``, ``x_t`` into layer
0), ``RFB`` (value and gradient rounded: ``h0``, ``h1``, ``h2`` behind the relu), ``RB`` (value untouched, gradient rounded:
phi in front of the spline).

The model is evaluated in float64 (the reference: ``g_T64``, ``loss_T64``) and in float32 (the yardstick ``g_T32``);
``g_64`` is plain float64 autograd of ``torch_loss`` and ``d_round = |g_T64 - g_64|`` what bf16 costs on the same rows.

Criterion (``verdict``): overall ``|g - g_T64| <= 0.25 d_round``, every parameter tensor against its own ``d_round`` <= 0.5,
``|loss - loss_T64| <= 5e-5 |loss_T64|`` (the float32 spline trainer's own tolerance), masked entries exactly 0.  The
yardstick must hold 0.10 / 0.25 on the same rows.  The two ratios are conditions: the kernel has to be several times
nearer to the model that rounds where it rounds than bf16 is to the unrounded gradient.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import cases
from oracle.maf import rqs_forward, torch_loss
from pocomc_amd.maf_spec import MAFSpec

OVERALL, PER_TENSOR, LOSS_RTOL = 0.25, 0.5, 5e-5
YARD_OVERALL, YARD_PER_TENSOR = 0.10, 0.25

# single defects of the model that the criterion has to reject
DEFECTS = ("spline_x_rounded",        # the spline evaluated at rne(x)
           "drop_output_kstep",       # the output product stops one k-step of 32 (slot order) early
           "swap_widths_heights",     # phi[0:K] and phi[K:2K] of a feature exchanged
           "gx_missing",              # dL/dx_t without the spline's own dL/dx
           "ladj_missing")            # the log-determinant's term missing from the gradient

# (D, T, H, bins, n, weighted, s): the flows are cases.flow_params(spec, 2, gain=1.0), the rows default_rng(D + n).normal * s
CASES = ((16, 2, 64, 8, 100, True, 2.5), (16, 2, 64, 8, 1, False, 2.5), (5, 3, 32, 8, 33, False, 2.5),
         (16, 2, 64, 4, 31, True, 2.5), (16, 2, 64, 16, 40, False, 2.5), (40, 3, 256, 8, 300, False, 2.5),
         (64, 6, 256, 8, 200, True, 2.5), (128, 3, 512, 8, 512, False, 2.5), (128, 3, 512, 8, 700, True, 1.2))


def _rne(v):
    return v.to(torch.float32).to(torch.bfloat16).to(v.dtype)


class RF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        return _rne(v)

    @staticmethod
    def backward(ctx, g):
        return g


class RFB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        return _rne(v)

    @staticmethod
    def backward(ctx, g):
        return _rne(g)


class RB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        return v.clone()

    @staticmethod
    def backward(ctx, g):
        return _rne(g)


def model_loss(spec, flat_t, x_t, w_t=None, rounding=True, defect=None):
    """``torch_loss`` of a spline ``spec`` as the engine evaluates it, in the dtype of ``flat_t`` / ``x_t``."""
    assert spec.univariate == "rqs" and (defect is None or defect in DEFECTS)
    ident = lambda v: v
    rf, rfb, rb = (RF.apply, RFB.apply, RB.apply) if rounding else (ident, ident, ident)
    D, K, dt = spec.n_dim, spec.bins, x_t.dtype
    x = x_t
    ladj = torch.zeros(x.shape[0], dtype=dt)
    for t in range(spec.n_transforms):
        M = [torch.from_numpy(m.astype(np.float64)).to(dt) for m in spec.masks(t)]

        def v(name):
            off, sz = spec.offsets[name]
            b = t * spec.params_per_transform + off
            return flat_t[b:b + sz].reshape(spec.shapes()[name])
        W3 = rf(v("W3") * M[3])
        if defect == "drop_output_kstep":
            su = np.asarray(spec.slot_unit)
            HK = (spec.Hp + 31) // 32 * 32
            late = su[HK - 32:spec.Hp]
            keep = torch.ones(spec.hidden, dtype=dt)
            keep[torch.from_numpy(late[late >= 0])] = 0.0
            W3 = W3 * keep[None, :]
        h = rfb(torch.relu(rf(x) @ rf(v("W0") * M[0]).T + v("b0")))
        h = rfb(torch.relu(h + h @ rf(v("W1") * M[1]).T + v("b1")))
        h = rfb(torch.relu(h + h @ rf(v("W2") * M[2]).T + v("b2")))
        phi = rb((h @ W3.T + v("b3")).reshape(x.shape[0], D, spec.n_out))
        if defect == "swap_widths_heights":
            phi = torch.cat([phi[..., K:2 * K], phi[..., :K], phi[..., 2 * K:]], -1)
        xs = x
        if defect == "spline_x_rounded":
            xs = RF.apply(x)
        if defect == "gx_missing":
            xs = x.detach()
        x, ls = rqs_forward(xs, phi, K, xp=torch)
        if defect == "ladj_missing":
            ls = ls.detach()
        ladj = ladj + ls.sum(dim=1)
    lp = -0.5 * (x ** 2).sum(dim=1) - 0.5 * D * math.log(2 * math.pi) + ladj
    if w_t is None:
        return -lp.sum()
    return (-(lp * w_t * 1000.0)).sum() / w_t.sum()


def loss_and_gradient(spec, flat, x, w=None, dtype=torch.float64, rounding=True, defect=None, plain=False):
    """``(loss, gradient)`` as float64 numpy; ``plain``: ``oracle.maf.torch_loss`` itself."""
    ft = torch.tensor(np.asarray(flat, np.float32), dtype=dtype, requires_grad=True)
    xt = torch.tensor(np.asarray(x, np.float32), dtype=dtype)
    wt = None if w is None else torch.tensor(np.asarray(w, np.float32), dtype=dtype)
    lo = torch_loss(spec, ft, xt, wt) if plain else model_loss(spec, ft, xt, wt, rounding, defect)
    lo.backward()
    return float(lo.detach()), ft.grad.numpy().astype(np.float64)


def case_inputs(case):
    """``(spec, flat, x, w)`` of one of ``CASES``."""
    D, T, H, K, n, weighted, s = case
    spec = MAFSpec(D, T, hidden=H, univariate="rqs", bins=K)
    flat = cases.flow_params(spec, 2, gain=1.0)
    rng = np.random.default_rng(D + n)
    x = (rng.normal(size=(n, D)) * s).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    return spec, flat, x, w


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Computed once per process and shared: ``dict(spec, flat, x, w, g64, loss64, gT64, lossT64, gT32, lossT32)``."""
    spec, flat, x, w = case_inputs(case)
    l64, g64 = loss_and_gradient(spec, flat, x, w, plain=True)
    lT64, gT64 = loss_and_gradient(spec, flat, x, w)
    lT32, gT32 = loss_and_gradient(spec, flat, x, w, dtype=torch.float32)
    return dict(spec=spec, flat=flat, x=x, w=w, g64=g64, loss64=l64, gT64=gT64, lossT64=lT64, gT32=gT32, lossT32=lT32)


def ratios(spec, g, gT64, g64):
    """``(overall, worst tensor, its name)``: ``|g - g_T64| / d_round`` over the whole gradient and over every parameter
    tensor ``(t, name)`` against that tensor's own ``d_round`` (a tensor bf16 costs nothing must be matched exactly)."""
    def ratio(a, ref, plain):
        err, dr = np.linalg.norm(a - ref), np.linalg.norm(ref - plain)
        return 0.0 if err == 0.0 else (err / dr if dr > 0.0 else np.inf)
    worst, where = 0.0, None
    for t in range(spec.n_transforms):
        for name in spec.offsets:
            r = ratio(spec.view(g, t, name), spec.view(gT64, t, name), spec.view(g64, t, name))
            if r > worst:
                worst, where = r, (t, name)
    return ratio(g, gT64, g64), worst, where


def verdict(spec, loss, g, ref, overall=OVERALL, per_tensor=PER_TENSOR):
    """The criterion on ``(loss, g)`` against ``case_reference``'s dictionary: ``dict(ok, overall, worst, where, loss_rel,
    masked_zero)``."""
    ov, worst, where = ratios(spec, g, ref["gT64"], ref["g64"])
    loss_rel = abs(loss - ref["lossT64"]) / abs(ref["lossT64"])
    masked_zero = bool(np.all(g[spec.mask_flat() == 0] == 0.0))
    ok = ov <= overall and worst <= per_tensor and loss_rel <= LOSS_RTOL and masked_zero
    return dict(ok=bool(ok), overall=ov, worst=worst, where=where, loss_rel=loss_rel, masked_zero=masked_zero)
