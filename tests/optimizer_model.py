"""The clipped AdamW step of ``csrc/maf_train.hip`` (``adamw_kernel`` behind ``launch_adamw``) restated in numpy: a float64
model (``step64``), its float32 twin in the kernel's operation order (``step32``), and the per-element deviation a
float32 evaluation of those statements may have from the float64 one (``bound``).  No GPU.

``tests/test_optimizer_model_cpu.py`` pins ``step64`` to ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW`` on
float64 tensors and holds both forms of the twin to HALF of ``bound`` on every input of the table below;
``tests/test_gpu_optimizer_epoch.py`` holds the kernels to ``bound``."""
from __future__ import annotations

import itertools
from collections import namedtuple

import numpy as np

F = np.float32
U = 2.0 ** -24                     # unit roundoff of float32: one rounding moves a value by at most U of its magnitude
FLOOR = 4.0 * 2.0 ** -149          # results in the subnormal range round absolutely, not relatively
CLIP_EPS = float(F(1e-6))          # the kernel's 1e-6f
BLOCK = 256                        # threads of a block in every kernel here
SQ_BLOCKS = 256                    # PMC_ADAMW_SCRATCH: blocks of sqnorm_partial_kernel (pmc_adamw_step, the bf16 engines)

Scalars = namedtuple("Scalars", "lr b1 b2 eps wd max_norm bc1 bc2")


def scalars(step, lr, wd, max_norm, beta1=0.9, beta2=0.999, eps=1e-8, rounded=True):
    """What ``launch_adamw`` hands the kernel: every hyper-parameter cast to float32, and the bias corrections
    ``1 - beta^step`` computed in double from the DOUBLE betas and then cast.  ``rounded=False``: everything left in
    double, the corrections taken from the given betas (what torch computes; the pin test passes float32-rounded betas)."""
    bc1, bc2 = 1.0 - beta1 ** float(step), 1.0 - beta2 ** float(step)
    v = (lr, beta1, beta2, eps, wd, max_norm, bc1, bc2)
    return Scalars(*(float(F(x)) if rounded else float(x) for x in v))


def coefficient64(g, sc, partials=None):
    """``min(1, max_norm / (sqrt(S) + 1e-6))``, ``S`` the float64 sum of the partials or of ``g**2``; 1 if max_norm <= 0."""
    if sc.max_norm <= 0.0:
        return 1.0
    S = np.sum(np.asarray(partials, np.float64)) if partials is not None else np.sum(np.asarray(g, np.float64) ** 2)
    return min(1.0, sc.max_norm / (np.sqrt(S) + CLIP_EPS))


def step64(p, g, m, v, scalars, partials=None):
    """arguments ``(p, g, m, v, scalars, partials=None)``: one clipped AdamW step in float64 numpy, ``(p, m, v)`` after it.

    Restates ``adamw_kernel`` plus ``launch_adamw`` (``csrc/maf_train.hip``) with the float32-rounded scalars the launcher
    passes (``scalars(...)``)::

        coef = min(1, max_norm / (sqrt(S) + 1e-6))            S = sum(partials) | sum(g**2);  max_norm <= 0: coef = 1
        gr   = g coef
        p'   = p (1 - lr wd)
        m'   = b1 m + (1 - b1) gr
        v'   = b2 v + (1 - b2) gr gr
        p''  = p' - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)

    ``partials``: the float32 sums of squares the device wrote (``sq_partial[:n_jobs]``), added in float64."""
    sc = scalars
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gr = g * coefficient64(g, sc, partials)
    pv = p * (1.0 - sc.lr * sc.wd)
    m1 = sc.b1 * m + (1.0 - sc.b1) * gr
    v1 = sc.b2 * v + (1.0 - sc.b2) * gr * gr
    pv = pv - (sc.lr / sc.bc1) * m1 / (np.sqrt(v1) * (1.0 / np.sqrt(sc.bc2)) + sc.eps)
    return pv, m1, v1


# ------------------------------------------------------------------------------------------------ the float32 twin
def _fma(a, b, c):
    """``a b + c`` rounded once (float32 products are exact in float64; the double rounding of the sum is below 2^-53)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _fma2(a, b, c, d):
    """``a b + c d`` taken as one operation: both products exact, one rounding."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64) * np.asarray(d, np.float64)).astype(F)


def _block_sum(s):
    """A 256-thread block's reduction of per-thread float32 sums ``s [..., 256]``: xor butterflies inside each wave of
    64, then ``(r0 + r1) + (r2 + r3)``."""
    s = np.asarray(s, F).reshape(s.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    r = s[..., 0]
    return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


def sum_partials32(part):
    """``adamw_kernel``'s sum of ``n_part`` partials: thread ``t`` adds entries ``t, t + 256, ...`` in order."""
    part = np.asarray(part, F)
    rows = -(-part.size // BLOCK)
    a = np.zeros(rows * BLOCK, F)
    a[:part.size] = part
    s = np.zeros(BLOCK, F)
    for r in a.reshape(rows, BLOCK):
        s = s + r
    return _block_sum(s)


def sq_partials32(g, fused=False):
    """``sqnorm_partial_kernel``: 256 blocks, thread ``(b, t)`` adds ``g[e]^2`` for ``e = 256 b + t + 65536 k``."""
    g = np.asarray(g, F)
    stride = SQ_BLOCKS * BLOCK
    rows = -(-g.size // stride)
    a = np.zeros(rows * stride, F)
    a[:g.size] = g
    s = np.zeros(stride, F)
    for r in a.reshape(rows, stride):
        s = _fma(r, r, s) if fused else s + r * r
    return _block_sum(s.reshape(SQ_BLOCKS, BLOCK))


def step32(p, g, m, v, scalars, partials=None, fused=False):
    """The float32 twin of ``step64``: the kernel's statements in numpy float32, in its order of operations.
    ``fused=False``: every product and sum rounded on its own.  ``fused=True``: what a compiler that contracts may emit --
    ``b m + (1 - b) g`` (and its ``v`` counterpart) as one operation rounded once, ``1 - lr wd`` and
    ``sqrt(v) rs2 + eps`` as fused multiply-adds.  hipcc may contract either way; the kernels are held to ``bound``, which
    both forms meet with a factor of two to spare."""
    sc = scalars
    lr, b1, b2, eps, wd, max_norm, bc1, bc2 = (F(x) for x in sc)
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    one = F(1.0)
    coef = one
    if max_norm > 0:
        part = np.asarray(partials, F) if partials is not None else sq_partials32(g, fused)
        coef = max_norm / (np.sqrt(sum_partials32(part)) + F(1e-6))
        coef = one if coef > one else F(coef)
    step, rs2 = lr / bc1, one / np.sqrt(bc2)
    gr = g * coef
    if fused:
        pv = p * _fma(-lr, wd, one)
        m1 = _fma2(b1, m, one - b1, gr)
        v1 = _fma2(b2, v, (one - b2) * gr, gr)
        den = _fma(np.sqrt(v1), rs2, eps)
    else:
        pv = p * (one - lr * wd)
        m1 = b1 * m + (one - b1) * gr
        v1 = b2 * v + (one - b2) * gr * gr
        den = np.sqrt(v1) * rs2 + eps
    pv = pv - step * m1 / den
    assert pv.dtype == m1.dtype == v1.dtype == F
    return pv, m1, v1


# ------------------------------------------------------------------------------------------------ the bound
def sq_depth(n):
    """Roundings in ONE partial of ``sqnorm_partial_kernel`` over ``n`` entries: per thread ``ceil(n / 65536)`` squares
    added (a product and a sum each, one rounding if fused: counted as two), six butterfly levels, two block sums."""
    return 2 * -(-int(n) // (SQ_BLOCKS * BLOCK)) + 8


def bound(p, g, m, v, scalars, partials=None, n_part=None, sq_roundings=0):
    """Per element, how far a float32 evaluation of the step may lie from ``step64``: ``(bp, bm, bv)``.

    First-order worst case over the kernel's operations, ``u = 2^-24`` per rounding (sqrtf and the division are correctly
    rounded; ``1 - b1`` and ``1 - b2`` are exact), times TWO -- the factor covers the second-order terms and is what the
    CPU test checks: the twin stays within half of this.  ``S`` sums positive terms, so every rounding in it is relative.

    * ``coef``: the float32 sum of ``n_part`` partials is ``n_part / 256`` additions per thread, six butterfly levels and
      two block sums; sqrt, ``+ 1e-6``, the division: ``dc = (n_part / 256 + 12) u`` (the sqrt halves the sum's share;
      not used).  Where the partials themselves are not the device's (``partials=None``: the model squares the gradient in
      float64) their own ``sq_roundings`` (``sq_depth(n)``) add to it.  ``max_norm <= 0``: ``dc = 0``.
    * ``gr = g coef``: ``dc + u``.
    * ``m' = b1 m + (1 - b1) gr``: two products, one sum; the sum may cancel, so the error is relative to
      ``A = |b1 m| + |(1 - b1) g coef|``, not to ``|m'|``:   ``|dm| <= (dc + 4u) A``.
    * ``v' = b2 v + (1 - b2) gr gr``: positive terms, ``gr`` twice:   ``|dv| <= (2 dc + 6u) v'``.
    * ``den = sqrt(v') rs2 + eps``: half of ``dv`` and the sqrt (``dc + 4u``), ``rs2 = 1 / sqrt(bc2)`` (2u), the product,
      the sum:   ``(dc + 8u) den``.
    * the update ``Upd = (lr / bc1) m' / den``: the step size, the product, the division (3u), ``den``, and ``dm``:
      ``|dUpd| <= (lr / bc1) / den * ((dc + 4u) A + (dc + 11u) |m'|) <= (lr / bc1) / den * A (2 dc + 15u)``.
    * ``p'' = p (1 - lr wd) - Upd``: ``lr wd``, ``1 -``, the product (3u |p|), the difference (u (|p| + |Upd|)):
      ``|dp| <= 4u |p| + (lr / bc1) / den * A (2 dc + 16u)``.

    Every term also gets ``FLOOR`` (a few float32 subnormal steps)."""
    sc = scalars
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    dc = 0.0
    if sc.max_norm > 0.0:
        if n_part is None:
            n_part = SQ_BLOCKS if partials is None else np.asarray(partials).size
        dc = (n_part / 256.0 + 12.0 + sq_roundings) * U
    coef = coefficient64(g, sc, partials)
    A = np.abs(sc.b1 * m) + np.abs((1.0 - sc.b1) * g * coef)
    _, _, v1 = step64(p, g, m, v, sc, partials)
    den = np.sqrt(v1) / np.sqrt(sc.bc2) + sc.eps
    bm = (dc + 4 * U) * A
    bv = (2 * dc + 6 * U) * v1
    bp = 4 * U * np.abs(p) + (sc.lr / sc.bc1) / den * A * (2 * dc + 16 * U)
    return tuple(2.0 * b + FLOOR for b in (bp, bm, bv))


def worst_ratio(got, want, bnd):
    """Largest ``|got - want| / bound`` over ``p, m, v`` (``nan`` anywhere: ``inf``)."""
    worst = 0.0
    for a, b, c in zip(got, want, bnd):
        r = np.abs(np.asarray(a, np.float64) - b) / c
        worst = max(worst, float(np.inf if not np.isfinite(r).all() else r.max()))
    return worst


# ------------------------------------------------------------------------------------------------ the inputs
STATES = ("fresh", "opposed", "mixed")
HYPER = tuple(itertools.product((1, 2, 10, 10000), (1e-3, 2e-4, 1e-6), (0.0, 0.01), (0.0, 1.0, 1e9)))   # step, lr, wd, max_norm


def state(kind, n, seed=0):
    """``(p, g, m, v)`` float32 ``[n]`` shaped like a fit's: three entries in ten masked (``g = m = v = 0``), ``|g|``
    log-uniform over 1e-8 .. 1e3 with either sign (its norm stays far below 1e9);  ``fresh``: ``m = v = 0``;
    ``opposed``: ``m`` opposite in sign to ``g``, on half of the entries within 1e-3 of cancelling ``(1 - b1) g`` against
    ``b1 m``;  ``mixed``: moments of an earlier gradient of either sign, a tenth of them fresh."""
    rng = np.random.default_rng([seed, n, STATES.index(kind)])
    p = (0.3 * rng.normal(size=n)).astype(F)
    g = (10.0 ** rng.uniform(-8.0, 3.0, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(F)
    masked = rng.random(n) < 0.3
    g[masked] = 0
    g64 = g.astype(np.float64)
    if kind == "fresh":
        m, v = np.zeros(n), np.zeros(n)
    elif kind == "opposed":
        near = rng.random(n) < 0.5
        b1 = float(F(0.9))
        m = -g64 * np.where(near, (1.0 - b1) / b1 * (1.0 + 1e-3 * rng.normal(size=n)), rng.uniform(0.5, 2.0, size=n))
        v = g64 ** 2 * rng.uniform(0.5, 2.0, size=n)
    else:
        old = g64 * 10.0 ** rng.uniform(-2.0, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
        m, v = 0.1 * old, 0.001 * old ** 2
        new = rng.random(n) < 0.1
        m[new], v[new] = 0, 0
    m, v = m.astype(F), v.astype(F)
    m[masked], v[masked] = 0, 0
    return p, g, m, v
