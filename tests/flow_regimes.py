"""Flows in the regimes the Sampler runs them in, inputs at the spline's edges, and the criterion the flow kernels are held
to there (``tests/test_flow_regimes_cpu.py``, ``tests/test_gpu_flow_regimes.py``).

Why: every other parity test builds its flow from the default initialisation (``cases.flow_params``), but the Sampler
trains its flow before every MCMC call, and a trained flow -- or one whose hyper-network output layer sits at the soft
clip's ceiling -- conditions the maps much worse: even the float32 oracle misses the suite's fixed bounds there.  So the
yardstick here is not a fixed bound alone but the SENSITIVITY of each row:

* reference: the float64 oracle on the same float32 parameters and inputs (``OracleMAF(dtype=float64)``);
* envelope ``e_i``: the largest deviation from that reference among ``N_PERTURB`` float64 evaluations whose inputs and
  parameters carry independent random +-2^-24 relative perturbations (half an ulp of float32: what rounding the inputs
  of any float32 evaluation does to it) -- and, in spline flows, so do the computed knots and interior derivatives, which
  every float32 evaluation rounds near +-5 whatever the bin's width (``tests/test_flow_regimes_cpu.py`` shows that inputs
  and parameters alone do not bound the float32 oracle's own error on a trained spline flow);
* criterion: ``err_i <= max(bound, C * e_i)`` on every row (``bound``: the suite's existing bound of that quantity), the
  median over rows of ``err_i / max(e_i, 2^-24)`` at most ``MEDIAN_BOUND`` (or 1.25 x the median of a float32 evaluation
  of the same rows where that exceeds it -- measured in the same test, never a constant), and a finite result wherever the reference
  and every perturbed evaluation are finite and below float32's maximum.

Errors are measured per row like ``parity.close_rel``: a vector (z, x) by ``max_j |a_ij - b_ij| / max_j |b_ij|``, a
log-determinant or log-density against the size of its terms (``cancel``).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import parity
from oracle.maf import OracleMAF, _rqs_knots, torch_loss
from pocomc_amd.maf_spec import MAFSpec

C = 16.0                     # one constant for every kernel family
MEDIAN_BOUND = 2.0
EPS = 2.0 ** -24
N_PERTURB = 8
F32_MAX = float(np.finfo(np.float32).max)
TINY = np.finfo(np.float64).tiny

# the suite's existing bounds (tests/parity.py TOL for the affine flows, tests/test_gpu_flow.py NSF_* for the splines)
AFFINE_BOUND = {"z": 1e-5, "x": 1e-5, "ladj": 1e-5, "log_prob": 1e-5}
NSF_BOUND = {"z": 2e-5, "x": 5e-5, "ladj": 1e-4, "log_prob": 1e-4}
TRAIN_BOUND = 2e-5           # tests/test_gpu_train.py: the gradient's absolute slack, relative to its scale

NONFINITE_ROWS = (0, 15, 16, 17, -1)     # the edges of the 16-row tiles, and the last row


def bounds(spec):
    return NSF_BOUND if spec.univariate == "rqs" else AFFINE_BOUND


# ------------------------------------------------------------------------------------------------------------ flows
def gain_params(spec, g, seed=0):
    """The default initialisation with the output layer (W3, b3) of every transform scaled by ``g``: hidden layers at init,
    the hyper-network's outputs pushed towards the soft clip's ceiling."""
    flat = spec.init_params(seed).astype(np.float32)
    for t in range(spec.n_transforms):
        for name in ("W3", "b3"):
            off, sz = spec.offsets[name]
            b = t * spec.params_per_transform + off
            flat[b:b + sz] *= np.float32(g)
    return flat


def two_modes(D, n, seed=0, sep=2.0, width=0.1):
    """Two narrow modes at ``+-sep`` (each row picks one), standard deviation ``width`` per coordinate."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.random(n) < 0.5, -sep, sep)[:, None]
    return (s + width * rng.normal(size=(n, D))).astype(np.float32)


def rosenbrock_draws(D, n, seed=0):
    """Exact draws of the Rosenbrock density ``exp(-sum 10 (x_2i^2 - x_2i+1)^2 + (x_2i - 1)^2)`` (tests/golden/cases.py)."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, D))
    x[:, ::2] = 1.0 + rng.normal(size=(n, (D + 1) // 2)) / math.sqrt(2.0)
    x[:, 1::2] = x[:, 0:2 * (D // 2):2] ** 2 + rng.normal(size=(n, D // 2)) / math.sqrt(20.0)
    return x.astype(np.float32)


def bimodal_draws(D, n, seed=0, sep=3.0):
    """Config 3's mixture: unit Gaussians at ``+-sep`` in every coordinate, equal weights."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.random(n) < 0.5, -sep, sep)[:, None]
    return (s + rng.normal(size=(n, D))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def twin_trained(name, steps=400, seed=0):
    """(spec, float32 parameters) of the oracle's torch twin (``torch_loss``) trained by ``steps`` AdamW steps on two narrow
    modes at D = 10: the CPU stand-in for a flow ``Flow.fit`` trained."""
    import torch
    spec = {"maf3": MAFSpec(10, 3), "nsf6": MAFSpec(10, 6, univariate="rqs")}[name]
    x = torch.from_numpy(two_modes(10, 512, seed))
    ft = torch.tensor(spec.init_params(seed), requires_grad=True)
    opt = torch.optim.AdamW([ft], lr=3e-3)
    for _ in range(steps):
        opt.zero_grad()
        (torch_loss(spec, ft, x) / len(x)).backward()
        torch.nn.utils.clip_grad_norm_([ft], 1.0)
        opt.step()
    return spec, ft.detach().numpy().astype(np.float32)


def regime_stats(spec, flat, x):
    """What the hyper-network outputs on rows ``x``: for spline flows the share of bins (widths and heights) below 2e-3 of
    the box and the range of the interior derivatives; for affine flows the share of |log-scale| > 5."""
    o = OracleMAF(spec, flat)
    x = np.asarray(x, np.float32)
    out = {}
    cur = x
    if spec.univariate == "rqs":
        small, dmin, dmax = [], np.inf, 0.0
        K = spec.bins
        for t in range(spec.n_transforms):
            phi = o._phi(t, cur)
            xk, yk, dk = _rqs_knots(phi, K, np)
            small.append(((np.diff(xk, axis=-1) < 2e-3 * 10) | (np.diff(yk, axis=-1) < 2e-3 * 10)).mean())
            dmin, dmax = min(dmin, float(dk[..., 1:-1].min())), max(dmax, float(dk[..., 1:-1].max()))
            cur, _ = o._fwd(t, cur)
        out.update(small_bin_share=float(np.mean(small)), deriv_min=dmin, deriv_max=dmax)
    else:
        big = []
        for t in range(spec.n_transforms):
            _, ls = o._hyper(t, cur)
            big.append((np.abs(ls) > 5.0).mean())
            cur, _ = o._fwd(t, cur)
        out.update(big_log_scale_share=float(np.mean(big)))
    return out


# ------------------------------------------------------------------------------------------------------ edge inputs
def _ulps(v, k):
    """``v`` moved by ``k`` ulps of float32 (k of either sign)."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return v


def first_feature(spec, t):
    """The feature of rank 0 in transform ``t`` (zuko MAF: identity order in even transforms, reversed in odd ones): its
    conditioner reads nothing, its spline is constant over the rows."""
    return 0 if t % 2 == 0 else spec.n_dim - 1


def constant_knots(spec, flat, t):
    """The float32 oracle's x knots and y knots of the first-ranked feature of transform ``t``."""
    o = OracleMAF(spec, flat)
    phi = o._phi(t, np.zeros((1, spec.n_dim), np.float32))[0, first_feature(spec, t)]
    xk, yk, _ = _rqs_knots(phi[None], spec.bins, np)
    return xk[0], yk[0]


def knot_rows(spec, flat, base, inverse=False, knots=None):
    """Rows of ``base`` (cycled) whose first-ranked coordinate -- of transform 0 for the forward map, of the last transform
    for the inverse -- sits exactly on each float32 knot of the oracle (``knots``: on these knots only) and one ulp either
    side.  Returns ``(rows, where)`` with ``where[i] = (knot index, ulps)``."""
    t = spec.n_transforms - 1 if inverse else 0
    xk, yk = constant_knots(spec, flat, t)
    kn = yk if inverse else xk
    f = first_feature(spec, t)
    rows, where = [], []
    for j in (range(len(kn)) if knots is None else knots):
        for d in (-1, 0, 1):
            r = np.array(base[len(rows) % len(base)], np.float32)
            r[f] = _ulps(kn[j], d)
            rows.append(r)
            where.append((j, d))
    return np.stack(rows), where


def all_knot_rows(spec, flat, base):
    """Rows of ``base`` set rank by rank so that EVERY coordinate sits on one of the float32 oracle's knots of transform 0
    (feature r's spline depends on features of rank < r only, which are set first).  Row i puts feature r on knot
    ``(i + r) % (K + 1)`` -- end knots included."""
    o = OracleMAF(spec, flat)
    x = np.array(base, np.float32)
    K = spec.bins
    pick = (np.arange(len(x))[:, None] + np.arange(spec.n_dim)[None, :]) % (K + 1)
    for r in range(spec.n_dim):                          # transform 0: rank r = feature r
        phi = o._phi(0, x)[:, r]
        xk, _, _ = _rqs_knots(phi, K, np)
        x[:, r] = xk[np.arange(len(x)), pick[:, r]]
    return x, pick


def box_rows(spec, flat, base, inverse=False):
    """Rows whose first-ranked coordinate (transform 0 / the last transform) is at +-5.0f, one and two ulps either side,
    and in the ulp band between the oracle's computed end knot of that spline and 5.0f (both ends included).  Returns
    ``(rows, band)``: ``band[i]`` is True for the rows in the band."""
    t = spec.n_transforms - 1 if inverse else 0
    xk, yk = constant_knots(spec, flat, t)
    end = (yk if inverse else xk)[-1]
    f = first_feature(spec, t)
    vals = [_ulps(s * 5.0, d) for s in (-1.0, 1.0) for d in (-2, -1, 0, 1, 2)]
    band = []
    lo, hi = min(end, np.float32(5.0)), max(end, np.float32(5.0))
    v = lo
    while v <= hi and len(band) < 16:
        band.append(v)
        v = _ulps(v, 1)
    rows = []
    for i, v in enumerate(vals + band):
        r = np.array(base[i % len(base)], np.float32)
        r[f] = v
        rows.append(r)
    return np.stack(rows), np.array([False] * len(vals) + [True] * len(band))


def outside_rows(spec, base, n_all=4):
    """Rows with coordinates well beyond every spline's box (|x| >= 5.0001: the computed end knots are within a few ulps of
    5), for the bit-for-bit identity tests; the first ``n_all`` rows have EVERY coordinate outside.  Returns ``(rows,
    outside mask)``."""
    rng = np.random.default_rng(17)
    x = np.array(base, np.float32)
    mag = np.float32([5.0001, 5.5, 7.0, 1e3, 1e6, 1e20])
    out = rng.random(x.shape) < 0.3
    out[:n_all] = True
    v = rng.choice(mag, size=x.shape) * np.where(rng.random(x.shape) < 0.5, -1.0, 1.0).astype(np.float32)
    x[out] = v[out]
    return x, out


RELU_MARGIN = 2.0 ** -18     # 64 half-ulps of float32, relative to the sum of the magnitudes of a pre-activation's terms


def relu_margin(spec, flat, x):
    """Per row of ``x``: the smallest ``|pre-activation| / sum |its terms|`` over the hidden units of the three ReLU layers
    of every transform (float64 oracle; a unit whose terms are all zero is exactly zero in every evaluation and does not
    count).  Below ``RELU_MARGIN`` the sign of that pre-activation is within a float32 evaluation's rounding -- measured:
    -1.5e-7 in float64, +4.1e-7 in the float32 numpy oracle, against units of ~0.3, on one row of 5 of ``nsf3-d102-g2`` --
    and the loss is not differentiable in the parameters there: the two one-sided gradients differ by that unit's whole
    contribution (2.4e-3 of the bias block), and which one a float32 evaluation returns depends on its order of additions."""
    o = oracle64(spec, flat)
    cur = np.asarray(x, np.float64)
    worst = np.full(len(cur), np.inf)
    for t in range(spec.n_transforms):
        m, h = o._mats[t], cur
        for i in range(3):
            W, b = m[f"W{i}"], m[f"b{i}"]
            pre = h @ W.T + b + (h if i else 0.0)
            terms = np.abs(h) @ np.abs(W).T + np.abs(b) + (np.abs(h) if i else 0.0)
            ratio = np.where(terms > 0, np.abs(pre) / np.maximum(terms, TINY), np.inf)
            worst = np.minimum(worst, ratio.min(axis=1))
            h = np.maximum(pre, 0.0)
        cur, _ = o._fwd(t, cur)
    return worst


def with_nonfinite(x):
    """``x`` with NaN / +inf / -inf in one coordinate of the rows ``NONFINITE_ROWS``; returns ``(bad, rows)``."""
    bad = np.array(x, np.float32)
    n, D = bad.shape
    rows = sorted({r % n for r in NONFINITE_ROWS})
    for i, r in enumerate(rows):
        bad[r, (5 * i) % D] = (np.nan, np.inf, -np.inf)[i % 3]
    return bad, rows


# ------------------------------------------------------------------------------ the fixed rows of a fixture
ROWS = {10: (384, 192), 32: (256, 96), 50: (256, 96), 86: (32, 16), 102: (32, 16), 128: (64, 8)}   # forward / inverse rows per D (float64 D-pass cost)


def n_perturb(spec):
    """Perturbed evaluations of the envelope: 4 from D = 86 on (the float64 D-pass costs D passes of a 43- to 51-tile
    network)."""
    return min(N_PERTURB, 4) if spec.n_dim >= 86 else N_PERTURB


def forward_inputs(spec, flat, data):
    n = ROWS[spec.n_dim][0]
    x = data[np.random.default_rng(11).choice(len(data), n, replace=False)]
    parts = [x]
    if spec.univariate == "rqs":
        parts += [knot_rows(spec, flat, x)[0], all_knot_rows(spec, flat, x[:16])[0], box_rows(spec, flat, x)[0]]
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


WIDE_INVERSE_KNOTS = (0, 2, 4, 6, 8)      # D >= 86: both end knots and every other interior one (the float64 D-pass of a
                                          # spline flow costs ~0.2-0.3 s per row there; the forward rows keep every knot)


def inverse_inputs(spec, flat, data, latent_of):
    """Half latent images (``latent_of(x)``: a float32 forward map of the flow) of the flow's own rows, half N(0, 1.2^2);
    spline flows: and the knot and box rows of the last transform."""
    n = ROWS[spec.n_dim][1]
    rng = np.random.default_rng(12)
    x = data[rng.choice(len(data), n // 2, replace=False)]
    z = np.concatenate([np.asarray(latent_of(x), np.float32), (rng.normal(size=(n - n // 2, spec.n_dim)) * 1.2).astype(np.float32)])
    parts = [z]
    if spec.univariate == "rqs":
        knots = WIDE_INVERSE_KNOTS if spec.n_dim >= 86 else None
        parts += [knot_rows(spec, flat, z, inverse=True, knots=knots)[0], box_rows(spec, flat, z, inverse=True)[0]]
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


# ------------------------------------------------------------------- the default-width flows at n_dim 102 and 128
# Scaled-up flows at the default hidden width (MAFSpec(D, 3): H = 512; D = 102 pads it to Hp = 816, 51 hidden tiles, the
# widest there is), where AUTO is the lean D-pass kernel and only the workgroup sweeps are triangular.  name: (D, family,
# gain).  The gains: at gain 2 every inverse row, at gain 3 most of them have C e_i <= WELL (tests/test_flow_regimes_cpu.py
# asserts the shares); at gain 4 half the inverse rows have envelopes up to 1 and the criterion would be empty -- but the
# FORWARD map stays well conditioned at gain 4 and 16, so those two flows are held forward only (WIDE_FORWARD_ONLY).
# D = 128 and 86 are widths where AUTO's lone-wave spline sweep and the workgroup spline sweep run on the same rows.  At
# D = 128 (33 hidden tiles of three or four degree groups each) no output product is dealt by K range -- ``k_split_tiles``
# is 0: a factor on the second K range's partial changes nothing there -- so nsf3-d86-g2 (43 tiles of two groups, 27 of them
# split) is the fixture where both sweeps run AND the products are split.
WIDE_GAIN = {"maf3-d102-g2": (102, "affine", 2.0), "maf3-d102-g3": (102, "affine", 3.0),
             "nsf3-d102-g2": (102, "rqs", 2.0), "nsf3-d102-g3": (102, "rqs", 3.0), "nsf3-d128-g2": (128, "rqs", 2.0),
             "maf3-d102-g16": (102, "affine", 16.0), "nsf3-d102-g4": (102, "rqs", 4.0), "nsf3-d86-g2": (86, "rqs", 2.0)}
WIDE_FORWARD_ONLY = ("maf3-d102-g16", "nsf3-d102-g4")
WELL = 1e-2                  # non-vacuity: a row counts as held by the criterion where C e_i <= WELL
WELL_SHARE = 0.75            # ... and at least this share of the inverse rows must be (every forward row)


def wide_gain_fixture(name):
    """(spec, float32 parameters, data rows) of a ``WIDE_GAIN`` flow."""
    D, uni, g = WIDE_GAIN[name]
    spec = MAFSpec(D, 3, univariate=uni)
    return spec, gain_params(spec, g), two_modes(D, 1000, 9) * np.float32(1.3)


def oracle_latent(spec, flat):
    """The float32 numpy oracle's forward map: the latent images of the wide fixtures' inverse rows (the same rows with and
    without a GPU)."""
    o = OracleMAF(spec, flat)
    return lambda x: o.forward(np.asarray(x, np.float32))[0]


def k_split_tiles(spec):
    """Hidden tiles whose output partials the workgroup spline sweep deals by K range (``output_partials``,
    csrc/maf_inverse_wg_nsf.hip: products of >= 16 K tiles of a tile with one or two degree groups), counted from the degree
    words the kernel reads (``quad_meta``).  What a test of the split path must see > 0."""
    deg = (spec.quad_meta & 0xffff).reshape(spec.nT, 4)
    return sum(len({int(d) for d in deg[J] if d < spec.n_dim}) in (1, 2) for J in range(16, spec.nT))


def well_share(R, q):
    """(share, count, of) of the rows the reference counts whose envelope keeps the criterion tight: ``C e_i <= WELL``."""
    well = R.ok & (C * R.env[q] <= WELL)
    return float(well.sum()) / max(int(R.ok.sum()), 1), int(well.sum()), int(R.ok.sum())


def assert_non_vacuous(R, what):
    """The non-vacuity condition of the wide fixtures (a condition on the INPUTS, no tolerance of a kernel): on the inverse
    rows at least ``WELL_SHARE`` of the counted rows, on the forward rows every one, has ``C e_i <= WELL`` in every
    quantity.  Returns the shares."""
    shares = {}
    for q in R.ref:
        s, k, n = well_share(R, q)
        shares[q] = s
        need = 1.0 if R.direction == "forward" else WELL_SHARE
        assert n > 0 and s >= need, f"{what} {R.direction} {q}: {k} of {n} counted rows have C e_i <= {WELL:g} (needs {need:g})"
    return shares


# ------------------------------------------------------------------------------------------- reference and envelope
def oracle64(spec, flat, rng=None, knots=True):
    """The float64 oracle on the float32 parameters ``flat``; with ``rng``: every parameter multiplied by an independent
    ``1 +- 2^-24``, and (``knots``, spline flows) every computed knot and interior derivative of every spline evaluation
    too -- the end knots -5 and the end derivatives 1 are exact in float32 and stay."""
    if rng is None:
        return OracleMAF(spec, flat, dtype=np.float64)

    def jitter(v):
        return v * (1.0 + EPS * rng.choice([-1.0, 1.0], size=np.shape(v)))
    o = OracleMAF(spec, flat, dtype=np.float64)
    for m in o._mats:
        for k, v in m.items():
            m[k] = jitter(v)
    if knots and spec.univariate == "rqs":
        def tables(xk, yk, dk):
            xk, yk, dk = xk.copy(), yk.copy(), dk.copy()
            xk[..., 1:], yk[..., 1:], dk[..., 1:-1] = jitter(xk[..., 1:]), jitter(yk[..., 1:]), jitter(dk[..., 1:-1])
            return xk, yk, dk
        o.tables = tables
    return o


def forward_terms(o, x):
    """``(z, ladj, sum_j |ladj term_j|)`` of the oracle ``o`` (same arithmetic as ``o.forward``)."""
    x = np.asarray(x, o.F)
    ladj = np.zeros(len(x), o.F)
    terms = np.zeros(len(x), np.float64)
    for t in range(o.spec.n_transforms):
        x, l = o._fwd(t, x)
        ladj = (ladj + l.sum(axis=1, dtype=o.F)).astype(o.F)
        terms += np.abs(l.astype(np.float64)).sum(axis=1)
    return x, ladj, terms


def evaluate(o, inp, direction):
    """Quantities of one evaluation: forward -> z, ladj, log_prob; inverse -> x, ladj."""
    D = o.spec.n_dim
    with np.errstate(all="ignore"):
        if direction == "forward":
            z, l, _ = forward_terms(o, inp)
            base = (-0.5 * (z.astype(o.F) ** 2).sum(axis=1, dtype=o.F) - o.F(0.5 * D * math.log(2 * math.pi))).astype(o.F)
            return {"z": z, "ladj": l, "log_prob": (base + l).astype(o.F)}
        x, l = o.inverse(inp)
        return {"x": x, "ladj": l}


def row_err(a, b, cancel=None):
    """Per-row error of ``a`` against the reference ``b`` (both float64-castable); non-finite ``a`` -> inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
        if a.ndim == 2:
            fin_a = np.isfinite(a).all(axis=1)
            d, ref = d.max(axis=1), np.abs(b).max(axis=1)
        else:
            fin_a = np.isfinite(a)
            ref = np.abs(b)
        if cancel is not None:
            ref = np.maximum(ref, cancel)
        e = d / np.maximum(ref, TINY)
    return np.where(fin_a, np.where(np.isfinite(e), e, np.inf), np.inf)


def _usable(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (np.abs(v) < F32_MAX)
    return ok.all(axis=1) if v.ndim == 2 else ok


class Reference:
    """Float64 reference of one direction of a flow on float32 inputs, with the sensitivity envelope of every row."""

    def __init__(self, spec, flat, inp, direction, seed=0, k=N_PERTURB, knots=True):
        rng = np.random.default_rng(seed)
        inp = np.asarray(inp, np.float32)
        self.spec, self.direction, self.inp = spec, direction, inp
        o = oracle64(spec, flat)
        self.ref = evaluate(o, inp.astype(np.float64), direction)
        with np.errstate(all="ignore"):
            if direction == "forward":
                terms = forward_terms(o, inp.astype(np.float64))[2]
                zb = 0.5 * (self.ref["z"] ** 2).sum(axis=1) + 0.5 * spec.n_dim * math.log(2 * math.pi)
                self.cancel = {"ladj": terms, "log_prob": terms + zb}
            else:
                self.cancel = {"ladj": forward_terms(o, np.nan_to_num(self.ref["x"]))[2]}
        self.ok = np.ones(len(inp), bool)
        for q, v in self.ref.items():
            self.ok &= _usable(v)
        self.env = {q: np.zeros(len(inp)) for q in self.ref}
        for _ in range(k):
            pin = inp.astype(np.float64) * (1.0 + EPS * rng.choice([-1.0, 1.0], size=inp.shape))
            p = evaluate(oracle64(spec, flat, rng, knots), pin, direction)
            for q, v in p.items():
                self.ok &= _usable(v)
                self.env[q] = np.maximum(self.env[q], row_err(v, self.ref[q], self.cancel.get(q)))

    def err(self, q, got):
        return row_err(got, self.ref[q], self.cancel.get(q))

    def check(self, q, got, what, bound=None, rows=None, raise_=True, f32=None, record=True):
        """The criterion on quantity ``q`` (rows ``rows``, default all).  Records the worst ``err/e`` and the worst error
        on well-conditioned rows (``C e_i <= bound``) in ``parity.MEASURED``; returns them and the median ratio.
        ``f32``: float32 evaluations of the same rows (the numpy oracle; for spline flows also ``KernelSplineOracle``, the
        kernels' formulas).  Where one's median ``err/e`` exceeds ``MEDIAN_BOUND`` (the median is beyond that float32
        arithmetic on these rows), the median bound is 1.25 x that median instead."""
        bound = bounds(self.spec)[q] if bound is None else bound
        sel = np.ones(len(self.inp), bool) if rows is None else np.isin(np.arange(len(self.inp)), rows)
        ok = self.ok & sel
        err, e = self.err(q, got), self.env[q]
        ratio = err / np.maximum(e, EPS)
        limit = np.maximum(bound, C * e)
        bad = ok & ~(err <= limit)
        well = ok & (C * e <= bound)
        stats = dict(worst_ratio=float(ratio[ok].max()) if ok.any() else 0.0,
                     median_ratio=float(np.median(ratio[ok])) if ok.any() else 0.0,
                     worst_well=float(err[well].max()) if well.any() else 0.0,
                     worst=float(err[ok].max()) if ok.any() else 0.0, rows=int(ok.sum()), failing=int(bad.sum()))
        fam = what.split(",")[0]
        for key, v in ((f"{fam} {q} err/e", stats["worst_ratio"]), (f"{fam} {q} err(well)", stats["worst_well"])):
            if record:
                parity.MEASURED[key] = max(parity.MEASURED.get(key, 0.0), v)
        msg = (f"{what} {q}: {stats['failing']} of {stats['rows']} rows beyond max({bound:g}, {C:g} e_i) "
               f"(worst err {stats['worst']:.3e}, worst err/e {stats['worst_ratio']:.3g}, median err/e {stats['median_ratio']:.3g})")
        med_bound = MEDIAN_BOUND
        for ref32 in ([] if f32 is None else f32 if isinstance(f32, list) else [f32]):
            r32 = self.err(q, ref32) / np.maximum(e, EPS)
            m32 = float(np.median(r32[ok])) if ok.any() else 0.0
            med_bound = max(med_bound, 1.25 * m32)
            msg += f" [float32 evaluation: median err/e {m32:.3g}, {int((ok & ~(self.err(q, ref32) <= limit)).sum())} rows beyond]"
        stats["median_bound"] = med_bound
        if raise_:
            assert stats["failing"] == 0, msg + f"; first rows {np.flatnonzero(bad)[:8].tolist()}"
            assert stats["median_ratio"] <= med_bound, msg
        return stats

    def passes(self, q, got, bound=None, rows=None):
        s = self.check(q, got, "probe", bound, rows, raise_=False, record=False)
        return s["failing"] == 0 and s["median_ratio"] <= MEDIAN_BOUND


def check(R, q, got, what, f32):
    """The criterion on ``got``.  ``f32``: float32 evaluations of the same rows (numpy oracle first).  Where one of them
    fails the row criterion, the quantity is ill-conditioned beyond the envelope on these rows (tests/test_flow_regimes_cpu.py:
    BEYOND_F32), and WHICH rows a float32 evaluation misses depends on its order of additions (numpy and the sequential
    oracle miss different rows of the affine x16 inverse by the same ~0.12).  There the kernel is held to be as good a
    float32 evaluation as those: at most twice as many rows beyond ``C e_i`` as the worst of them, a worst error at most
    twice theirs, and the median criterion on the rows every evaluation meets.  Returns the statistics (``beyond``: rows
    of ``got`` / of the worst float32 evaluation beyond ``C e_i``)."""
    lim = np.maximum(bounds(R.spec)[q], C * R.env[q])
    bad = [R.ok & ~(R.err(q, v) <= lim) for v in f32]
    beyond = np.logical_or.reduce(bad)
    if not beyond.any():
        s = R.check(q, got, what, f32=f32)
        s["beyond"] = (0, 0)
    else:
        held = np.flatnonzero(~beyond)
        s = R.check(q, got, what, rows=held, f32=f32, raise_=False)
        assert s["median_ratio"] <= s["median_bound"], (what, q, s)
        err = R.err(q, got)
        bad_k = R.ok & ~(err <= lim)
        n_e = max(int(b.sum()) for b in bad)
        worst_e = max(float(R.err(q, v)[b].max()) for v, b in zip(f32, bad) if b.any())
        worst_k = float(err[bad_k].max()) if bad_k.any() else 0.0
        key = f"{what.split(',')[0]} {q} rows beyond C e (kernel / float32)"
        print(f"{what} {q}: beyond C e_i on {int(bad_k.sum())} rows (worst err {worst_k:.3g}); float32 evaluations: up to "
              f"{n_e} rows (worst err {worst_e:.3g})")
        parity.MEASURED[key] = max(parity.MEASURED.get(key, 0.0), float(bad_k.sum()))
        assert bad_k.sum() <= 2 * n_e and worst_k <= 2 * worst_e, (what, q, int(bad_k.sum()), n_e, worst_k, worst_e)
        s["beyond"] = (int(bad_k.sum()), n_e)
    print(f"{what} {q}: worst err/e {s['worst_ratio']:.3g}, median {s['median_ratio']:.3g} (bound {s['median_bound']:.3g}), "
          f"worst err {s['worst']:.2e}, well-conditioned rows {s['worst_well']:.2e}")
    return s


# ----------------------------------------------------------------- the kernels' spline arithmetic, modelled in float32
_F = np.float32
_INV_LS = _F(1.0) / _F(-6.907755278982137)          # csrc/maf_common.h PMC_LOG_SLOPE, csrc/rqs.h RQS_INV_LS


def _k_rcp(v):
    return (_F(1.0) / v).astype(_F)                  # v_rcp_f32 (<= 1 ulp): modelled correctly rounded


def _k_exp(v):
    return np.exp2((v * _F(1.4426950408889634)).astype(_F)).astype(_F)    # rqs_exp: exp2 of the ROUNDED product


def _k_log(v):
    return (np.log2(v).astype(_F) * _F(0.6931471805599453)).astype(_F)   # rqs_log


def _k_knots(v, K):
    """``rqs_softmax_knots_t``: soft clip by reciprocal, exp of the shifted values, knots by a running sum of
    ``c_j * (1 / sum)``."""
    c = (v * _k_rcp(_F(1.0) + np.abs(v * (_F(2.0) * _INV_LS)))).astype(_F)
    c = _k_exp((c - c.max(axis=-1, keepdims=True)).astype(_F))
    tot = np.zeros(v.shape[:-1], _F)
    for j in range(K):
        tot = (tot + c[..., j]).astype(_F)
    rs = _k_rcp(tot)
    kn = [np.full(v.shape[:-1], _F(-5.0))]
    cum = np.zeros(v.shape[:-1], _F)
    for j in range(K):
        cum = (cum + (c[..., j] * rs).astype(_F)).astype(_F)
        kn.append((_F(5.0) * (_F(2.0) * cum - _F(1.0))).astype(_F))
    return np.stack(kn, -1)


def _k_tables(phi, K, knots_of):
    xk, yk = _k_knots(phi[..., :K], K), _k_knots(phi[..., K:2 * K], K)
    return xk, yk, knots_of(xk, yk)


def _k_bin(phi, K, xk, yk, kn, v):
    """``rqs_select_t``: inside ``(kn_0, kn_K]``, bin = last j >= 1 with ``kn_j < v``; the derivatives by exp of the
    soft-clipped raw values (end knots: exp(0) = 1)."""
    inside = (v > kn[..., 0]) & (v <= kn[..., K])
    k = np.zeros(v.shape, np.int64)
    for j in range(1, K):
        k = np.where(kn[..., j] < v, j, k)
    take = lambda a, i: np.take_along_axis(a, i[..., None], -1)[..., 0]
    raw = phi[..., 2 * K:]
    clip = (raw * _k_rcp(_F(1.0) + np.abs(raw * _INV_LS))).astype(_F)
    clip = np.concatenate([np.zeros(v.shape + (1,), _F), clip, np.zeros(v.shape + (1,), _F)], -1)
    d0, d1 = _k_exp(take(clip, k)), _k_exp(take(clip, k + 1))
    return inside, take(xk, k), take(xk, k + 1), take(yk, k), take(yk, k + 1), d0, d1


class KernelSplineOracle(OracleMAF):
    """The float32 oracle with the spline evaluated the way ``csrc/rqs.h`` evaluates it (``rqs_forward_t`` /
    ``rqs_inverse_t``): reciprocals instead of divisions, ``exp2`` of a rounded product for ``exp``, ``log2`` times ln 2
    for ``log``, knots from a running sum of ``c_j / sum``, the kernels' bin search.  The hardware's own ~1 ulp of
    ``v_rcp`` / ``v_exp`` / ``v_log`` is not modelled (they are taken as correctly rounded): what this shows is the error
    the kernels' FORMULAS carry, with any float32 arithmetic."""

    def _fwd(self, t, x):
        if self.spec.univariate == "affine":
            return super()._fwd(t, x)
        K = self.spec.bins
        phi = self._phi(t, x)
        xk, yk, kn = _k_tables(phi, K, lambda xk, yk: xk)
        inside, x0, x1, y0, y1, d0, d1 = _k_bin(phi, K, xk, yk, kn, x)
        with np.errstate(all="ignore"):
            dx, dy = (x1 - x0).astype(_F), (y1 - y0).astype(_F)
            rdx = _k_rcp(dx)
            s = (dy * rdx).astype(_F)
            z = np.where(inside, (x - x0) * rdx, _F(0.0)).astype(_F)
            u = (z * (_F(1.0) - z)).astype(_F)
            rden = _k_rcp((s + (d0 + d1 - _F(2.0) * s) * u).astype(_F))
            yy = (y0 + dy * (s * z * z + d0 * u) * rden).astype(_F)
            jac = (s * s * (_F(2.0) * s * u + d0 * (_F(1.0) - z) * (_F(1.0) - z) + d1 * z * z) * (rden * rden)).astype(_F)
            return np.where(inside, yy, x).astype(_F), np.where(inside, _k_log(jac), _F(0.0)).astype(_F)

    def _inv(self, t, xcur, y):
        if self.spec.univariate == "affine":
            return super()._inv(t, xcur, y)
        K = self.spec.bins
        phi = self._phi(t, xcur)
        xk, yk, kn = _k_tables(phi, K, lambda xk, yk: yk)
        inside, x0, x1, y0, y1, d0, d1 = _k_bin(phi, K, xk, yk, kn, y)
        with np.errstate(all="ignore"):
            dx, dy = (x1 - x0).astype(_F), (y1 - y0).astype(_F)
            s = (dy * _k_rcp(dx)).astype(_F)
            yr = np.where(inside, y - y0, _F(0.0)).astype(_F)
            e = (d0 + d1 - _F(2.0) * s).astype(_F)
            qa = (dy * (s - d0) + yr * e).astype(_F)
            qb = (dy * d0 - yr * e).astype(_F)
            qc = (-s * yr).astype(_F)
            z = (_F(2.0) * qc * _k_rcp((-qb - np.sqrt((qb * qb - _F(4.0) * qa * qc).astype(_F))).astype(_F))).astype(_F)
            u = (z * (_F(1.0) - z)).astype(_F)
            rden = _k_rcp((s + e * u).astype(_F))
            jac = (s * s * (_F(2.0) * s * u + d0 * (_F(1.0) - z) * (_F(1.0) - z) + d1 * z * z) * (rden * rden)).astype(_F)
            return np.where(inside, x0 + z * dx, y).astype(_F), np.where(inside, _k_log(jac), _F(0.0)).astype(_F)


class SequentialOracle(OracleMAF):
    """The float32 oracle with every dot product of the hyper-network accumulated one term at a time in index order (no
    BLAS blocking): another valid float32 evaluation.  Where it and the numpy oracle disagree with the float64 reference
    on DIFFERENT rows, the error of those rows is float32's, and which rows it hits depends on the order of additions
    (measured: the affine flow x16's inverse log-determinant, 10 / 4 rows of 192 beyond ``C e_i``)."""

    def _phi(self, t, x):
        m = self._mats[t]

        def mm(a, W):
            acc = np.zeros((a.shape[0], W.shape[0]), np.float32)
            for k in range(W.shape[1]):
                acc = (acc + a[:, k:k + 1] * W[:, k][None, :]).astype(np.float32)
            return acc
        h = np.maximum(mm(x, m["W0"]) + m["b0"], 0).astype(np.float32)
        h = np.maximum(h + (mm(h, m["W1"]) + m["b1"]), 0).astype(np.float32)
        h = np.maximum(h + (mm(h, m["W2"]) + m["b2"]), 0).astype(np.float32)
        return (mm(h, m["W3"]) + m["b3"]).astype(np.float32).reshape(len(x), self.spec.n_dim, self.spec.n_out)
