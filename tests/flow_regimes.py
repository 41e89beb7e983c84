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


def knot_rows(spec, flat, base, inverse=False):
    """Rows of ``base`` (cycled) whose first-ranked coordinate -- of transform 0 for the forward map, of the last transform
    for the inverse -- sits exactly on each float32 knot of the oracle and one ulp either side.  Returns ``(rows, where)``
    with ``where[i] = (knot index, ulps)``."""
    t = spec.n_transforms - 1 if inverse else 0
    xk, yk = constant_knots(spec, flat, t)
    kn = yk if inverse else xk
    f = first_feature(spec, t)
    rows, where = [], []
    for j in range(len(kn)):
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


def with_nonfinite(x):
    """``x`` with NaN / +inf / -inf in one coordinate of the rows ``NONFINITE_ROWS``; returns ``(bad, rows)``."""
    bad = np.array(x, np.float32)
    n, D = bad.shape
    rows = sorted({r % n for r in NONFINITE_ROWS})
    for i, r in enumerate(rows):
        bad[r, (5 * i) % D] = (np.nan, np.inf, -np.inf)[i % 3]
    return bad, rows


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
