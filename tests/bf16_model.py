"""Rounding-exact numpy restatement of the bf16 matrix-core kernels, and the criterion they are held to against it
(``tests/test_bf16_model_cpu.py``, ``tests/test_gpu_bf16_model.py``).

Why: the parity tests of ``csrc/maf_forward_bf16.hip`` and ``csrc/maf_train_bf16.hip`` compare with the plain float32
oracle, so their tolerances (3e-2; 2e-2 / 1e-1) have to absorb the legitimate bf16 rounding and leave little to catch a
wrong kernel.  This model rounds to bf16 exactly where the kernels do, so that what is left between a correct kernel
and the model evaluated in float64 is float32 accumulation noise (~2^-23) and rare FLIPS: a value that lands within
that noise of a bf16 rounding boundary rounds the other way and propagates.

Where the kernels round (read off ``maf_forward_bf16_kernel`` and ``maf_wide_phase_kernel``; ``to_bf16`` of
``csrc/bf16.h``), per transform:

* weights: ``rne(W * mask)`` (``pmc_maf_pack_bf16``); biases stay float32;
* the matmul input ``rne(x_t)``; the affine map uses the unrounded ``x_t``;
* ``h0 = rne(relu(W0 xb + b0))``, ``h_k = rne(relu((W_k h_{k-1} + b_k) + h_{k-1}))`` with the ROUNDED ``h_{k-1}``;
* the output layer, ``ls = raw / (1 + |raw / log 1e-3|)``, ``y = x e^{ls} + shift``, the log-determinant and the
  log-density are float32, never rounded;
* trainer backward: ``do = rne([gy, (gy x e^{ls} - c) / den^2])``, ``da2 = rne(gate(h2) W3^T do)``,
  ``da1 = rne(gate(h1) (W2^T da2 + da2))``, ``da0 = rne(gate(h0) (W1^T da1 + da1))``; ``dL/dx = W0^T da0 + gy e^{ls}``
  stays float32; weight gradients are products of the rounded operands (``dW3 = do^T h2``, ``dW2 = da2^T h1``,
  ``dW1 = da1^T h0``, ``dW0 = da0^T xb``), bias gradients the column sums of the rounded ``do`` / ``da``.

The model is parametrised by dtype: float64 is the reference, float32 (in several contraction orders) the yardstick a
kernel's distance from the reference is measured with -- in the same test, never as a constant (the convention of
``tests/flow_regimes.py``).  Hidden units are kept in the kernels' slot order (``MAFSpec.slot_unit``: sorted by degree,
padded) so that contraction orders and the k-steps of a tile mean what they mean in the kernels; the masks are the
oracle's own (``oracle.maf.zuko_masks``).
"""
from __future__ import annotations

import math

import numpy as np

from oracle.maf import LOG_SLOPE, zuko_masks

DEFECTS = ("truncate", "drop_kstep", "residual_unrounded", "act_unrounded", "da0_unrounded", "no_backward_residual")
FORWARD_DEFECTS = DEFECTS[:4]
ORDERS = ("natural", "reversed", "split4", "pairwise")
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------- rounding
def bf16_bits(v, truncate=False):
    """float32 -> bf16 bit patterns (uint16) by the integer arithmetic of ``fbf::to_bf16``: round to nearest even, NaN
    stays NaN with the quiet bit set.  ``truncate``: the defect (drop the low half)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    if truncate:
        return (u >> np.uint64(16)).astype(np.uint16)
    nan = (u & np.uint64(0x7fffffff)) > np.uint64(0x7f800000)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xffff)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)) & np.uint64(0xffff), r).astype(np.uint16)


def rne(v, truncate=False):
    """float32 -> bf16 -> float32."""
    return (bf16_bits(v, truncate).astype(np.uint32) << np.uint32(16)).view(np.float32)


def crafted_vector(seed=0, n_random=100_000):
    """float32 values at the edges of the conversion: exact ties above an even and above an odd bf16 mantissa, one ulp
    either side of a tie, +-0, denormals, +-inf, the largest finites (they round to inf), and random bit patterns.
    Returns ``(values, is_nan)``."""
    bits = []
    for hi in (0x3f80, 0x3f81, 0x4049, 0x404a, 0x0080, 0x0081, 0x7f7e, 0x7f7f, 0x0000, 0x0001):
        for lo in (0x8000, 0x7fff, 0x8001, 0x0000, 0x0001, 0xffff):
            for sign in (0, 0x8000):
                bits.append(((hi | sign) << 16) | lo)
    bits += [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00008000, 0x00018000,
             0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff, 0xff7f8000,
             0x7fc00000, 0xffc00000, 0x7f800001, 0x7fbfffff, 0xff800001, 0x7fffffff]
    rnd = np.random.default_rng(seed).integers(0, 2 ** 32, size=n_random + n_random // 64 + 64, dtype=np.uint64)
    rnd = rnd[(rnd & 0x7fffffff) <= 0x7f800000][:n_random]                 # (non-NaN; the NaN patterns are listed above)
    assert len(rnd) == n_random
    u = np.concatenate([np.asarray(bits, np.uint64), rnd]).astype(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    return u.view(np.float32), nan


# ------------------------------------------------------------------------------------------------------ contractions
def _matmul(a, w, order):
    """``a (N, K) @ w (M, K)^T`` in the dtype of the operands; ``order`` only matters in float32."""
    K = a.shape[1]
    if order == "natural" or K <= 32:
        return a @ w.T
    if order == "reversed":
        return np.ascontiguousarray(a[:, ::-1]) @ np.ascontiguousarray(w[:, ::-1]).T
    if order == "split4":                                    # the k-steps of 32 dealt to four wavefronts
        ks = (K + 31) // 32
        cut = [32 * ((ks * i) >> 2) for i in range(5)]
        cut[4] = K
        p = [a[:, cut[i]:cut[i + 1]] @ w[:, cut[i]:cut[i + 1]].T if cut[i + 1] > cut[i] else
             np.zeros((a.shape[0], w.shape[0]), a.dtype) for i in range(4)]
        return (p[0] + p[1]) + (p[2] + p[3])
    if order == "pairwise":
        parts = [a[:, k:k + 32] @ w[:, k:k + 32].T for k in range(0, K, 32)]
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        return parts[0]
    raise KeyError(order)


# ------------------------------------------------------------------------------------------------------------- model
class BF16Model:
    """The affine flow ``spec`` with float32 parameters ``flat`` as the bf16 kernels evaluate it.

    ``dtype``: float64 (reference) or float32 (yardstick); ``order``: contraction order of every product (float32);
    ``rounding=False``: no bf16 rounding anywhere (then the model is the plain flow: the CPU test holds it to float64
    autograd); ``defect``: one of ``DEFECTS`` (CPU discrimination test only)."""

    def __init__(self, spec, flat, dtype=np.float64, order="natural", rounding=True, defect=None):
        assert spec.univariate == "affine"
        assert defect is None or defect in DEFECTS
        assert order in ORDERS
        self.spec, self.F, self.order, self.rounding, self.defect = spec, np.dtype(dtype).type, order, rounding, defect
        flat = np.asarray(flat, np.float32)
        assert flat.shape == (spec.n_params,)
        D, Hp = spec.n_dim, spec.Hp
        su = np.asarray(spec.slot_unit)
        self.live = live = np.flatnonzero(su >= 0)
        unit = su[live]
        self.layers, self.index = [], []
        for t in range(spec.n_transforms):
            order_t = np.arange(D) if t % 2 == 0 else np.arange(D)[::-1]
            M = zuko_masks(order_t, 2, spec.hidden)
            base = t * spec.params_per_transform
            lay, idx = {}, {}
            for k, (wn, bn) in enumerate((("W0", "b0"), ("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
                off, _ = spec.offsets[wn]
                rows, cols = spec.shapes()[wn]
                canon = base + off + np.arange(rows * cols).reshape(rows, cols)
                canon = np.where(M[k], canon, -1)
                w = np.where(M[k], spec.view(flat, t, wn), np.float32(0.0)).astype(np.float32)
                if k > 0:                                    # hidden inputs: slot order, zero columns at the padding
                    c2, w2 = np.full((rows, Hp), -1, np.int64), np.zeros((rows, Hp), np.float32)
                    c2[:, live], w2[:, live] = canon[:, unit], w[:, unit]
                    canon, w = c2, w2
                if k < 3:                                    # hidden outputs: slot order, zero rows at the padding
                    c2, w2 = np.full((Hp, canon.shape[1]), -1, np.int64), np.zeros((Hp, w.shape[1]), np.float32)
                    c2[live], w2[live] = canon[unit], w[unit]
                    canon, w = c2, w2
                boff, bsz = spec.offsets[bn]
                bcanon = base + boff + np.arange(bsz)
                b = spec.view(flat, t, bn).astype(np.float32)
                if k < 3:
                    b2, bc2 = np.zeros(Hp, np.float32), np.full(Hp, -1, np.int64)
                    b2[live], bc2[live] = b[unit], bcanon[unit]
                    b, bcanon = b2, bc2
                lay[wn], lay[bn] = self._round(w).astype(self.F), b.astype(self.F)
                idx[wn], idx[bn] = canon, bcanon
            if defect == "drop_kstep":                       # layer 1, last hidden tile: its last k-step of 32 is missing
                Tt = spec.nT - 1
                last = (Tt >> 1) if spec.tri_ok else (Hp + 31) // 32 - 1
                w1 = lay["W1"].copy()
                w1[16 * Tt:16 * Tt + 16, 32 * last:32 * last + 32] = 0
                lay["W1_forward"] = w1
            self.layers.append(lay)
            self.index.append(idx)

    # ---- rounding of a value of the model's dtype, where the kernel stores bf16
    def _round(self, v, what=None):
        if not self.rounding:
            return np.asarray(v)
        if what is not None and what == {"act_unrounded": "h2", "da0_unrounded": "da0"}.get(self.defect):
            return np.asarray(v)
        return rne(np.asarray(v, np.float32), truncate=self.defect == "truncate").astype(self.F)

    def _mm(self, a, w):
        return _matmul(a, w, self.order).astype(self.F)

    def _transform(self, t, x):
        """One transform at ``x`` (N, D): everything the backward pass needs."""
        F, L = self.F, self.layers[t]
        zero = F(0.0)
        xb = self._round(x)
        a0 = np.maximum(self._mm(xb, L["W0"]) + L["b0"], zero)
        h0 = self._round(a0, "h0")
        r0 = a0 if self.defect == "residual_unrounded" else h0
        a1 = np.maximum((self._mm(h0, L.get("W1_forward", L["W1"])) + L["b1"]) + r0, zero)
        h1 = self._round(a1, "h1")
        r1 = a1 if self.defect == "residual_unrounded" else h1
        a2 = np.maximum((self._mm(h1, L["W2"]) + L["b2"]) + r1, zero)
        h2 = self._round(a2, "h2")
        out = self._mm(h2, L["W3"]) + L["b3"]                # canonical rows 2 f + s
        shift, raw = out[:, 0::2], out[:, 1::2]
        den = F(1.0) + np.abs(raw / F(LOG_SLOPE))
        ls = raw / den
        y = x * np.exp(ls) + shift
        return dict(x=x, xb=xb, h0=h0, h1=h1, h2=h2, ls=ls.astype(F), dd=(F(1.0) / (den * den)).astype(F), y=y.astype(F))

    def forward(self, x, keep=False):
        """``{"z", "ladj", "log_prob", "terms"}`` (``terms``: ``sum |ls|`` per row, the condition of the ladj sum);
        ``keep``: also the per-transform records under ``"tape"``."""
        F = self.F
        x = np.asarray(x, np.float32).astype(F)
        D = self.spec.n_dim
        ladj, terms, tape = np.zeros(len(x), F), np.zeros(len(x), np.float64), []
        with np.errstate(all="ignore"):
            for t in range(self.spec.n_transforms):
                r = self._transform(t, x)
                ladj = (ladj + r["ls"].sum(axis=1, dtype=F)).astype(F)
                terms += np.abs(r["ls"].astype(np.float64)).sum(axis=1)
                x = r["y"]
                if keep:
                    tape.append(r)
            lp = ((F(-0.5) * (x * x).sum(axis=1, dtype=F) - F(HALF_LOG_2PI) * F(D)) + ladj).astype(F)
        out = {"z": x, "ladj": ladj, "log_prob": lp, "terms": terms}
        if keep:
            out["tape"] = tape
        return out

    def loss_and_grad(self, x, w=None):
        """``(loss, gradient over the canonical flat vector)`` of ``Flow.fit``'s batch loss, as ``maf_wide_phase_kernel``
        forms them.  Masked entries of the gradient are exactly zero."""
        F, spec = self.F, self.spec
        fw = self.forward(x, keep=True)
        n = len(fw["z"])
        if w is None:
            c = np.ones(n, F)
        else:
            wf = np.asarray(w, np.float32).astype(F)
            c = (wf * F(1000.0) / wf.sum(dtype=F)).astype(F)
        loss = float((-(c * fw["log_prob"])).sum(dtype=F))
        g = np.zeros(spec.n_params, np.float64)
        gy = (c[:, None] * fw["z"]).astype(F)
        back = F(0.0) if self.defect == "no_backward_residual" else F(1.0)
        for t in reversed(range(spec.n_transforms)):
            r, L, I = fw["tape"][t], self.layers[t], self.index[t]
            e = np.exp(r["ls"])
            do = np.empty((n, 2 * spec.n_dim), F)
            do[:, 0::2] = gy
            do[:, 1::2] = (gy * r["x"] * e - c[:, None]) * r["dd"]
            do = self._round(do, "do")
            da2 = self._round(np.where(r["h2"] > 0, self._mm(do, L["W3"].T), F(0.0)), "da2")
            da1 = self._round(np.where(r["h1"] > 0, self._mm(da2, L["W2"].T) + back * da2, F(0.0)), "da1")
            da0 = self._round(np.where(r["h0"] > 0, self._mm(da1, L["W1"].T) + back * da1, F(0.0)), "da0")
            gy = (self._mm(da0, L["W0"].T) + gy * e).astype(F)
            for wn, bn, d, h in (("W3", "b3", do, r["h2"]), ("W2", "b2", da2, r["h1"]), ("W1", "b1", da1, r["h0"]),
                                 ("W0", "b0", da0, r["xb"])):
                dw = self._mm(np.ascontiguousarray(d.T), np.ascontiguousarray(h.T))          # the contraction runs over the rows
                ok = I[wn] >= 0
                g[I[wn][ok]] = dw[ok]
                db = d.sum(axis=0, dtype=F)
                ok = I[bn] >= 0
                g[I[bn][ok]] = db[ok]
        return loss, g


# --------------------------------------------------------------------------------------------------------- criterion
FWD_QUANTITIES = ("z", "ladj", "log_prob")
FWD_FLOOR = 2.0 ** -20
FWD_C = 8.0                  # x the yardstick's 75th percentile
FWD_FLIP_SHARE = 0.25        # rows beyond the bound, kernel
FWD_FLIP_SHARE_F32 = 0.10    # rows beyond the bound, float32 model: the shapes are chosen so that this holds
PLAIN_BOUND = 3e-2           # tests/test_gpu_config.py: the bf16 forward against the plain float32 oracle
TRAIN_C = 4.0                # x the largest of the four float32 orders
LOSS_FLOOR = 2.0 ** -20
GRAD_FLOOR = 1e-6
TINY = np.finfo(np.float64).tiny


def forward_row_err(q, got, ref):
    """Per-row error of quantity ``q`` against the reference evaluation ``ref`` (a ``forward`` dict), measured like
    ``parity.close_rel``: a vector by ``max_j |a - b| / max_j |b|``, the log-determinant against ``max(|b|, sum |terms|)``,
    the log-density against ``max(|b|, sum |terms| + |z|^2 / 2)`` (``OracleMAF.ladj_abs_terms``).  Non-finite -> inf."""
    a, b = np.asarray(got, np.float64), np.asarray(ref[q], np.float64)
    with np.errstate(all="ignore"):
        if q == "z":
            d, s, fin = np.abs(a - b).max(axis=1), np.abs(b).max(axis=1), np.isfinite(a).all(axis=1)
        else:
            d, fin = np.abs(a - b), np.isfinite(a)
            s = np.maximum(np.abs(b), ref["terms"])
            if q == "log_prob":
                s = np.maximum(np.abs(b), ref["terms"] + 0.5 * (np.asarray(ref["z"], np.float64) ** 2).sum(axis=1))
        e = d / np.maximum(s, TINY)
    return np.where(fin & np.isfinite(e), e, np.inf)


def forward_verdict(err, e32):
    """The forward criterion on one quantity: ``err`` the per-row errors of the evaluation under test, ``e32`` those of
    the float32 model, both against the float64 model on the same rows.  Returns a dict with ``ok`` and the figures."""
    err, e32 = np.asarray(err, np.float64), np.asarray(e32, np.float64)
    b = max(FWD_C * float(np.percentile(e32, 75)), FWD_FLOOR)
    p75 = float(np.percentile(err, 75))
    share, share32 = float((err > b).mean()), float((e32 > b).mean())
    return dict(bound=b, p75=p75, p75_f32=float(np.percentile(e32, 75)), flipped=share, flipped_f32=share32,
                worst=float(err.max()), worst_f32=float(e32.max()),
                ok=bool(p75 <= b and share <= FWD_FLIP_SHARE and share32 <= FWD_FLIP_SHARE_F32))


def blocks(spec):
    """``(name, slice)`` of every canonical tensor of the flat parameter vector."""
    for t in range(spec.n_transforms):
        for name, (off, sz) in spec.offsets.items():
            b = t * spec.params_per_transform + off
            yield f"t{t}.{name}", slice(b, b + sz)


def train_measures(spec, loss, g, loss_ref, g_ref):
    """``{"loss": relative error, "grad": relative L2 error, "t0.W0": ..., ...}`` against the reference."""
    g, g_ref = np.asarray(g, np.float64), np.asarray(g_ref, np.float64)
    m = {"loss": abs(loss - loss_ref) / max(abs(loss_ref), TINY),
         "grad": float(np.linalg.norm(g - g_ref) / max(np.linalg.norm(g_ref), TINY))}
    for name, sl in blocks(spec):
        m[name] = float(np.linalg.norm(g[sl] - g_ref[sl]) / max(np.linalg.norm(g_ref[sl]), TINY))
    return {k: (v if np.isfinite(v) else np.inf) for k, v in m.items()}


class TrainReference:
    """Float64 model and the float32 yardstick (the largest of the four contraction orders, per measure) of one batch."""

    def __init__(self, spec, flat, x, w=None):
        self.spec = spec
        self.loss, self.grad = BF16Model(spec, flat).loss_and_grad(x, w)
        self.yard = {}
        for order in ORDERS:
            l32, g32 = BF16Model(spec, flat, np.float32, order).loss_and_grad(x, w)
            for k, v in train_measures(spec, l32, g32, self.loss, self.grad).items():
                self.yard[k] = max(self.yard.get(k, 0.0), v)

    def verdict(self, loss, g):
        m = train_measures(self.spec, loss, g, self.loss, self.grad)
        lim = {k: max(TRAIN_C * self.yard[k], LOSS_FLOOR if k == "loss" else GRAD_FLOOR) for k in m}
        bad = [k for k in m if not m[k] <= lim[k]]
        ratio = {k: m[k] / max(self.yard[k], (LOSS_FLOOR if k == "loss" else GRAD_FLOOR) / TRAIN_C) for k in m}
        worst = max((k for k in m if k not in ("loss", "grad")), key=lambda k: ratio[k])
        return dict(ok=not bad, failing=bad, measures=m, limits=lim, ratio=ratio, worst_tensor=worst,
                    summary=(f"loss {m['loss']:.2e} (yardstick {self.yard['loss']:.2e}), gradient {m['grad']:.2e} "
                             f"({self.yard['grad']:.2e}), worst tensor {worst} {m[worst]:.2e} ({self.yard[worst]:.2e})"))
