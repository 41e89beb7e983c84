"""Rounding-exact numpy restatement of the bf16 matrix-core forward kernel's SPLINE instances (``csrc/maf_forward_bf16.h``,
``UNI`` = 4 / 8 / 16), the counterpart of ``tests/bf16_model.py`` for the neural spline flows
(``tests/test_bf16_spline_model_cpu.py``, ``tests/test_gpu_bf16_spline.py``).

The hyper-network rounds to bf16 exactly where the kernel does, per transform:

* weights ``rne(W * mask)`` (``pmc_maf_pack_bf16``); the biases, ``b3`` included, stay float32;
* ``rne(x_t)`` into layer 0;
* ``h0 = rne(relu(W0 xb + b0))``, ``h_k = rne(relu((W_k h_{k-1} + b_k) + h_{k-1}))`` with the ROUNDED ``h_{k-1}``;
* the output panel ``phi = W3 h2 + b3`` over all k-steps of the rounded ``h2``, the spline, the log-determinant and the
  log-density are never rounded, and the spline is evaluated at the UNROUNDED ``x_t``.

Two evaluations of that model: float64 with the oracle's spline (``OracleMAF``: the reference) and float32 with the
kernels' spline formulas (``flow_regimes.KernelSplineOracle``: the yardstick, measured in the same test on the same rows).
Hidden units are kept in the kernels' slot order (``MAFSpec.slot_unit``), so that ``bf16_model._matmul``'s contraction
orders and "the last k-step" mean what they mean in the kernel.  The criterion and its constants are ``bf16_model``'s,
unchanged: ``forward_row_err`` / ``forward_verdict`` with ``FWD_C`` = 8, ``FWD_FLOOR`` = 2^-20, ``FWD_FLIP_SHARE`` = 25 %,
``FWD_FLIP_SHARE_F32`` = 10 %.
"""
from __future__ import annotations

import numpy as np

import bf16_model as bm
import flow_regimes as fr
from oracle.maf import OracleMAF

# single defects the criterion has to reject (tests/test_bf16_spline_model_cpu.py)
DEFECTS = ("truncate",            # truncation instead of round-to-nearest-even, everywhere
           "drop_panel_kstep",    # the output panel's products stop one k-step of 32 early
           "h2_unrounded",        # the output panel reads the float h2
           "spline_x_rounded",    # the spline is evaluated at rne(x)
           "b3_rounded",          # the output bias through bf16
           "swap_widths_heights")  # the panel's rows [0, K) and [K, 2K) of a feature exchanged


class _RoundedHyperNetwork:
    """Mixin in front of ``OracleMAF`` (or a subclass): the masked weights in slot order, rounded; ``_phi`` rounding its
    input and activations.  ``rounding=False``: the plain flow (then the float64 model IS ``OracleMAF(float64)`` up to the
    order of its sums).  ``order``: ``bf16_model.ORDERS``; ``defect``: one of ``DEFECTS``."""

    def __init__(self, spec, flat, dtype, order="natural", rounding=True, defect=None):
        assert spec.univariate == "rqs"
        assert order in bm.ORDERS and (defect is None or defect in DEFECTS)
        super().__init__(spec, flat, dtype=dtype)
        self.order, self.rounding, self.defect = order, rounding, defect
        F, Hp = self.F, spec.Hp
        su = np.asarray(spec.slot_unit)
        live = np.flatnonzero(su >= 0)
        unit = su[live]
        for m in self._mats:                                 # canonical unit order -> slot order, zeros at the padding
            for k in ("W0", "W1", "W2", "W3"):
                w = np.asarray(m[k], np.float32)             # (float32 parameter x 0/1 mask: exact)
                if k != "W0":
                    w2 = np.zeros((w.shape[0], Hp), np.float32)
                    w2[:, live] = w[:, unit]
                    w = w2
                if k != "W3":
                    w2 = np.zeros((Hp, w.shape[1]), np.float32)
                    w2[live] = w[unit]
                    w = w2
                m[k] = self._round(w).astype(F)
            for k in ("b0", "b1", "b2"):
                b = np.zeros(Hp, F)
                b[live] = m[k][unit]
                m[k] = b
            if defect == "b3_rounded":
                m["b3"] = bm.rne(np.asarray(m["b3"], np.float32)).astype(F)
            if defect == "drop_panel_kstep":
                m["W3"] = m["W3"].copy()
                m["W3"][:, 32 * ((Hp + 31) // 32 - 1):] = 0

    def _round(self, v, what=None):
        if not self.rounding or (what == "h2" and self.defect == "h2_unrounded"):
            return np.asarray(v)
        return bm.rne(np.asarray(v, np.float32), truncate=self.defect == "truncate").astype(self.F)

    def _mm(self, a, w):
        return bm._matmul(a, w, self.order).astype(self.F)

    def _phi(self, t, x):
        F, m = self.F, self._mats[t]
        zero = F(0.0)
        xb = self._round(np.asarray(x, F))
        h0 = self._round(np.maximum(self._mm(xb, m["W0"]) + m["b0"], zero))
        h1 = self._round(np.maximum((self._mm(h0, m["W1"]) + m["b1"]) + h0, zero))
        h2 = self._round(np.maximum((self._mm(h1, m["W2"]) + m["b2"]) + h1, zero), "h2")
        phi = (self._mm(h2, m["W3"]) + m["b3"]).astype(F).reshape(len(x), self.spec.n_dim, self.spec.n_out)
        if self.defect == "swap_widths_heights":
            K = self.spec.bins
            phi = np.concatenate([phi[..., K:2 * K], phi[..., :K], phi[..., 2 * K:]], -1)
        return phi

    def _fwd(self, t, x):
        if self.defect == "spline_x_rounded":
            x = self._round(np.asarray(x, self.F))
        return super()._fwd(t, x)

    def forward(self, x):
        """``{"z", "ladj", "log_prob", "terms"}`` in the model's dtype (``terms``: ``sum |ladj terms|`` per row in float64, the
        condition of the log-determinant's sum) -- the dictionary ``bf16_model.forward_row_err`` measures against."""
        F, D = self.F, self.spec.n_dim
        with np.errstate(all="ignore"):
            z, ladj, terms = fr.forward_terms(self, np.asarray(x, np.float32).astype(F))
            lp = ((F(-0.5) * (z * z).sum(axis=1, dtype=F) - F(bm.HALF_LOG_2PI) * F(D)) + ladj).astype(F)
        return {"z": z, "ladj": ladj, "log_prob": lp, "terms": terms}


class _Model64(_RoundedHyperNetwork, OracleMAF):
    pass


class _Model32(_RoundedHyperNetwork, fr.KernelSplineOracle):
    pass


def SplineBF16Model(spec, flat, dtype=np.float64, order="natural", rounding=True, defect=None):
    """The spline flow ``spec`` with float32 parameters ``flat`` as the bf16 kernel evaluates it: float64 with the oracle's
    spline (the reference) or float32 with the kernels' spline formulas (the yardstick)."""
    cls = {np.float64: _Model64, np.float32: _Model32}[np.dtype(dtype).type]
    return cls(spec, flat, np.dtype(dtype).type, order, rounding, defect)


def verdicts(got, ref, f32):
    """``bf16_model.forward_verdict`` of every quantity: ``got`` the evaluation under test, ``ref`` / ``f32`` the float64 /
    float32 model on the same rows (``forward`` dictionaries)."""
    return {q: bm.forward_verdict(bm.forward_row_err(q, got[q], ref), bm.forward_row_err(q, f32[q], ref))
            for q in bm.FWD_QUANTITIES}


# ------------------------------------------------------------------------------------------ what the GPU test runs on
ROWS = (1, 15, 16, 17, 33)
# (D, T, hidden, bins): extra row counts (None: n = 33 only)
SHAPES = {
    (2, 2, 32, 8): (),             # tri_ok false
    (7, 2, 32, 8): (4113,),        # odd tile count; two row sets, the last workgroup's second set holds one row
    (17, 2, 64, 8): (),            # the second panel holds one rank
    (33, 2, 128, 8): (),           # two input k tiles
    (40, 2, 256, 8): (),           # sixteen waves
    (10, 2, 256, 4): (),           # 4 bins
    (10, 2, 256, 16): (),          # 16 bins (eight waves: csrc/maf_forward_bf16.h)
    (128, 3, 512, 8): None,        # D = 128 / H = 512: eight panels, 33 hidden tiles, 99 KB of LDS for one row set; n = 33 only
}
# REPLACED SHAPE: the last one was to be nsf6 at this size, (128, 6, 512, 8).  There the float32 model itself has 15 % of
# these 33 rows beyond its own bound (17 - 19 % of 264 rows: six transforms x ~1700 rounded values per row, and a row
# flips when one of them lands within float32 noise of a bf16 boundary), above the 10 % the criterion allows the
# yardstick; with four transforms 6 % of 33 but 8 - 11 % of 264; with three 6 % / 5 - 6 %.  So the neighbour with three
# transforms stands in: the same widths, tiles, panels and LDS, half the depth (the kernel's loop over transforms is
# exercised by every shape).  tests/test_bf16_spline_model_cpu.py holds every shape here to the 10 %.


def shape_spec(D, T, H, K):
    from pocomc_amd.maf_spec import MAFSpec
    return MAFSpec(D, T, hidden=H, univariate="rqs", bins=K)


def default_params(spec, seed=3):
    return spec.init_params(seed).astype(np.float32)


def rows_for(D, n, seed=0, scale=1.2):
    return (np.random.default_rng(1000 * D + seed).normal(size=(n, D)) * scale).astype(np.float32)


def shape_counts(key):
    return (33,) if SHAPES[key] is None else ROWS + SHAPES[key]


# Trained and saturated flows (tests/flow_regimes.py) with rows at the spline's edges.  The trained twin is
# ``fr.twin_trained("nsf6")``, the spline twin that helper trains (it has no "nsf3"); the saturated flows are nsf3 at D = 10
# with the output layer scaled by 4 and by 16.
REGIMES = {"nsf6-d10-twin": None, "nsf3-d10-g4": 4.0, "nsf3-d10-g16": 16.0}


def regime(name):
    """(spec, parameters, two-mode rows) of a trained / saturated spline flow."""
    from pocomc_amd.maf_spec import MAFSpec
    if REGIMES[name] is None:
        spec, flat = fr.twin_trained("nsf6")
        return spec, flat, fr.two_modes(10, 1000, 9)
    spec = MAFSpec(10, 3, univariate="rqs")
    return spec, fr.gain_params(spec, REGIMES[name]), fr.two_modes(10, 1000, 9) * np.float32(1.3)


def edge_rows(spec, flat, data):
    """``(rows for the criterion, rows with EVERY coordinate outside the box)``.

    The criterion's rows, one set like ``tests/test_gpu_flow_regimes.py`` builds it: 96 of the flow's own rows, 48 rows with
    every coordinate on a knot of transform 0 (``fr.all_knot_rows``), the rows at +-5 and in the band up to the computed
    end knot (``fr.box_rows``), and those of ``fr.outside_rows`` that float32 can square (|x| < 1e18: at 1e20 the base
    density's z^2 overflows float32, for the kernel as for the float32 model; those rows are in the second set, which is
    held bit for bit instead: z = x, ladj = 0).  Measured on the CPU, float32 model alone, rows beyond its own bound: at
    most 6.9 % in a quantity with this set; the edge rows alone (59 knot and box rows) 0 / 0 / 8.5 % on the twin / x4 / x16
    -- one row from the 10 % cap -- and knot, box and outside rows without the flow's own rows 10.9 % on the twin."""
    base = np.ascontiguousarray(data[:64])
    out, mask = fr.outside_rows(spec, base, n_all=8)
    safe = np.abs(out).max(axis=1) < 1e18
    crit = np.concatenate([data[64:160], fr.all_knot_rows(spec, flat, base[:48])[0], fr.box_rows(spec, flat, base)[0], out[safe]])
    return np.ascontiguousarray(crit, np.float32), np.ascontiguousarray(out[mask.all(axis=1)], np.float32)
