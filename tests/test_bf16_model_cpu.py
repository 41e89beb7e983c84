"""The rounding-exact model of the bf16 kernels (``tests/bf16_model.py``) checked on the CPU, without the kernels:

* with rounding switched off it IS the flow: float64 autograd of ``oracle.maf.torch_loss`` and ``OracleMAF(float64)``
  to 1e-12 (measured <= 5e-16);
* its ``rne`` is torch's float32 -> bfloat16 conversion bit for bit, on the edges of the conversion and 1e5 random bit
  patterns;
* the criterion the GPU tests hold the kernels to (``forward_verdict``, ``TrainReference.verdict``) tells a correct
  float32 evaluation of the model from one with a single defect, at every shape tried.

Measured here at the three shapes (float32 model against the float64 model).  Trainer, relative L2 of the gradient: the
largest of the four clean orders 1.8e-8 / 5.1e-6 / 7.1e-8, ``da0`` left unrounded (the mildest defect) 1.6e-4 / 3.7e-4 /
5.1e-4.  Forward, 75th percentile of z: bound 9.5e-7 / 1.2e-6 / 1.0e-6, layer-2 activations left unrounded (the
mildest) 8.7e-4 / 1.2e-3 / 6.8e-4."""
import numpy as np
import pytest
import torch

import bf16_model as bm
import cases
from oracle.maf import OracleMAF, torch_loss
from pocomc_amd.maf_spec import MAFSpec

# (D, T, hidden, rows, weighted): tri_ok False (D = 2), an odd tile count, a 64-wide flow with five tiles
SHAPES = [(2, 2, None, 40, True), (5, 3, 32, 33, False), (16, 2, 64, 100, True)]


def batch(D, T, H, n, weighted, seed=2):
    spec = MAFSpec(D, T, hidden=H)
    flat = cases.flow_params(spec, seed, gain=1.0)
    rng = np.random.default_rng(D + n)
    x = (rng.normal(size=(n, D)) * 1.2).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    return spec, flat, x, w


@pytest.mark.parametrize("D,T,H,n,weighted", SHAPES + [(7, 2, None, 17, False), (33, 2, 128, 70, True), (50, 6, 256, 24, False)])
def test_without_rounding_the_model_is_float64_autograd(D, T, H, n, weighted):
    spec, flat, x, w = batch(D, T, H, n, weighted)
    m = bm.BF16Model(spec, flat, rounding=False)
    loss, g = m.loss_and_grad(x, w)
    ft = torch.tensor(flat.astype(np.float64), requires_grad=True)
    lo = torch_loss(spec, ft, torch.from_numpy(x).double(), None if w is None else torch.from_numpy(w).double())
    lo.backward()
    l_ref, g_ref = float(lo.detach()), ft.grad.numpy()
    el = abs(loss - l_ref) / abs(l_ref)
    eg = np.linalg.norm(g - g_ref) / np.linalg.norm(g_ref)
    print(f"unrounded model vs float64 autograd D={D} T={T} H={spec.hidden} n={n}: loss {el:.1e}, gradient L2 {eg:.1e}")
    assert el <= 1e-12 and eg <= 1e-12
    assert np.all(g[spec.mask_flat() == 0] == 0.0)
    o = OracleMAF(spec, flat, dtype=np.float64)
    z, ladj = o.forward(x.astype(np.float64))
    f = m.forward(x)
    scale = max(1.0, float(np.abs(z).max()))
    assert np.abs(f["z"] - z).max() <= 1e-12 * scale
    assert np.abs(f["ladj"] - ladj).max() <= 1e-12 * max(1.0, float(f["terms"].max()))
    lp = o.log_prob(x.astype(np.float64))
    assert np.abs(f["log_prob"] - lp).max() <= 1e-12 * max(1.0, float(np.abs(lp).max()))
    np.testing.assert_allclose(f["terms"], o.ladj_abs_terms(x.astype(np.float64)), rtol=1e-12)


def test_rne_is_torchs_bfloat16_conversion_bit_for_bit():
    v, nan = bm.crafted_vector()
    assert nan.sum() >= 6 and (~nan).sum() >= 100_000
    got = bm.bf16_bits(v)
    want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(got[~nan], want[~nan])
    back = bm.rne(v)
    assert np.isnan(back[nan]).all() and not np.isnan(back[~nan]).any()
    assert ((got[nan] & 0x0040) != 0).all()                                   # the quiet bit
    np.testing.assert_array_equal(got[nan] & 0x8000, (v[nan].view(np.uint32) >> 16) & 0x8000)   # and the sign stays
    # the named edges, spelled out: ties go to the even mantissa, the largest finites round to inf, -0 stays -0
    edge = np.array([0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x7f7f8000, 0x7f7fffff, 0x80000000, 0x00000001],
                    np.uint32).view(np.float32)
    np.testing.assert_array_equal(bm.bf16_bits(edge), np.array([0x3f80, 0x3f82, 0x3f80, 0x3f81, 0x7f80, 0x7f80, 0x8000, 0x0000], np.uint16))
    np.testing.assert_array_equal(bm.bf16_bits(edge, truncate=True), (edge.view(np.uint32) >> 16).astype(np.uint16))


@pytest.mark.parametrize("D,T,H,n,weighted", SHAPES)
def test_the_criterion_tells_every_defect_from_a_clean_float32_evaluation(D, T, H, n, weighted):
    spec, flat, x, w = batch(D, T, H, n, weighted)
    ref = bm.BF16Model(spec, flat).forward(x)
    clean = bm.BF16Model(spec, flat, np.float32).forward(x)
    e32 = {q: bm.forward_row_err(q, clean[q], ref) for q in bm.FWD_QUANTITIES}
    for order in bm.ORDERS[1:]:                             # a clean evaluation in another order meets it too
        other = bm.BF16Model(spec, flat, np.float32, order).forward(x)
        for q in bm.FWD_QUANTITIES:
            v = bm.forward_verdict(bm.forward_row_err(q, other[q], ref), e32[q])
            assert v["ok"], (order, q, v)
    for q in bm.FWD_QUANTITIES:
        assert bm.forward_verdict(e32[q], e32[q])["ok"]
    for d in bm.FORWARD_DEFECTS:
        got = bm.BF16Model(spec, flat, np.float32, defect=d).forward(x)
        for q in bm.FWD_QUANTITIES:
            v = bm.forward_verdict(bm.forward_row_err(q, got[q], ref), e32[q])
            print(f"forward D={D} T={T} {d} {q}: p75 {v['p75']:.2e} (bound {v['bound']:.2e}), beyond {v['flipped']:.0%}")
            assert not v["ok"], (d, q, v)
    R = bm.TrainReference(spec, flat, x, w)
    for order in bm.ORDERS:
        l32, g32 = bm.BF16Model(spec, flat, np.float32, order).loss_and_grad(x, w)
        v = R.verdict(l32, g32)
        assert v["ok"], (order, v["failing"], v["summary"])
    print(f"trainer D={D} T={T} clean float32: {v['summary']}")
    for d in bm.DEFECTS:
        l32, g32 = bm.BF16Model(spec, flat, np.float32, defect=d).loss_and_grad(x, w)
        v = R.verdict(l32, g32)
        print(f"trainer D={D} T={T} {d}: {v['summary']}; {len(v['failing'])} measures beyond {bm.TRAIN_C:g} x the yardstick")
        assert not v["ok"] and "grad" in v["failing"], (d, v["summary"])
        assert v["measures"]["grad"] >= 10.0 * R.yard["grad"], (d, v["summary"])     # (the margin behind TRAIN_C)
    # a masked entry that is written fails whatever its size
    l32, g32 = bm.BF16Model(spec, flat, np.float32).loss_and_grad(x, w)
    assert np.all(g32[spec.mask_flat() == 0] == 0.0)
