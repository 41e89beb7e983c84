"""The rounding-exact model of the bf16 forward kernel's spline instances (``tests/bf16_spline_model.py``) and the bf16
fragment image of the spline flows, checked on the CPU without the kernels:

(a) with rounding switched off the model IS the flow: ``OracleMAF(float64)`` to 1e-12 (measured <= 7e-14);
(b) ``MAFSpec.pack_index_bf16`` of spline specs decodes, slot by slot, to the (layer, row, column) the kernel's fragment
    addressing implies -- written down here from the kernel's side, with the oracle's masks -- and every masked or padded
    slot is -1; the image is ``bf16_bits`` of the masked canonical weights bit for bit;
(c) on every shape and row set ``tests/test_gpu_bf16_spline.py`` runs, the float32 model alone stays within the 10 % of
    rows the criterion allows the yardstick, with a finite 75th percentile in every quantity;
(d) the criterion rejects each of six single defects on every listed shape, by the kernel-side terms alone (75th
    percentile beyond the bound, or more than 25 % of the rows beyond it) -- and accepts a clean float32 evaluation in
    another contraction order;
(e) the width rule of ``Flow(..., precision="bf16")``."""
import functools

import numpy as np
import pytest

import bf16_model as bm
import bf16_spline_model as sm
from oracle.maf import OracleMAF, zuko_masks
from pocomc_amd.maf_spec import MAFSpec, WIDE_MIN_HIDDEN, bf16_forward_refusal, spec_by_name


# --------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("D,T,H,K", [(2, 2, 32, 8), (7, 2, 32, 8), (17, 2, 64, 8), (10, 2, 256, 4), (10, 2, 256, 16), (33, 3, 128, 8)])
def test_without_rounding_the_model_is_the_float64_oracle(D, T, H, K):
    spec = sm.shape_spec(D, T, H, K)
    flat = sm.default_params(spec)
    x = sm.rows_for(D, 40)
    f = sm.SplineBF16Model(spec, flat, rounding=False).forward(x)
    o = OracleMAF(spec, flat, dtype=np.float64)
    z, ladj = o.forward(x.astype(np.float64))
    lp = o.log_prob(x.astype(np.float64))
    ez = np.abs(f["z"] - z).max() / max(1.0, float(np.abs(z).max()))
    el = np.abs(f["ladj"] - ladj).max() / max(1.0, float(f["terms"].max()))
    ep = np.abs(f["log_prob"] - lp).max() / max(1.0, float(np.abs(lp).max()))
    print(f"unrounded spline model vs float64 oracle D={D} T={T} H={H} K={K}: z {ez:.1e}, ladj {el:.1e}, log_prob {ep:.1e}")
    assert ez <= 1e-12 and el <= 1e-12 and ep <= 1e-12
    np.testing.assert_allclose(f["terms"], o.ladj_abs_terms(x.astype(np.float64)), rtol=1e-12)
    # and the rounded model differs: the switch does something
    r = sm.SplineBF16Model(spec, flat).forward(x)
    assert np.abs(r["z"] - z).max() > 1e-6


# --------------------------------------------------------------------------------------------------------------- (b)
def decoded_image(spec, flat):
    """``(expected gather index, expected bf16 image)`` of the bf16 fragment image, from the kernel's side: transform t,
    block g0 / g1 / g2 / g3, record ``[out tile][k tile][lane][e]`` holds ``W[out row 16 tile + (lane & 15)][k = 32 ktile +
    8 (lane >> 4) + e]`` (``csrc/bf16.h``: the A operand of v_mfma_f32_16x16x32_bf16) with hidden units addressed by slot
    (``slot_unit``), features by rank, and W3's rows as ``n_out * rank + j``; masks: ``oracle.maf.zuko_masks``."""
    D, H, Hp, Dp, NO = spec.n_dim, spec.hidden, spec.Hp, spec.Dp, spec.n_out
    nT, nOT = Hp // 16, NO * Dp // 16
    nX2, nK2 = -(-Dp // 32), -(-Hp // 32)
    su = np.asarray(spec.slot_unit)
    lane, e = np.arange(64)[:, None], np.arange(8)[None, :]
    row_in_tile, k_in_tile = lane & 15, 8 * (lane >> 4) + e                     # (64, 8)
    idx, img = [], []
    for t in range(spec.n_transforms):
        order = np.arange(D) if t % 2 == 0 else np.arange(D)[::-1]              # rank of every feature
        feat_of_rank = np.argsort(order)
        M = zuko_masks(order, NO, H)
        base = t * spec.params_per_transform
        for layer, n_out_tiles, n_k_tiles in ((0, nT, nX2), (1, nT, nK2), (2, nT, nK2), (3, nOT, nK2)):
            name = f"W{layer}"
            off, _ = spec.offsets[name]
            ncol = spec.shapes()[name][1]
            W = spec.view(flat, t, name)
            for To in range(n_out_tiles):
                orow = 16 * To + row_in_tile + 0 * e
                if layer < 3:
                    crow = su[orow]                                             # hidden unit of the out slot, -1 = padding
                else:
                    rank, j = orow // NO, orow % NO
                    crow = np.where(rank < D, NO * feat_of_rank[np.minimum(rank, D - 1)] + j, -1)
                for Tk in range(n_k_tiles):
                    k = 32 * Tk + k_in_tile + 0 * lane
                    if layer == 0:
                        ccol = np.where(k < D, feat_of_rank[np.minimum(k, D - 1)], -1)
                    else:
                        ccol = np.where(k < Hp, su[np.minimum(k, Hp - 1)], -1)
                    ok = (crow >= 0) & (ccol >= 0)
                    r, c = np.where(ok, crow, 0), np.where(ok, ccol, 0)
                    ok &= M[layer][r, c]
                    idx.append(np.where(ok, base + off + r * ncol + c, -1).reshape(-1))
                    img.append(np.where(ok, bm.bf16_bits((W * M[layer]).astype(np.float32))[r, c], 0).reshape(-1))
    return np.concatenate(idx).astype(np.int32), np.concatenate(img).astype(np.uint16)


# K = 4, 8, 16; D not a multiple of 16 (2, 7, 17, 33, 10); odd tile counts (7: three hidden tiles, 10 / 256: seventeen)
@pytest.mark.parametrize("D,T,H,K", [(2, 2, 32, 8), (7, 2, 32, 8), (17, 2, 64, 8), (33, 2, 128, 8), (10, 2, 256, 4), (10, 2, 256, 16), (16, 3, 64, 4)])
def test_the_bf16_image_of_a_spline_flow_decodes_to_layer_row_and_column(D, T, H, K):
    spec = sm.shape_spec(D, T, H, K)
    flat = sm.default_params(spec, 5)
    want_idx, want_img = decoded_image(spec, flat)
    idx = spec.pack_index_bf16()
    L = spec.bf16_layout()
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape == (L["per_transform"] * T,)
    np.testing.assert_array_equal(idx, want_idx)                               # every masked or padded slot: -1, the rest: its weight
    img = np.where(idx >= 0, bm.bf16_bits(flat[np.maximum(idx, 0)]), 0).astype(np.uint16)      # pmc_maf_pack_bf16
    np.testing.assert_array_equal(img, want_img)
    # every unmasked weight of every layer is in the image at least once, and nothing else is
    used = np.zeros(spec.n_params, bool)
    used[idx[idx >= 0]] = True
    mask = spec.mask_flat() > 0
    weights = np.zeros(spec.n_params, bool)
    for t in range(T):
        for name in ("W0", "W1", "W2", "W3"):
            off, sz = spec.offsets[name]
            weights[t * spec.params_per_transform + off: t * spec.params_per_transform + off + sz] = True
    np.testing.assert_array_equal(used, mask & weights)
    if D == 7:
        assert spec.nT % 2 == 1
    if K == 8 and D in (2, 7):
        assert spec.tri_ok == (D != 2)


# --------------------------------------------------------------------------------------------------------------- (c)
@functools.lru_cache(maxsize=None)
def shape_models(key):
    spec = sm.shape_spec(*key)
    flat = sm.default_params(spec)
    x = sm.rows_for(key[0], max(sm.shape_counts(key)))
    return spec, flat, x, sm.SplineBF16Model(spec, flat).forward(x), sm.SplineBF16Model(spec, flat, np.float32).forward(x)


def prefix(d, n):
    return {k: v[:n] for k, v in d.items()}


def hold_the_yardstick(ref, f32, tag):
    for q, v in sm.verdicts(f32, ref, f32).items():
        print(f"{tag} {q}: float32 model p75 {v['p75_f32']:.2e} worst {v['worst_f32']:.2e} beyond {v['flipped_f32']:.1%} | bound {v['bound']:.2e}")
        assert np.isfinite(v["p75_f32"]), f"{tag} {q}: the yardstick's 75th percentile is not finite"
        assert v["flipped_f32"] <= bm.FWD_FLIP_SHARE_F32, f"{tag} {q}: {v['flipped_f32']:.1%} of the float32 model's rows beyond {v['bound']:.3e}"


@pytest.mark.parametrize("key", list(sm.SHAPES), ids=str)
def test_the_float32_model_holds_its_share_on_every_shape_of_the_gpu_test(key):
    spec, flat, x, ref, f32 = shape_models(key)
    for n in sm.shape_counts(key):
        hold_the_yardstick(prefix(ref, n), prefix(f32, n), f"spline model {key} n={n}")


@pytest.mark.parametrize("name", list(sm.REGIMES))
def test_the_float32_model_holds_its_share_on_the_edge_rows(name):
    spec, flat, data = sm.regime(name)
    x, allout = sm.edge_rows(spec, flat, data)
    assert len(allout) >= 4
    hold_the_yardstick(sm.SplineBF16Model(spec, flat).forward(x), sm.SplineBF16Model(spec, flat, np.float32).forward(x),
                       f"spline model {name} edge rows")
    # the model maps rows beyond the box to themselves, with no log-determinant
    for dtype in (np.float64, np.float32):
        r = sm.SplineBF16Model(spec, flat, dtype).forward(allout)
        np.testing.assert_array_equal(r["z"], allout.astype(dtype))
        assert np.all(r["ladj"] == 0.0)


# --------------------------------------------------------------------------------------------------------------- (d)
DEFECT_SHAPES = [(7, 2, 32, 8), (17, 2, 64, 8), (10, 2, 256, 4), (10, 2, 256, 16)]


def rejected(v):
    """Rejected by what the kernel contributes to the verdict (not by the yardstick's own share)."""
    return v["p75"] > v["bound"] or v["flipped"] > bm.FWD_FLIP_SHARE


@pytest.mark.parametrize("key", DEFECT_SHAPES, ids=str)
def test_the_criterion_tells_every_defect_from_a_clean_float32_evaluation(key):
    spec, flat, x, ref, f32 = shape_models(key)
    n = 33
    x, ref, f32 = x[:n], prefix(ref, n), prefix(f32, n)
    for order in bm.ORDERS[1:]:                              # a clean evaluation in another order meets the criterion
        other = sm.SplineBF16Model(spec, flat, np.float32, order).forward(x)
        for q, v in sm.verdicts(other, ref, f32).items():
            assert v["ok"], (order, q, v)
    for q, v in sm.verdicts(f32, ref, f32).items():
        assert v["ok"], (q, v)
    for d in sm.DEFECTS:
        got = sm.SplineBF16Model(spec, flat, np.float32, defect=d).forward(x)
        vs = sm.verdicts(got, ref, f32)
        for q, v in vs.items():
            print(f"spline forward {key} {d} {q}: p75 {v['p75']:.2e} (bound {v['bound']:.2e}), beyond {v['flipped']:.0%}")
        assert all(rejected(v) for v in vs.values()), (d, {q: (v["p75"], v["bound"], v["flipped"]) for q, v in vs.items()})


# --------------------------------------------------------------------------------------------------------------- (e)
def test_the_width_rule_of_precision_bf16():
    assert WIDE_MIN_HIDDEN == 256
    # affine flows: every width
    for spec in (MAFSpec(4, 3), MAFSpec(10, 3, hidden=32), MAFSpec(128, 8, hidden=512)):
        assert bf16_forward_refusal(spec) is None
    # spline flows: from 256 hidden units on, whatever the bins
    for K in (4, 8, 16):
        assert bf16_forward_refusal(MAFSpec(10, 3, hidden=256, univariate="rqs", bins=K)) is None
        assert bf16_forward_refusal(MAFSpec(10, 3, hidden=255, univariate="rqs", bins=K)) is not None
    assert bf16_forward_refusal(MAFSpec(128, 6, hidden=512, univariate="rqs")) is None
    assert bf16_forward_refusal(spec_by_name(128, "nsf6")) is None               # default width 512
    assert bf16_forward_refusal(spec_by_name(64, "nsf6")) is None                # 256
    for D in (4, 10, 42):                                                        # default widths 32, 32, 128
        why = bf16_forward_refusal(spec_by_name(D, "nsf3"))
        assert why is not None and "256" in why and str(spec_by_name(D, "nsf3").hidden) in why
