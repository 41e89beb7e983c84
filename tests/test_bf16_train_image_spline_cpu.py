"""``MAFSpec.wide_layout`` / ``wide_index`` (the row-major bf16 image of ``csrc/maf_train_bf16.hip`` and the scatter map of
its weight gradients) for SPLINE specs: ``OK = n_out DK``, W3 rows and ``b3`` in the canonical order ``n_out feature + s``
(widths, heights, derivatives).  Affine specs keep the arrays they had: their hashes are pinned."""
import hashlib

import numpy as np
import pytest

from oracle.maf import OracleMAF
from pocomc_amd.maf_spec import MAFSpec

SPECS = [(10, 3, 256, 8), (5, 2, 32, 4), (16, 2, 64, 16)]


def _parts(spec, img, bias, t):
    L = spec.wide_layout()
    DK, HK, OK = L["DK"], L["HK"], L["OK"]
    o = t * L["per_transform"]
    out = {}
    for name, (r, c) in (("W0f", (HK, DK)), ("W0b", (DK, HK)), ("W1f", (HK, HK)), ("W1b", (HK, HK)), ("W2f", (HK, HK)),
                         ("W2b", (HK, HK)), ("W3f", (OK, HK)), ("W3b", (HK, OK))):
        out[name] = img[o:o + r * c].reshape(r, c)
        o += r * c
    assert o == (t + 1) * L["per_transform"]
    ob = t * L["bias_per_transform"]
    for k, name in enumerate(("b0", "b1", "b2")):
        out[name] = bias[ob + k * HK: ob + (k + 1) * HK]
    out["b3"] = bias[ob + 3 * HK: ob + 3 * HK + OK]
    assert ob + 3 * HK + OK == (t + 1) * L["bias_per_transform"]
    return out


@pytest.mark.parametrize("D,T,H,K", SPECS)
def test_spline_training_image_holds_every_canonical_parameter(D, T, H, K):
    spec = MAFSpec(D, T, hidden=H, univariate="rqs", bins=K)
    NO = 3 * K - 1
    L = spec.wide_layout()
    DK, HK, OK = L["DK"], L["HK"], L["OK"]
    assert DK == -(-D // 32) * 32 and HK == -(-spec.Hp // 32) * 32 and OK == NO * DK
    assert L["per_transform"] == 2 * (HK * DK + 2 * HK * HK + OK * HK) and L["bias_per_transform"] == 3 * HK + OK
    img, bias = spec.wide_index()
    assert img.dtype == np.int32 and bias.dtype == np.int32
    assert img.size == T * L["per_transform"] and bias.size == T * L["bias_per_transform"]
    # every unmasked weight once in W and once in W^T, every bias once, masked entries nowhere
    m = spec.mask_flat()
    is_bias = np.zeros(spec.n_params, dtype=bool)
    for t in range(T):
        for k in ("b0", "b1", "b2", "b3"):
            o, sz = spec.offsets[k]
            is_bias[t * spec.params_per_transform + o: t * spec.params_per_transform + o + sz] = True
    cnt = np.bincount(img[img >= 0], minlength=spec.n_params)
    cb = np.bincount(bias[bias >= 0], minlength=spec.n_params)
    assert np.all(cnt[(m > 0) & ~is_bias] == 2) and np.all(cnt[(m == 0) | is_bias] == 0)
    assert np.all(cb[is_bias] == 1) and np.all(cb[~is_bias] == 0)
    # element by element: the canonical parameter, or -1 where masked or padded
    su = np.full(HK, -1)
    su[:spec.Hp] = spec.slot_unit
    for t in range(T):
        p = _parts(spec, img, bias, t)
        base = t * spec.params_per_transform
        masks = dict(zip(("W0", "W1", "W2", "W3"), spec.masks(t)))
        rows = {"W0": su, "W1": su, "W2": su,                                             # canonical row of every image row
                "W3": np.array([r if r // NO < D else -1 for r in range(OK)])}
        cols = {"W0": np.array([f if f < D else -1 for f in range(DK)]), "W1": su, "W2": su, "W3": su}
        for name in ("W0", "W1", "W2", "W3"):
            off, _ = spec.offsets[name]
            ncol = spec.shapes()[name][1]
            want = np.full((len(rows[name]), len(cols[name])), -1, dtype=np.int64)
            for i, r in enumerate(rows[name]):
                if r < 0:
                    continue
                ok = (cols[name] >= 0)
                c = np.where(ok, cols[name], 0)
                ok &= masks[name][r, c]
                want[i] = np.where(ok, base + off + r * ncol + c, -1)
            assert np.array_equal(p[name + "f"], want), (t, name)
            assert np.array_equal(p[name + "b"], want.T), (t, name)
        for name in ("b0", "b1", "b2"):
            off, _ = spec.offsets[name]
            assert np.array_equal(p[name], np.where(su >= 0, base + off + su, -1))
        off, _ = spec.offsets["b3"]
        assert np.array_equal(p["b3"], np.where(rows["W3"] >= 0, base + off + rows["W3"], -1))
    # the hyper-network through the image gives the oracle's phi in its order: (feature, [widths | heights | derivatives])
    flat = spec.init_params(1)
    vals = np.where(img >= 0, flat[np.maximum(img, 0)], 0.0).astype(np.float64)
    bv = np.where(bias >= 0, flat[np.maximum(bias, 0)], 0.0).astype(np.float64)
    x = np.random.default_rng(0).normal(size=(3, D))
    om = OracleMAF(spec, flat, dtype=np.float64)
    for t in range(T):
        p = _parts(spec, vals, bv, t)
        xp = np.zeros((3, DK))
        xp[:, :D] = x
        h = np.maximum(xp @ p["W0f"].T + p["b0"], 0.0)
        h = np.maximum(h + h @ p["W1f"].T + p["b1"], 0.0)
        h = np.maximum(h + h @ p["W2f"].T + p["b2"], 0.0)
        phi = (h @ p["W3f"].T + p["b3"])[:, :NO * D].reshape(3, D, NO)
        np.testing.assert_allclose(phi, om._phi(t, x), rtol=1e-11, atol=1e-12)


# sha256 of image_idx bytes + bias_idx bytes, computed on the commit before the image became general in n_out
AFFINE_HASHES = {
    (10, 3, 256): "a9ef85f8711d3662f52a758725194964fb94ef96390a072ff67b617b103f6899",
    (5, 2, 32): "ca2eb3b63ceee68a50817d80cde1deab08154985bee138964926710c9e688f6f",
    (16, 2, 64): "9454601afa7de34cf6654de02ab38671b0c2482dbeb2544ac337e4b7e1641aa0",
    (128, 8, 512): "d9bbd8f5cc008f5a8007d6f266b2804102d6ff7491b59e810de3401d2f046e38",
}


@pytest.mark.parametrize("D,T,H", sorted(AFFINE_HASHES))
def test_affine_training_image_is_byte_identical(D, T, H):
    spec = MAFSpec(D, T, hidden=H)
    img, bias = spec.wide_index()
    assert spec.wide_layout()["OK"] == 2 * spec.wide_layout()["DK"]
    assert hashlib.sha256(img.tobytes() + bias.tobytes()).hexdigest() == AFFINE_HASHES[(D, T, H)]
