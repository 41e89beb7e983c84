"""The spline instances of the bf16 matrix-core forward kernel (``csrc/maf_forward_bf16.h``, ``pmc_maf_forward_bf16`` with
``n_out`` = 11 / 23 / 47) against the float64 evaluation of a model that rounds where they round
(``tests/bf16_spline_model.py``), with the float32 evaluation of the same model -- the kernels' own spline formulas -- as
the yardstick, measured in the same test on the same rows.  ``tests/test_bf16_spline_model_cpu.py`` shows that the
criterion rejects six single defects and that the yardstick holds its own share on every shape and row set used here.

Per quantity (z, ladj, log_prob): ``b = max(8 x p75 of the float32 model's errors, 2^-20)``; the kernel's 75th percentile
is at most ``b``, at most 25 % of its rows lie beyond ``b``, at most 10 % of the float32 model's own rows do; every row
is finite; the distance from the plain float32 oracle is printed, not asserted (it measures bf16, not the kernel).  Bit
for bit: each output requested alone, a permuted copy of the batch, the ``idx`` gather, the first 17 rows of a two-row-set
call against a 17-row call, ``Flow.forward`` / ``Flow.log_prob`` against the raw entry, rows wholly outside the splines'
box (z = x, ladj = 0), and every finite row of a batch with non-finite rows in it.

The C entry has no width rule: the narrow shapes are reached by setting ``precision = "bf16"`` on a float32 ``Flow``.
Two departures from the shapes first planned, both explained in ``tests/bf16_spline_model.py``: the widest shape has three
transforms, not six (the YARDSTICK misses its 10 % at six), and the trained twin is ``fr.twin_trained("nsf6")``.

MEASURED on MI355X: see docs/LAB_NOTEBOOK.md ("bf16 spline forward").
"""
import ctypes as C
import functools
import pickle

import numpy as np
import pytest
import torch

import bf16_model as bm
import bf16_spline_model as sm
import flow_regimes as fr
from oracle.maf import OracleMAF
from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu


def bf16_flow(spec, flat):
    """A float32 ``Flow`` switched to the bf16 forward kernel behind the constructor's width rule."""
    from pocomc_amd import Flow
    f = Flow(spec.n_dim, spec, seed=0)
    f.precision = "bf16"
    f.set_params(flat)
    return f


def forward_call(f, xd, n, want=bm.FWD_QUANTITIES, idx=None, per_t=None):
    """``pmc_maf_forward_bf16`` on the first ``n`` rows of the device tensor ``xd`` (or the rows ``idx`` of it) with exactly
    the outputs ``want``; the others are passed as null.  ``per_t``: another image stride than the flow's (refused)."""
    from pocomc_amd import _lib
    _, img, own = f._bf16_image()
    per_t = own if per_t is None else per_t
    D = f.spec.n_dim
    out = {"z": torch.full((n, D), 7.0, dtype=torch.float32, device=xd.device) if "z" in want else None,
           "ladj": torch.full((n,), 7.0, dtype=torch.float32, device=xd.device) if "ladj" in want else None,
           "log_prob": torch.full((n,), 7.0, dtype=torch.float32, device=xd.device) if "log_prob" in want else None}
    with torch.cuda.device(xd.device):
        _lib.check(f.lib.pmc_maf_forward_bf16(C.byref(f._desc), _lib.ptr(img), per_t, _lib.ptr(xd), _lib.ptr(out["z"]),
                                              _lib.ptr(out["ladj"]), _lib.ptr(out["log_prob"]), n, _lib.ptr(idx),
                                              _lib.stream_handle()), "pmc_maf_forward_bf16")
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def prefix(d, n):
    return {k: v[:n] for k, v in d.items()}


def hold_forward(spec, flat, x, got, ref, f32, tag):
    """The criterion on the rows ``x`` (``ref`` / ``f32``: the float64 / float32 model on the same rows)."""
    with np.errstate(all="ignore"):
        o = OracleMAF(spec, flat)
        plain = {"z": o.forward(x)[0], "ladj": o.forward(x)[1], "log_prob": o.log_prob(x)}
    for q, v in sm.verdicts(got, ref, f32).items():
        far = float(bm.forward_row_err(q, got[q], {**ref, q: plain[q]}).max())
        print(f"{tag} {q}: kernel p75 {v['p75']:.2e} worst {v['worst']:.2e} beyond {v['flipped']:.1%} | float32 model p75 "
              f"{v['p75_f32']:.2e} worst {v['worst_f32']:.2e} beyond {v['flipped_f32']:.1%} | bound {v['bound']:.2e} | "
              f"from the plain float32 oracle {far:.2e}")
        assert np.isfinite(got[q]).all(), f"{tag} {q}: non-finite rows"
        assert v["flipped_f32"] <= bm.FWD_FLIP_SHARE_F32, f"{tag} {q}: the float32 model itself has {v['flipped_f32']:.1%} of its rows beyond the bound"
        assert v["p75"] <= v["bound"], f"{tag} {q}: 75th percentile {v['p75']:.3e} > {v['bound']:.3e}"
        assert v["flipped"] <= bm.FWD_FLIP_SHARE, f"{tag} {q}: {v['flipped']:.1%} of the rows beyond {v['bound']:.3e}"


@functools.lru_cache(maxsize=None)
def shape_case(key):
    """(spec, parameters, rows, float64 model, float32 model, flow) of a shape: computed once, shared, never written to."""
    spec = sm.shape_spec(*key)
    flat = sm.default_params(spec)
    x = sm.rows_for(key[0], max(sm.shape_counts(key) + (53,)))
    ref, f32 = sm.SplineBF16Model(spec, flat).forward(x), sm.SplineBF16Model(spec, flat, np.float32).forward(x)
    return spec, flat, x, ref, f32, bf16_flow(spec, flat)


@pytest.mark.parametrize("key", list(sm.SHAPES), ids=str)
def test_forward_against_the_rounding_exact_model(key):
    spec, flat, x, ref, f32, f = shape_case(key)
    xd = torch.from_numpy(x).cuda()
    for n in sm.shape_counts(key):
        tag = f"bf16 spline forward (D, T, H, K)={key} n={n}"
        got = forward_call(f, xd, n)
        hold_forward(spec, flat, x[:n], got, prefix(ref, n), prefix(f32, n), tag)
        for q in bm.FWD_QUANTITIES:                         # each output alone: the other two null
            alone = forward_call(f, xd, n, want=(q,))
            np.testing.assert_array_equal(alone[q], got[q], err_msg=f"{tag}: {q} requested alone")
    # the Flow's own entry points take the same path
    z, ladj = f.forward(torch.from_numpy(x[:33]))
    got = forward_call(f, xd, 33)
    np.testing.assert_array_equal(z.numpy(), got["z"])
    np.testing.assert_array_equal(ladj.numpy(), got["ladj"])
    np.testing.assert_array_equal(f.log_prob(torch.from_numpy(x[:33])).numpy(), got["log_prob"])
    # and it is not the float32 kernel's answer: the switch reached the bf16 kernel
    f.precision = "f32"
    try:
        z32, _ = f.forward(torch.from_numpy(x[:33]))
    finally:
        f.precision = "bf16"
    assert not np.array_equal(z32.numpy(), got["z"])


@pytest.mark.parametrize("key", [(17, 2, 64, 8), (40, 2, 256, 8), (10, 2, 256, 16)], ids=str)
def test_a_rows_outputs_do_not_depend_on_its_position(key):
    """Bit for bit: a permuted copy of the batch, and the same permutation through the ``idx`` gather argument."""
    spec, flat, x, ref, f32, f = shape_case(key)
    n = 53
    x = x[:n]
    perm = np.random.default_rng(4).permutation(n)
    xd = torch.from_numpy(x).cuda()
    base = forward_call(f, xd, n)
    copy = forward_call(f, torch.from_numpy(np.ascontiguousarray(x[perm])).cuda(), n)
    gathered = forward_call(f, xd, n, idx=torch.from_numpy(perm.astype(np.int64)).cuda())
    short = forward_call(f, xd, 20, idx=torch.from_numpy(perm[:20].astype(np.int64)).cuda())
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(copy[q], base[q][perm], err_msg=f"{q}: permuted copy")
        np.testing.assert_array_equal(gathered[q], base[q][perm], err_msg=f"{q}: idx gather")
        np.testing.assert_array_equal(short[q], base[q][perm[:20]], err_msg=f"{q}: idx gather of 20 rows")


def test_a_rows_outputs_do_not_depend_on_the_row_sets():
    """The first 17 rows of the 4113-row call (eight waves, two row sets) against a call of 17 rows (eight waves, one row
    set): a tile's k order does not depend on the row sets, a (rank, row) of row set 1 is evaluated by the thread 256
    places behind the one that evaluates it in row set 0 -- four waves on, the same lane -- so the log-determinant's
    per-wave partial sums are the same numbers in other slots, with zeros between them."""
    key = (7, 2, 32, 8)
    spec, flat, x, ref, f32, f = shape_case(key)
    n_big = 4113
    xd = torch.from_numpy(x).cuda()
    big, small = forward_call(f, xd, n_big), forward_call(f, xd, 17)
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(big[q][:17], small[q], err_msg=q)
    tail0 = (n_big // 32) * 32                               # the last workgroup: its second row set holds one row
    tail = forward_call(f, xd[tail0:].contiguous(), n_big - tail0)
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(big[q][tail0:], tail[q], err_msg=f"{q}: tail")


# ---------------------------------------------------------------------------------------------------------- regimes
@functools.lru_cache(maxsize=None)
def regime_case(name):
    spec, flat, data = sm.regime(name)
    return spec, flat, data, bf16_flow(spec, flat)


@pytest.mark.parametrize("name", list(sm.REGIMES))
def test_forward_at_the_splines_edges_on_trained_and_saturated_flows(name):
    spec, flat, data, f = regime_case(name)
    x, allout = sm.edge_rows(spec, flat, data)
    ref, f32 = sm.SplineBF16Model(spec, flat).forward(x), sm.SplineBF16Model(spec, flat, np.float32).forward(x)
    got = forward_call(f, torch.from_numpy(x).cuda(), len(x))
    hold_forward(spec, flat, x, got, ref, f32, f"bf16 spline forward {name}, edge rows")
    # rows with every coordinate outside the box: every spline of every transform is the identity
    assert len(allout) >= 4
    out = forward_call(f, torch.from_numpy(allout).cuda(), len(allout))
    np.testing.assert_array_equal(out["z"], allout)
    assert np.all(out["ladj"] == 0.0)


@pytest.mark.parametrize("name", list(sm.REGIMES))
@pytest.mark.parametrize("n", [64, 4096])
def test_non_finite_rows_stay_in_their_rows(name, n):
    """NaN / +inf / -inf in one coordinate of rows 0, 15, 16, 17 and n - 1: every other row is bit-identical to the same
    batch with those rows finite (one and two row sets per workgroup)."""
    spec, flat, data, f = regime_case(name)
    good = np.ascontiguousarray(data[np.random.default_rng(n).choice(len(data), n, replace=n > len(data))])
    bad, rows = fr.with_nonfinite(good)
    keep = np.setdiff1d(np.arange(n), rows)
    a = forward_call(f, torch.from_numpy(good).cuda(), n)
    b = forward_call(f, torch.from_numpy(bad).cuda(), n)
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(b[q][keep], a[q][keep], err_msg=f"{name} n={n} {q}")
        assert np.isfinite(a[q]).all()
    assert not np.isfinite(b["z"][rows]).all(axis=1).any()           # (the bad rows do come out non-finite)


# ---------------------------------------------------------------------------------------------------- Flow, Sampler
def image_of(f):
    idx, img, _ = f._bf16_image()
    return idx.cpu().numpy(), img.cpu().numpy().view(np.uint16)


def assert_image_in_step(f):
    idx, img = image_of(f)
    flat = f.params.detach().cpu().numpy()
    np.testing.assert_array_equal(img, np.where(idx >= 0, bm.bf16_bits(flat[np.maximum(idx, 0)]), 0).astype(np.uint16))


def test_the_entry_refuses_other_output_counts():
    from pocomc_amd import _lib
    spec = sm.shape_spec(7, 2, 32, 8)
    f = bf16_flow(spec, sm.default_params(spec))
    xd = torch.zeros(16, 7, device="cuda")
    f._desc.n_out = 5
    try:
        with pytest.raises(_lib.PocomcAmdError, match="n_out must be 2"):
            forward_call(f, xd, 16)
    finally:
        f._desc.n_out = spec.n_out
    # ... and an image that is not laid out as the kernel's fragment pointers assume
    with pytest.raises(_lib.PocomcAmdError, match="bf16 layout"):
        forward_call(f, xd, 16, per_t=spec.bf16_layout()["per_transform"] - 512)
    assert np.isfinite(forward_call(f, xd, 16)["log_prob"]).all()


def test_flow_with_precision_bf16_on_a_wide_spline_flow():
    from pocomc_amd import Flow
    spec = MAFSpec(10, 3, hidden=256, univariate="rqs")
    f = Flow(10, spec, precision="bf16", seed=1)
    assert f.precision == "bf16"
    with pytest.raises(NotImplementedError, match="256"):
        Flow(10, MAFSpec(10, 3, hidden=128, univariate="rqs"), precision="bf16")
    with pytest.raises(NotImplementedError):
        Flow(10, spec, precision="bf16", inverse_precision="bf16")
    x = torch.from_numpy(sm.rows_for(10, 200, seed=3))
    z, ladj = f.forward(x)
    lp = f.log_prob(x)
    raw = forward_call(f, x.cuda(), 200)
    np.testing.assert_array_equal(z.numpy(), raw["z"])
    np.testing.assert_array_equal(lp.numpy(), raw["log_prob"])
    assert_image_in_step(f)
    # pickle: the same flow, the same outputs
    g = pickle.loads(pickle.dumps(f))
    assert g.precision == "bf16" and g.spec.univariate == "rqs" and g.spec.hidden == 256
    z2, ladj2 = g.forward(x)
    np.testing.assert_array_equal(z2.numpy(), z.numpy())
    np.testing.assert_array_equal(ladj2.numpy(), ladj.numpy())
    np.testing.assert_array_equal(g.log_prob(x).numpy(), lp.numpy())
    # set_params: the image follows
    flat = sm.default_params(spec, 9)
    f.set_params(flat)
    assert_image_in_step(f)
    ref = sm.SplineBF16Model(spec, flat).forward(x.numpy())
    assert np.abs(f.forward(x)[0].numpy() - ref["z"]).max() < 1e-3 * np.abs(ref["z"]).max()
    # train_engine="bf16" on a spline flow still raises when the engine is asked for
    f.train_engine = "bf16"
    with pytest.raises(ValueError, match="affine"):
        f.fit(x, epochs=1)
    f.train_engine = None
    # a 5-epoch fit (float32 kernels) moves the parameters; the image follows
    before = f.params.clone()
    f.fit(fr.two_modes(10, 512, 1), epochs=5, batch_size=256)
    assert not torch.equal(before, f.params)
    assert_image_in_step(f)
    lp = f.log_prob(x)
    assert torch.isfinite(lp).all()
    np.testing.assert_array_equal(lp.numpy(), forward_call(f, x.cuda(), 200)["log_prob"])


def test_sampler_runs_to_beta_one_on_a_bf16_spline_flow():
    import pocomc_amd as pc
    from scipy.stats import uniform
    D = 4
    prior = pc.Prior([uniform(-5, 10)] * D)

    def loglike(x):
        return np.sum(-0.5 * ((x - 0.7) / 0.5) ** 2, axis=1)
    flow = pc.Flow(D, MAFSpec(D, 3, hidden=256, univariate="rqs"), precision="bf16", seed=2)
    s = pc.Sampler(prior=prior, likelihood=loglike, vectorize=True, flow=flow, random_state=5, n_effective=128,
                   n_active=64, train_config=dict(epochs=20))
    s.run(progress=False)
    assert s.flow is flow and s.flow.precision == "bf16" and s.flow._bf16 is not None      # (the run went through the bf16 forward)
    logz, beta = s.evidence()[0], float(s.particles.get("beta", index=-1))
    print(f"bf16 spline flow in a Sampler: beta {beta}, logZ {logz:.3f} (analytic {D * np.log(0.5 * np.sqrt(2 * np.pi)) - D * np.log(10.0):.3f})")
    assert beta == 1.0 and np.isfinite(logz)
    assert_image_in_step(s.flow)
