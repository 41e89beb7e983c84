"""bf16 matrix-core training of the spline flows (``csrc/maf_train_bf16.hip``, ``train_engine="bf16_spline"``) against a
torch-autograd model that rounds where the engine rounds (``tests/bf16_spline_train_model.py``; the CPU side of the
argument is ``tests/test_bf16_spline_train_model_cpu.py``).

Criterion, per case: ``|g - g_T64| <= 0.25 d_round`` overall and ``<= 0.5`` for every parameter tensor against its own
``d_round = |g_T64 - g_64|`` (what bf16 costs on the same rows), the loss within 5e-5 of the model's, masked entries exactly 0;
the float32 evaluation of the model (the yardstick) holds 0.10 / 0.25 on the same rows.  What the float32 ENGINE's
hardware reciprocal / exp / log cost is printed per case as ``|g_f32 engine - g_64| / d_round``: a case where that share is
above 0.10 would be unfit for the 0.25, not the kernel.

The narrow shapes are reached as in ``test_gpu_bf16_spline.py``: ``precision`` and ``train_engine`` set as attributes on a
float32 ``Flow`` (the engine itself has no width rule).

MEASURED on MI355X: see docs/LAB_NOTEBOOK.md ("bf16 spline trainer").
"""
import os
import pickle
import socket

import numpy as np
import pytest
import torch

import bf16_spline_train_model as tm
from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu


def spline_flow(spec, flat, engine="bf16_spline"):
    """A float32 ``Flow`` switched to the bf16 spline trainer behind the constructor's width rule (``engine=None``: left
    float32 altogether)."""
    from pocomc_amd import Flow
    f = Flow(spec.n_dim, spec, seed=0)
    if engine is not None:
        f.precision = "bf16"
        f.train_engine = engine
    f.set_params(flat)
    return f


def _id(case):
    return "D%d-T%d-H%d-K%d-n%d-%s-s%g" % (case[0], case[1], case[2], case[3], case[4], "w" if case[5] else "u", case[6])


def _grad(f, x, w, **kw):
    from pocomc_amd.train import loss_and_grad, _train_state
    loss = float(loss_and_grad(f, x, w, **kw))
    return loss, _train_state(f).grad.cpu().numpy().copy()


@pytest.mark.parametrize("case", tm.CASES, ids=_id)
def test_loss_and_gradient_match_the_model_that_rounds_where_the_engine_rounds(case):
    from pocomc_amd._lib import PocomcAmdError
    from pocomc_amd.train import _train_state
    r = tm.case_reference(case)
    spec, flat = r["spec"], r["flat"]
    xd = torch.from_numpy(r["x"]).cuda()
    wd = None if r["w"] is None else torch.from_numpy(r["w"]).cuda()
    loss, g = _grad(spline_flow(spec, flat), xd, wd)
    d_round = np.linalg.norm(r["gT64"] - r["g64"])
    f32 = spline_flow(spec, flat, None)
    _train_state(f32).repack(f32)
    try:
        l32, g32 = _grad(f32, xd, wd)
        share = (f"float32 engine from plain autograd / d_round {np.linalg.norm(g32 - r['g64']) / d_round:.3f}, its loss "
                 f"{abs(l32 - r['loss64']) / abs(r['loss64']):.1e}")
    except PocomcAmdError as e:       # (D = 128 / H = 512: the float32 chain kernel's workgroup does not fit the LDS)
        share = f"float32 engine: {e}"
    v = tm.verdict(spec, loss, g.astype(np.float64), r)
    y = tm.verdict(spec, r["lossT32"], r["gT32"], r)
    print(f"{_id(case)}: d_round / |g| {d_round / np.linalg.norm(r['g64']):.1e} | engine overall {v['overall']:.3f}, worst tensor "
          f"{v['worst']:.3f} {v['where']}, loss {v['loss_rel']:.1e} | yardstick overall {y['overall']:.3f}, worst tensor "
          f"{y['worst']:.3f} | {share}")
    assert np.isfinite(g).all() and np.isfinite(loss)
    assert y["overall"] <= tm.YARD_OVERALL and y["worst"] <= tm.YARD_PER_TENSOR, y
    assert v["masked_zero"]
    assert v["loss_rel"] <= tm.LOSS_RTOL, v
    assert v["overall"] <= tm.OVERALL, v
    assert v["worst"] <= tm.PER_TENSOR, v


def test_rows_wholly_outside_the_box_are_the_identity():
    spec = MAFSpec(16, 2, hidden=64, univariate="rqs", bins=8)
    f = spline_flow(spec, tm.cases.flow_params(spec, 2, gain=1.0))
    rng = np.random.default_rng(7)
    x = (rng.uniform(6.0, 8.0, size=(40, 16)) * rng.choice([-1.0, 1.0], size=(40, 16))).astype(np.float32)
    loss, g = _grad(f, torch.from_numpy(x).cuda(), None)
    want = float((0.5 * (x.astype(np.float64) ** 2).sum(axis=1) + 0.5 * 16 * np.log(2 * np.pi)).sum())
    assert abs(loss - want) <= 1e-6 * abs(want)
    assert np.all(g == 0.0)


def test_indexed_batch_is_the_contiguous_batch_bit_for_bit():
    spec = MAFSpec(16, 2, hidden=64, univariate="rqs", bins=8)
    f = spline_flow(spec, tm.cases.flow_params(spec, 2, gain=1.0))
    n = 700                                            # two chunks of <= 512 rows
    rng = np.random.default_rng(5)
    x = torch.from_numpy((rng.normal(size=(n, 16)) * 2.5).astype(np.float32)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32)).cuda()
    loss, g = _grad(f, x, w)
    assert np.isfinite(loss) and np.abs(g).max() > 0.0
    perm = torch.randperm(n)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    loss2, g2 = _grad(f, x[perm.cuda()].contiguous(), w[perm.cuda()].contiguous(), idx=inv.cuda())
    assert loss2 == loss and np.array_equal(g2, g)
    # and a second call reproduces the first (fixed summation orders, no atomics)
    loss3, g3 = _grad(f, x, w)
    assert loss3 == loss and np.array_equal(g3, g)


@pytest.mark.parametrize("weighted", [False, True])
def test_epoch_call_equals_batch_by_batch(weighted):
    from pocomc_amd.train import loss_and_grad, AdamW
    rng = np.random.default_rng(3)
    n, D, bs = 1000, 16, 256
    x = torch.from_numpy((rng.normal(size=(n, D)) * 2.5).astype(np.float32)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32)).cuda() if weighted else None
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    spec = MAFSpec(D, 2, hidden=64, univariate="rqs", bins=8)
    flat = tm.cases.flow_params(spec, 2, gain=1.0)

    def run(epoch_call):
        f = spline_flow(spec, flat)
        opt = AdamW(f, 2e-3, weight_decay=0.01)
        acc = torch.zeros(1, dtype=torch.float32, device="cuda")
        if epoch_call:
            opt.epoch(x, w, perm, bs, 1.0, acc)
        else:
            for b0 in range(0, n, bs):
                idx = perm[b0:b0 + bs].contiguous()
                acc += loss_and_grad(f, x, w, idx=idx, refresh=False)
                opt.step(1.0)
        return f.params.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy(), float(acc), opt.t

    a, b, c = run(True), run(False), run(True)
    assert not np.array_equal(a[0], flat) and np.isfinite(a[3])
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    for u, v in zip(a, c):
        assert np.array_equal(u, v)


def test_the_switch():
    from pocomc_amd import Flow
    from test_gpu_bf16_spline import assert_image_in_step
    D = 10
    spec = MAFSpec(D, 3, hidden=256, univariate="rqs")
    f = Flow(D, spec, precision="bf16", train_engine="bf16_spline", seed=1)
    assert f.train_engine == "bf16_spline"
    with pytest.raises(ValueError, match="bf16_spline"):
        Flow(D, MAFSpec(D, 3, hidden=256), precision="bf16", train_engine="bf16_spline")       # an affine flow
    with pytest.raises(ValueError, match="bf16_spline"):
        Flow(D, spec, precision="f32", train_engine="bf16_spline")
    with pytest.raises(ValueError):
        Flow(D, spec, precision="bf16", train_engine="bf16_nsf")
    rng = np.random.default_rng(4)
    x = torch.from_numpy((rng.normal(size=(768, D)) * 1.5 + 0.3).astype(np.float32))
    # as attributes: the same refusals at fit
    a = Flow(D, MAFSpec(D, 3, hidden=256), precision="bf16", seed=1)
    a.train_engine = "bf16_spline"
    with pytest.raises(ValueError, match="bf16_spline"):
        a.fit(x, epochs=1)
    s = Flow(D, spec, seed=1)
    s.train_engine = "bf16_spline"
    with pytest.raises(ValueError, match="bf16_spline"):
        s.fit(x, epochs=1)
    # "bf16" stays the affine engine, and its message names the new value
    f.train_engine = "bf16"
    with pytest.raises(ValueError, match="affine") as e:
        f.fit(x, epochs=1)
    assert "bf16_spline" in str(e.value)
    f.train_engine = "bf16_spline"
    # pickle keeps the value
    g = pickle.loads(pickle.dumps(f))
    assert g.train_engine == "bf16_spline" and g.precision == "bf16" and torch.equal(g.params.cpu(), f.params.cpu())
    # train_engine=None keeps the float32 kernels, bit for bit
    fits = []
    for engine in (None, "f32"):
        h = Flow(D, spec, precision="bf16", train_engine=engine, seed=1)
        torch.manual_seed(11)
        h.fit(x, epochs=3, batch_size=256)
        assert getattr(h, "_wide", None) is None
        fits.append(h.params.cpu().numpy())
    assert np.array_equal(fits[0], fits[1])
    # a fit with the engine moves the parameters, and the bf16 forward image follows them
    before = f.params.clone()
    torch.manual_seed(11)
    f.fit(x, epochs=3, batch_size=256)
    assert f._wide is not None and not torch.equal(before, f.params) and torch.isfinite(f.params).all()
    assert not np.array_equal(f.params.cpu().numpy(), fits[0])       # (another engine than the float32 fits above)
    assert torch.isfinite(f.log_prob(x)).all()
    assert_image_in_step(f)


def test_fit_follows_the_float32_fit():
    """Same data, same start, same batches: training and validation loss both fall, the engine's fall from epoch 0 to the last
    epoch is at least 0.9 of the float32 engine's, and the fitted densities -- both under the float32 kernels -- differ by
    less than 0.1 of the float32 fit's own gain."""
    from pocomc_amd import Flow
    D = 24
    rng = np.random.default_rng(8)
    A = rng.normal(size=(D, D)) / np.sqrt(D) + np.eye(D)
    x = torch.from_numpy((rng.normal(size=(6000, D)) @ A.T + 0.5).astype(np.float32))
    spec = MAFSpec(D, 3, hidden=256, univariate="rqs")
    flat = spec.init_params(4)
    judge = Flow(D, spec)                               # float32 kernels for every log_prob below
    judge.set_params(flat)
    lp0 = judge.log_prob(x[:2000]).double().mean().item()
    hist, lp = {}, {}
    for name, kw in (("f32", {}), ("bf16_spline", dict(precision="bf16", train_engine="bf16_spline"))):
        f = Flow(D, spec, **kw)
        f.set_params(flat)
        hist[name] = f.fit(x, epochs=25, batch_size=512, validation_split=0.8, shuffle=False, annealing=False, patience=100)
        assert (getattr(f, "_wide", None) is not None) == (name == "bf16_spline")
        judge.set_params(f.params.cpu().numpy())
        lp[name] = judge.log_prob(x[:2000]).double().mean().item()
    l32, l16 = np.array(hist["f32"]["loss"]), np.array(hist["bf16_spline"]["loss"])
    v32, v16 = np.array(hist["f32"]["val_loss"]), np.array(hist["bf16_spline"]["val_loss"])
    print("train loss f32        :", np.array2string(l32, precision=3))
    print("train loss bf16_spline:", np.array2string(l16, precision=3))
    print("val loss f32          :", np.array2string(v32, precision=3))
    print("val loss bf16_spline  :", np.array2string(v16, precision=3))
    print("mean log_prob (float32 kernels): start", lp0, lp)
    assert np.isfinite(l16).all() and np.isfinite(v16).all()
    assert l16[-1] < l16[0] and v16[-1] < v16[0] and l32[-1] < l32[0] and v32[-1] < v32[0]
    assert l16[0] - l16[-1] >= 0.9 * (l32[0] - l32[-1])
    assert v16[0] - v16[-1] >= 0.9 * (v32[0] - v32[-1])
    gain = lp["f32"] - lp0
    assert gain > 0.0 and abs(lp["bf16_spline"] - lp["f32"]) < 0.1 * gain


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(n=1024, D=16):
    rng = np.random.default_rng(11)
    x = (rng.normal(size=(n, D)) * np.linspace(0.5, 2.0, D) + 0.3).astype(np.float32)
    w = rng.uniform(0.2, 1.0, size=n).astype(np.float32)
    return x, w


def _fit(x, w, sharded):
    spec = MAFSpec(x.shape[1], 3, hidden=64, univariate="rqs", bins=8)
    f = spline_flow(spec, spec.init_params(5))
    hist = f.fit(torch.from_numpy(x), weights=torch.from_numpy(w), validation_split=0.75, epochs=4, batch_size=256,
                 shuffle=False, annealing=False, patience=100, **({} if sharded else {"sharded": False}))
    return f, hist


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, w = _data()
    B, lb = 256, 256 // world
    rows = np.concatenate([np.arange(b0 + rank * lb, b0 + (rank + 1) * lb) for b0 in range(0, len(x), B)])
    f, hist = _fit(x[rows], w[rows], True)
    if rank == 0:
        np.savez(out, params=f.params.cpu().numpy(), loss=np.array(hist["loss"]), val=np.array(hist["val_loss"]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process(tmp_path):
    """Data-parallel training with the engine, the layout of ``test_gpu_train_bf16.py``'s two-rank test and its tolerances: a
    row's activations and output gradients do not depend on which rank holds it, so only the float32 order of the
    gradient sums differs."""
    import torch.multiprocessing as mp
    x, w = _data()
    out = str(tmp_path / "r0.npz")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = np.load(out)
    f, hist = _fit(x, w, False)
    p = f.params.cpu().numpy()
    print("two ranks against one process: loss", np.abs(got["loss"] / np.array(hist["loss"]) - 1).max(), "val",
          np.abs(got["val"] / np.array(hist["val_loss"]) - 1).max(), "parameters: max abs", np.abs(got["params"] - p).max(),
          "max of |d| / (5e-5 + 5e-3 |p|)", (np.abs(got["params"] - p) / (5e-5 + 5e-3 * np.abs(p))).max())
    assert f._wide is not None
    np.testing.assert_allclose(got["loss"], hist["loss"], rtol=5e-5)
    np.testing.assert_allclose(got["val"], hist["val_loss"], rtol=5e-5)
    np.testing.assert_allclose(got["params"], p, rtol=5e-3, atol=5e-5)


def test_sampler_runs_to_beta_one_with_the_engine():
    import pocomc_amd as pc
    from scipy.stats import uniform
    from test_gpu_bf16_spline import assert_image_in_step
    D = 4
    prior = pc.Prior([uniform(-5, 10)] * D)

    def loglike(x):
        return np.sum(-0.5 * ((x - 0.7) / 0.5) ** 2, axis=1)
    flow = pc.Flow(D, MAFSpec(D, 3, hidden=256, univariate="rqs"), precision="bf16", train_engine="bf16_spline", seed=2)
    s = pc.Sampler(prior=prior, likelihood=loglike, vectorize=True, flow=flow, random_state=5, n_effective=128,
                   n_active=64, train_config=dict(epochs=20))
    s.run(progress=False)
    assert s.flow is flow and s.flow.train_engine == "bf16_spline" and getattr(s.flow, "_wide", None) is not None
    logz, beta = s.evidence()[0], float(s.particles.get("beta", index=-1))
    print(f"bf16 spline trainer in a Sampler: beta {beta}, logZ {logz:.3f} (analytic {D * np.log(0.5 * np.sqrt(2 * np.pi)) - D * np.log(10.0):.3f})")
    assert beta == 1.0 and np.isfinite(logz)
    assert_image_in_step(s.flow)
