"""Blobs of a likelihood on the GPU (``Sampler(device_likelihood=True, device_blobs=True)``, a tensor ``blobs`` in the
kernels' ``state_dict``): the likelihood returns ``(logl, blobs)``, the blob rows live in HBM and the accept launch moves
an accepted walker's row (``pmc_step_t.blob_cur / blob_prop``).

Everything rests on one exact invariant, so no tolerance appears: with a blob function ``g`` that is row-wise and
independent of the layout of ``x``, a walker's blob is the likelihood's blob at the x it was last accepted at --
``blobs[k] == g(x[k])`` bit for bit for every walker that moved, and the blob it started with for every other."""
import numpy as np
import pytest
import torch

from .test_gpu_device_likelihood import FLOWS, KINDS, _problem, f_torch

SENTINEL = 10 ** 6          # walker k starts with -(k + 1) - SENTINEL in every element: no g below produces that


def _c0(x):
    return 2.0 * x[:, 0]


def _c1(x):
    """A column after column accumulation, like ``f_torch``."""
    acc = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    for j in range(x.shape[1]):
        acc = acc + x[:, j] ** 2
    return acc


def g(x):
    """float64 (n, 2): 16 bytes a row."""
    return torch.stack([_c0(x), _c1(x)], dim=1)


def g_f32x3(x):
    return torch.stack([_c0(x), _c1(x), _c0(x) - _c1(x)], dim=1).to(torch.float32)


def g_i32(x):
    return torch.floor(x[:, 0] * 1000.0).to(torch.int32)


def g_i64(x):
    return torch.floor(x[:, 1] * 1000.0).to(torch.int64)


def g_f64x2x2(x):
    a, b = _c0(x), _c1(x)
    return torch.stack([a, b, a + b, a * b], dim=1).reshape(-1, 2, 2)


def g_f64x40(x):
    a, b = _c0(x), _c1(x)
    return torch.stack([a * (j + 1.0) if j % 2 == 0 else b + float(j) for j in range(40)], dim=1)


def with_blobs(f, gg):
    return lambda xt: (f(xt), gg(xt))


def without_blobs(f):
    return lambda xt: (f(xt), None)


def sentinel(N, like):
    """(N, *blob_shape) of ``like``'s dtype on the GPU, walker k filled with -(k + 1) - SENTINEL."""
    col = -(torch.arange(N, dtype=torch.int64, device="cuda") + 1) - SENTINEL
    return col.reshape((N,) + (1,) * (like.ndim - 1)).expand((N,) + tuple(like.shape[1:])).to(like.dtype).contiguous()


def _g_of(gg, x):
    return gg(torch.from_numpy(np.ascontiguousarray(x)).cuda()).cpu().numpy()


def _call(kind, prob, loglike, logl0, blobs, n_max, scale=None, **extra):
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    D = x.shape[1]
    state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x),
                 beta=0.5, blobs=blobs)
    funcs = dict(loglike=loglike, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo, u_geometry=geo)
    opts = dict(n_max=n_max, n_steps=10 ** 6, progress_bar=None, proposal_scale=(scale or 0.25) / D ** 0.5, seed=5,
                device_likelihood=True, **extra)
    return getattr(pmcmc, kind)(state, funcs, opts)


def _assert_same(a, b):
    for k in ("u", "x", "logl", "logp", "logdetj"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("steps", "calls", "proposal_scale", "accept"):
        assert a[k] == b[k], (k, a[k], b[k])


def check_invariant(res, x0, start, gg, tag, need_both=True):
    """``blobs == g(x)`` on the rows that moved, the starting rows elsewhere; returns the mask of the moved rows."""
    blobs = res["blobs"]
    start = start.cpu().numpy()
    assert isinstance(blobs, np.ndarray) and blobs.shape == start.shape and blobs.dtype == start.dtype
    moved = (res["x"] != x0).any(axis=1)
    print(f"{tag}: moved {int(moved.sum())}, stayed {int((~moved).sum())} of {len(moved)}")
    if need_both:
        assert moved.any() and (~moved).any(), tag
    want = _g_of(gg, res["x"])
    assert np.array_equal(blobs[moved], want[moved]), tag
    assert np.array_equal(blobs[~moved], start[~moved]), tag
    return moved


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 1000])
@pytest.mark.parametrize("flow_name,D", FLOWS)
@pytest.mark.parametrize("kind", KINDS)
def test_blobs_follow_the_accepted_walkers_and_perturb_nothing(kind, flow_name, D, N):
    """All four kernels over the three pre-step launch sequences, whole blocks (N = 1024) and a tail block (N = 1000): the
    call with blobs is the call without them bit for bit, the moved walkers carry g(x), the others their sentinel.  Two
    steps: both sets are non-empty."""
    if not kind.startswith("preconditioned") and flow_name != "maf3":
        pytest.skip("pcn / rwm use no flow: covered once")
    prob = _problem(D, N, flow_name, seed=D)
    x0 = prob[4]
    logl0 = f_torch(torch.from_numpy(x0).cuda()).cpu().numpy()
    start = sentinel(N, g(torch.zeros(1, D, dtype=torch.float64, device="cuda")))
    a = _call(kind, prob, without_blobs(f_torch), logl0, None, n_max=2)
    b = _call(kind, prob, with_blobs(f_torch, g), logl0, start.clone(), n_max=2)
    _assert_same(a, b)
    assert a["blobs"] is None and b["steps"] == 2
    check_invariant(b, x0, start, g, f"{kind} {flow_name} N={N}")


WIDTHS = [(g_f32x3, torch.float32, (3,), 12, "preconditioned_pcn"), (g_i32, torch.int32, (), 4, "preconditioned_rwm"),
          (g_i64, torch.int64, (), 8, "pcn"), (g_f64x2x2, torch.float64, (2, 2), 32, "rwm"),
          (g_f64x40, torch.float64, (40,), 320, "preconditioned_pcn")]


@pytest.mark.gpu
@pytest.mark.parametrize("gg,dtype,shape,row_bytes,kind", WIDTHS, ids=[w[0].__name__ for w in WIDTHS])
def test_row_widths_and_dtypes(gg, dtype, shape, row_bytes, kind):
    """4 to 320 bytes a row (the last wider than one wavefront's dwords), the four dtypes, a tail block."""
    D, N = 6, 1000
    prob = _problem(D, N, "maf3", seed=11)
    x0 = prob[4]
    like = gg(torch.zeros(1, D, dtype=torch.float64, device="cuda"))
    assert like.dtype == dtype and tuple(like.shape[1:]) == shape and like[0].numel() * like.element_size() == row_bytes
    logl0 = f_torch(torch.from_numpy(x0).cuda()).cpu().numpy()
    start = sentinel(N, like)
    a = _call(kind, prob, without_blobs(f_torch), logl0, None, n_max=3)
    b = _call(kind, prob, with_blobs(f_torch, gg), logl0, start.clone(), n_max=3)
    _assert_same(a, b)
    assert b["blobs"].shape == (N,) + shape
    check_invariant(b, x0, start, gg, f"{gg.__name__} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["preconditioned_pcn", "pcn"])
def test_holes_and_gated_rows_never_move_a_blob(kind):
    """A likelihood that is NaN on a region, walkers at the edge of the prior's support: a NaN logl' and a row the gate set
    to -inf give alpha = 0, their blobs stay.  No row whose logl is still its first one changed its blob."""
    D, N = 5, 1024
    prob = _problem(D, N, "maf3", seed=9)
    x0 = prob[4]

    def holes(x):
        ll = f_torch(x)
        return torch.where(x[:, 1] < -0.4, torch.full_like(ll, float("nan")), ll)
    logl0 = f_torch(torch.from_numpy(x0).cuda()).cpu().numpy()
    start = sentinel(N, g(torch.zeros(1, D, dtype=torch.float64, device="cuda")))
    a = _call(kind, prob, without_blobs(holes), logl0, None, n_max=8, scale=1.0)
    b = _call(kind, prob, with_blobs(holes, g), logl0, start.clone(), n_max=8, scale=1.0)
    _assert_same(a, b)
    assert b["calls"] < 8 * N and np.isfinite(b["logl"]).all()         # rows were gated, no NaN was accepted
    moved = check_invariant(b, x0, start, g, f"holes {kind}", need_both=False)
    assert moved.any() and (b["x"][moved, 1] >= -0.4).all()
    first = b["logl"] == logl0
    print(f"holes {kind}: rows whose logl is their first {int(first.sum())}")
    assert np.array_equal(b["blobs"][first], start.cpu().numpy()[first])


@pytest.mark.gpu
def test_device_state_keeps_the_blobs_on_the_device():
    D, N = 6, 1024
    prob = _problem(D, N, "maf3", seed=1)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    start = sentinel(N, g(torch.zeros(1, D, dtype=torch.float64, device="cuda")))
    given = start.clone()
    r = _call("preconditioned_pcn", prob, with_blobs(f_torch, g), logl0, given, n_max=2, device_state=True)
    assert isinstance(r["blobs"], torch.Tensor) and r["blobs"].is_cuda and isinstance(r["x"], torch.Tensor)
    assert torch.equal(given, start)                                     # the caller's tensor is read, not written
    res = dict(x=r["x"].cpu().numpy(), blobs=r["blobs"].cpu().numpy())
    check_invariant(res, prob[4], start, g, "device_state")


@pytest.mark.gpu
def test_blob_contract_errors():
    """Blobs of the wrong shape, dtype or device, a missing blob, a later call with another blob_shape, numpy blobs in the
    state, replay and trace: ValueError naming the problem."""
    from pocomc_amd import mcmc as pmcmc
    D, N = 4, 256
    prob = _problem(D, N, "maf3", seed=2)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    start = sentinel(N, g(torch.zeros(1, D, dtype=torch.float64, device="cuda")))
    seen = []

    def changes_shape(xt):
        seen.append(1)
        return f_torch(xt), (g(xt) if len(seen) == 1 else g_f64x2x2(xt))
    bad = [(lambda xt: (f_torch(xt), g(xt)[:-1]), r"shape \(256, ...\), got \(255, 2\)"),
           (lambda xt: (f_torch(xt), g(xt).to(torch.float16)), "float16"),
           (lambda xt: (f_torch(xt), g(xt).float()), "dtype torch.float64 as in the first call, got torch.float32"),
           (lambda xt: (f_torch(xt), g(xt).cpu()), "device cuda:0, got one on cpu"),
           (lambda xt: (f_torch(xt), None), "NoneType"),
           (lambda xt: f_torch(xt), r"tuple \(logl, blobs\), got Tensor"),
           (lambda xt: (f_torch(xt), g(xt).cpu().numpy()), "ndarray"),
           (changes_shape, r"blob_shape \(2,\) as in the first call, got \(2, 2\)")]
    for fn, word in bad:
        with pytest.raises(ValueError, match=word):
            _call("preconditioned_pcn", prob, fn, logl0, start.clone(), n_max=3)
    assert len(seen) == 2
    for blobs, word in ((start.cpu(), "device"), (start.to(torch.float16), "float16"), (start[:-1], "shape"),
                        (start.cpu().numpy(), "blobs")):
        with pytest.raises(ValueError, match=word):
            _call("rwm", prob, with_blobs(f_torch, g), logl0, blobs, n_max=2)
    for kw in (dict(trace=[]), dict(replay=object())):
        prior, scaler, flow, geo, x, u = prob
        state = dict(u=u, x=x, logdetj=scaler.inverse(u)[1], logl=logl0, logp=prior.logpdf(x), beta=0.5, blobs=start.clone())
        with pytest.raises(ValueError, match="replayed variates and traces"):
            pmcmc.rwm(state, dict(loglike=with_blobs(f_torch, g), logprior=prior.logpdf, scaler=scaler, u_geometry=geo),
                      dict(n_max=2, n_steps=10, progress_bar=None, proposal_scale=0.5, device_likelihood=True), **kw)


def test_blob_checker_on_cpu_tensors():
    """``device_blobs`` itself (no GPU needed for the checks that come before the device's)."""
    from pocomc_amd.mcmc import device_blobs, device_logl
    ll = torch.zeros(4, dtype=torch.float64)
    assert device_logl((ll, None), 4, "cpu") is ll
    for dt in (torch.float64, torch.float32, torch.int64, torch.int32):
        b = torch.zeros(4, 3, dtype=dt)
        assert device_blobs((ll, b), 4, "cpu") is b
        assert device_blobs((ll, b), 4, "cpu", like=torch.empty(0, 3, dtype=dt)) is b
    t = torch.zeros(3, 4, dtype=torch.float64).t()                       # (4, 3), not contiguous
    out = device_blobs((ll, t), 4, "cpu")
    assert out.is_contiguous() and torch.equal(out, t)
    assert device_blobs((ll, torch.zeros(4, dtype=torch.int32)), 4, "cpu").shape == (4,)
    like = torch.empty(0, 3, dtype=torch.float64)
    ok = torch.zeros(4, 3, dtype=torch.float64)
    for out, kw, word in ((ll, {}, r"tuple \(logl, blobs\), got Tensor"), ((ll, ok, ok), {}, "a tuple of 3"),
                          ((ll, None), {}, "NoneType"), ((ll, np.zeros((4, 3))), {}, "ndarray"),
                          ((ll, torch.zeros(3, 3, dtype=torch.float64)), {}, r"shape \(4, ...\), got \(3, 3\)"),
                          ((ll, torch.zeros((), dtype=torch.float64)), {}, "shape"),
                          ((ll, torch.zeros(4, 3, dtype=torch.float16)), {}, "float16"),
                          ((ll, torch.zeros(4, 3, dtype=torch.bool)), {}, "bool"),
                          ((ll, torch.zeros(4, 0, dtype=torch.float64)), {}, "at least one element"),
                          ((ll, torch.zeros(4, 2, dtype=torch.float64)), dict(like=like), r"blob_shape \(3,\) as in the first call, got \(2,\)"),
                          ((ll, torch.zeros(4, 3, dtype=torch.int64)), dict(like=like), "dtype torch.float64 as in the first call, got torch.int64")):
        with pytest.raises(ValueError, match=word):
            device_blobs(out, 4, "cpu", **kw)
    with pytest.raises(ValueError, match="device cuda:0, got one on cpu"):
        device_blobs((ll, ok), 4, "cuda:0")


def test_step_struct_carries_the_blob_fields_at_its_end():
    """``pmc_step_t`` grew at its END: the offsets of everything before are the parent's, the sized structs keep their size."""
    import ctypes
    from pocomc_amd import _lib
    S = _lib.pmc_step_t
    names = [f[0] for f in S._fields_]
    assert names[-3:] == ["blob_cur", "blob_prop", "blob_row_bytes"] and names[-5:-3] == ["lik_x", "h_calls"]
    assert S.blob_cur.offset == S.h_calls.offset + 8 and ctypes.sizeof(S) == S.blob_row_bytes.offset + 8
    assert ctypes.sizeof(_lib.pmc_state_t) == 56 and ctypes.sizeof(_lib.pmc_proposal_t) == 72
    s = S()
    assert s.blob_cur is None and s.blob_prop is None and s.blob_row_bytes == 0       # zero: no blobs


@pytest.mark.gpu
def test_sampler_constructor_contract_for_device_blobs():
    from scipy.stats import uniform
    import pocomc_amd as pc
    prior = pc.Prior([uniform(-5, 10)] * 3)
    with pytest.raises(ValueError, match="device_blobs=True needs device_likelihood=True"):
        pc.Sampler(prior=prior, likelihood=f_torch, vectorize=True, device_blobs=True, random_state=0)
    with pytest.raises(ValueError, match="device_blobs"):
        pc.Sampler(prior=prior, likelihood=f_torch, vectorize=True, blobs_dtype=float, device_likelihood=True,
                   random_state=0)
    s = pc.Sampler(prior=prior, likelihood=with_blobs(f_torch, g), vectorize=True, device_likelihood=True,
                   device_blobs=True, random_state=0)
    assert s.have_blobs and s.device_blobs


def _sampler(blobs, **kw):
    from scipy.stats import uniform
    import pocomc_amd as pc
    D = 5
    prior = pc.Prior([uniform(-5, 10)] * D)
    like = with_blobs(f_torch, g) if blobs else f_torch
    return pc.Sampler(prior=prior, likelihood=like, vectorize=True, n_active=256, n_effective=512, random_state=7,
                      train_config={"epochs": 30}, device_likelihood=True, device_blobs=blobs, **kw)


@pytest.mark.gpu
def test_sampler_with_device_blobs(tmp_path, monkeypatch):
    """Default flow (nsf6), D = 5.  With ``device_blobs=True`` and without: samples, weights, logl, evidence and calls bit
    for bit.  The posterior's blobs, resampled or not, and ``results["blobs"]`` are g of the samples they belong to.  A run
    resumed from a mid-run checkpoint returns the uninterrupted run's samples and blobs -- given the random streams the
    uninterrupted run had at that checkpoint: they are not part of a state file (and loading one draws from torch's), so the
    test notes them when a state is saved and puts them back when it is loaded."""
    import pocomc_amd as pc
    streams = {}
    save = pc.Sampler.save_state

    def save_and_note_streams(self, path):
        streams[str(path)] = (np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state())
        return save(self, path)
    monkeypatch.setattr(pc.Sampler, "save_state", save_and_note_streams)
    load = pc.Sampler.load_state

    def load_and_restore_streams(self, path):
        load(self, path)
        np_state, cpu_state, gpu_state = streams[str(path)]
        np.random.set_state(np_state); torch.set_rng_state(cpu_state); torch.cuda.set_rng_state(gpu_state)
    monkeypatch.setattr(pc.Sampler, "load_state", load_and_restore_streams)
    out = []
    for blobs in (False, True):
        s = _sampler(blobs, output_dir=tmp_path / str(blobs), output_label="r")
        s.run(progress=False, n_total=1024, n_evidence=1024, save_every=2)
        x, w, logl, logp = s.posterior()
        out.append((x, w, logl, s.evidence(), s.calls))
    (xa, wa, la, za, ca), (xb, wb, lb, zb, cb) = out
    assert np.array_equal(xa, xb) and np.array_equal(wa, wb) and np.array_equal(la, lb)
    assert za == zb and ca == cb and np.isfinite(zb[0])
    with pytest.raises(ValueError, match="No blobs"):
        _sampler(False).posterior(return_blobs=True)

    x, w, logl, logp, b = s.posterior(return_blobs=True)
    assert np.array_equal(x, xb) and b.shape == (len(x), 2) and b.dtype == np.float64
    assert np.array_equal(b, _g_of(g, x))
    res = s.results
    T = res["x"].shape[0]
    assert res["blobs"].shape == (T, 256, 2) and res["blobs"].dtype == np.float64
    assert np.array_equal(res["blobs"].reshape(-1, 2), _g_of(g, res["x"].reshape(-1, 5)))
    assert np.array_equal(s.particles.get("blobs", index=-1), res["blobs"][-1])
    assert s.particles.blob_rows().is_cuda and all(isinstance(v, torch.Tensor) and v.is_cuda for v in s.particles.blobs)
    xr, lr, pr, br = s.posterior(resample=True, return_blobs=True)
    assert br.shape == (len(xr), 2) and np.array_equal(br, _g_of(g, xr))

    mid = sorted((tmp_path / "True").glob("r_[0-9]*.state"), key=lambda p: int(p.stem.split("_")[1]))
    assert len(mid) >= 2
    s2 = _sampler(True)
    s2.run(progress=False, n_total=1024, n_evidence=1024, resume_state_path=mid[1])
    assert s2.device_blobs is True and s2.particles.blob_rows().is_cuda
    x2, w2, _, _, b2 = s2.posterior(return_blobs=True)
    assert np.array_equal(x2, x) and np.array_equal(w2, w) and np.array_equal(b2, b)
    assert s2.evidence() == s.evidence() and s2.calls == s.calls

    # what a state file guarantees by itself, with the loading process's own streams: the saved pool and its blobs come back
    # to the device as they were, and the run that continues from them keeps the invariant
    monkeypatch.setattr(pc.Sampler, "load_state", load)
    s3 = _sampler(True)
    s3.load_state(mid[1])
    t_saved = s3.particles.T
    assert t_saved == int(mid[1].stem.split("_")[1]) and s3.particles.blob_rows().is_cuda
    assert np.array_equal(s3.particles.get("x"), res["x"][:t_saved])
    assert np.array_equal(s3.particles.get("blobs"), res["blobs"][:t_saved])
    s3.run(progress=False, n_total=1024, n_evidence=0)
    x3, _, _, _, b3 = s3.posterior(return_blobs=True)
    assert b3.dtype == np.float64 and np.array_equal(b3, _g_of(g, x3))
    assert np.array_equal(s3.results["blobs"][:t_saved], res["blobs"][:t_saved])
