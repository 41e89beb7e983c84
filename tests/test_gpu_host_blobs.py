"""Blobs of a vectorised HOST likelihood (``Sampler(vectorize=True, blobs_dtype=...)``, a tensor ``blobs`` in the kernels'
``state_dict`` next to a host likelihood): the likelihood returns ``(logl, blobs)`` numpy on whole blocks, the walkers' blob
rows live in HBM, the proposals' in a pinned host buffer, and a launch behind each accept moves the accepted walkers' rows
(``pmc_step_t.blob_host``, ``pmc_blob_rows_move``) -- the call keeps the mode it takes without blobs.

The invariant of ``tests/test_gpu_device_blobs.py``, so no tolerance appears: with a blob function ``g`` that is row-wise
and independent of the layout of ``x``, ``blobs[k] == g(x[k])`` bit for bit for every walker that moved, and the sentinel
it started with for every other."""
import numpy as np
import pytest
import torch

from .test_gpu_device_likelihood import _problem

SENTINEL = 10 ** 6          # walker k starts with -(k + 1) - SENTINEL in every element: no g below produces that
D, N = 5, 200               # 200 rows: no multiple of the accept's 64-row blocks or of the move kernel's


def f_np(x):
    """Row-wise and independent of the batch and of the layout of ``x`` (C or Fortran): column after column.  Narrow next
    to the walkers' spread, so that a good part of the proposals is refused (see ``check_invariant``)."""
    acc = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        acc = acc + (x[:, j] - 0.3) ** 2
    return -0.5 * acc / 0.12 ** 2


def _colsum(x):
    acc = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        acc = acc + x[:, j]
    return acc


def _bits(col):
    return np.ascontiguousarray(col, dtype=np.float64).view(np.int64)


def g(x):
    """float64 (n, 3): [sum x, x0 x1, x2]."""
    return np.stack([_colsum(x), x[:, 0] * x[:, 1], 1.0 * x[:, 2]], axis=1)


def g_i32x1(x):
    """The low word of x0's bits: one dword a row."""
    return (_bits(x[:, 0]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(-1, 1)


def g_i32x3(x):
    """Low word, high word of x0's bits and the low word of x1's: an odd number of dwords."""
    b0, b1 = _bits(x[:, 0]), _bits(x[:, 1])
    w = np.stack([b0 & 0xFFFFFFFF, (b0 >> 32) & 0xFFFFFFFF, b1 & 0xFFFFFFFF], axis=1)
    return w.astype(np.uint32).view(np.int32)


def g_f32x2x3(x):
    a, b = _colsum(x), x[:, 0] * x[:, 1]
    return np.stack([a, b, a + b, a - b, 2.0 * a, 3.0 * b], axis=1).astype(np.float32).reshape(-1, 2, 3)


def g_f64x130(x):
    """260 dwords a row: more than one pass of a 256-thread block over a row."""
    a, b = _colsum(x), x[:, 0] * x[:, 1]
    return np.stack([a * (j + 1.0) if j % 2 == 0 else b + float(j) for j in range(130)], axis=1)


def g_i64x1(x):
    return _bits(x[:, 1]).reshape(-1, 1).copy()


def with_blobs(f, gg):
    return lambda x: (f(x), gg(x))


def without_blobs(f):
    return lambda x: (f(x), None)


def sentinel(n, like):
    """(n, *blob_shape) of ``like``'s dtype on the GPU, walker k filled with -(k + 1) - SENTINEL."""
    col = -(np.arange(n, dtype=np.int64) + 1) - SENTINEL
    host = np.broadcast_to(col.reshape((n,) + (1,) * (like.ndim - 1)), (n,) + like.shape[1:]).astype(like.dtype)
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


def _call(prob, loglike, blobs, kind="preconditioned_pcn", n_max=3, scale=2.0, replay=None, **extra):
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=f_np(x), logp=prior.logpdf(x), beta=0.5,
                 blobs=blobs)
    funcs = dict(loglike=loglike, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo, u_geometry=geo)
    opts = dict(n_max=n_max, n_steps=n_max, progress_bar=None, proposal_scale=scale / x.shape[1] ** 0.5, seed=5, **extra)
    return getattr(pmcmc, kind)(state, funcs, opts, replay=replay)


def _assert_same(a, b):
    for k in ("u", "x", "logl", "logp", "logdetj"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("steps", "calls", "proposal_scale"):
        assert a[k] == b[k], (k, a[k], b[k])


def check_invariant(res, x0, start, gg, tag):
    """``blobs == g(x)`` on the rows that moved, the sentinels elsewhere; between 5 % and 95 % of the walkers moved (a
    condition on the test's inputs: seed and proposal scale are fixed so that it holds).  Returns the moved rows' mask."""
    blobs = res["blobs"]
    start = start.cpu().numpy()
    assert isinstance(blobs, np.ndarray) and blobs.shape == start.shape and blobs.dtype == start.dtype
    moved = (res["x"] != x0).any(axis=1)
    print(f"{tag}: moved {int(moved.sum())}, stayed {int((~moved).sum())} of {len(moved)}, calls {res['calls']}, "
          f"evaluations {res['evaluations']}")
    assert 0.05 * len(moved) <= moved.sum() <= 0.95 * len(moved), tag
    want = gg(res["x"])
    assert np.array_equal(blobs[moved], want[moved]), tag
    assert np.array_equal(blobs[~moved], start[~moved]), tag
    return moved


# the modes a kernel call can take with a host likelihood (all of them hand the likelihood Fortran-ordered blocks)
MODES = {"pipelined": dict(x_order="F"),
         "pipelined-2-lanes": dict(x_order="F", lanes=2, first_lane=0.8),            # 160 + 40 rows
         "pipelined-3-lanes": dict(x_order="F", lanes=3),                             # 80 + 80 + 40 rows
         "lanes-on-streams": dict(x_order="F", pipeline=False, lanes=2, first_lane=0.8),
         "host-threads": dict(x_order="F", host_threads=2),
         "one-engine": dict()}                                                        # row-major x', copies, sigma from the host


@pytest.fixture(scope="module")
def prob():
    return _problem(D, N, "maf3", seed=D)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_blobs_follow_the_accepted_walkers_in_every_mode(prob, mode):
    """Three steps of 200 walkers: the call with blobs is the same call without them bit for bit, the moved walkers carry
    g(x), the others their sentinel.  The lanes are unequal and one has 40 rows, fewer than a 64-row block."""
    from pocomc_amd import mcmc as pmcmc
    opts = MODES[mode]
    if "lanes" in opts:
        le = pmcmc.LanedEngine("preconditioned_pcn", N, D, prob[2], prob[1], lanes=opts["lanes"],
                               first_fraction=opts.get("first_lane"), x_order="F", streams=False)
        sizes = [hi - lo for lo, hi in le.bounds]
        assert len(sizes) == opts["lanes"] and len(set(sizes)) > 1 and min(sizes) < 64, sizes
    x0 = prob[4]
    start = sentinel(N, g(np.zeros((1, D))))
    a = _call(prob, without_blobs(f_np), None, **opts)
    b = _call(prob, with_blobs(f_np, g), start.clone(), **opts)
    _assert_same(a, b)
    assert a["blobs"] is None and b["steps"] == 3
    check_invariant(b, x0, start, g, mode)


@pytest.mark.gpu
def test_device_state_keeps_the_blobs_on_the_device(prob):
    start = sentinel(N, g(np.zeros((1, D))))
    given = start.clone()
    r = _call(prob, with_blobs(f_np, g), given, x_order="F", lanes=2, device_state=True)
    assert isinstance(r["blobs"], torch.Tensor) and r["blobs"].is_cuda and isinstance(r["x"], torch.Tensor)
    assert torch.equal(given, start)                                     # the caller's tensor is read, not written
    res = dict(x=r["x"].cpu().numpy(), blobs=r["blobs"].cpu().numpy(), calls=r["calls"], evaluations=r["evaluations"])
    check_invariant(res, prob[4], start, g, "device_state")


SHAPES = [(g_i32x1, np.int32, (1,), 4), (g_i32x3, np.int32, (3,), 12), (g_f32x2x3, np.float32, (2, 3), 24),
          (g_f64x130, np.float64, (130,), 1040), (g_i64x1, np.int64, (1,), 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("gg,dtype,shape,row_bytes", SHAPES, ids=[s[0].__name__ for s in SHAPES])
def test_row_shapes_and_dtypes(prob, gg, dtype, shape, row_bytes):
    """One dword, an odd number of dwords, a multi-dimensional row, 260 dwords (more than one pass of a 256-thread block
    over a row), an int64; the integer blobs are bits of x, so they are exact.  Pipelined, two unequal lanes."""
    like = gg(np.zeros((1, D)))
    assert like.dtype == dtype and like.shape[1:] == shape and like[0].size * like.itemsize == row_bytes
    start = sentinel(N, like)
    opts = MODES["pipelined-2-lanes"]
    a = _call(prob, without_blobs(f_np), None, **opts)
    b = _call(prob, with_blobs(f_np, gg), start.clone(), **opts)
    _assert_same(a, b)
    assert b["blobs"].shape == (N,) + shape
    check_invariant(b, prob[4], start, gg, gg.__name__)


def _cut_problem(seed=3):
    """Walkers on the x0 >= 0 side of a prior whose support ends at x0 = 0, the scaler's box going on to -10: the boundary
    cuts through the proposals, a good part of them never reaches the likelihood."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd.geometry import Geometry
    prior = pc.Prior([uniform(0.0, 10.0)] + [uniform(-3, 6)] * (D - 1))
    rng = np.random.default_rng(seed)
    scaler = pc.Reparameterize(D, bounds=np.array([[-10.0, 10.0]] * D))
    x = 0.5 * rng.uniform(-2.0, 2.0, size=(N, D))
    x[:, 0] = np.abs(x[:, 0]) + 1e-3
    scaler.fit(x)
    u = scaler.forward(x)
    flow = pc.Flow(D, "maf3", seed=0)
    flow.set_params(0.25 * flow.params.cpu())
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    geo.normal_cov = np.cov(u.T)
    return prior, scaler, flow, geo, x, u


POISON = 7.0e77


@pytest.mark.gpu
@pytest.mark.parametrize("fill_rejected", [True, False])
@pytest.mark.parametrize("which", ["cut", "edge"])
def test_rows_that_never_reach_the_likelihood_never_move_a_blob(prob, which, fill_rejected):
    """``cut``: a half-bounded prior through the walkers, many proposals outside the support (the compacted x'[mask]);
    ``edge``: three walkers at the edge of the support, a few proposals outside (with ``fill_rejected`` their host rows carry
    the walker's current x and the whole block goes to the likelihood).  The spy sees no row outside the support, would
    poison the blob of one, and no poisoned blob is kept; the invariant holds."""
    pr = _cut_problem() if which == "cut" else prob
    lo0, hi0 = (0.0, 10.0) if which == "cut" else (-3.0, 3.0)
    seen = []

    def spy(x):
        assert np.isfinite(x).all()
        outside = (x[:, 0] < lo0) | (x[:, 0] > hi0) | (np.abs(x[:, 1:]) > 3.0).any(axis=1)
        seen.append((len(x), int(outside.sum())))
        b = g(x)
        b[outside] = POISON
        return f_np(x), b
    start = sentinel(N, g(np.zeros((1, D))))
    opts = dict(MODES["pipelined-2-lanes"], fill_rejected=fill_rejected, scale=1.0)
    a = _call(pr, without_blobs(f_np), None, **opts)
    b = _call(pr, spy, start.clone(), **opts)
    _assert_same(a, b)
    assert b["calls"] < 3 * N                                            # rows were left out of the likelihood
    assert b["evaluations"] >= b["calls"] and sum(s[0] for s in seen) == b["evaluations"]
    if not fill_rejected:
        assert b["evaluations"] == b["calls"]                            # only x'[mask] went to the likelihood
    elif which == "edge":
        assert b["evaluations"] > b["calls"]                             # whole blocks went, some rows' values were dropped
    assert sum(s[1] for s in seen) == 0 and not (b["blobs"] == POISON).any()
    check_invariant(b, pr[4], start, g, f"{which} fill_rejected={fill_rejected}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined-2-lanes", "one-engine"])
def test_nothing_moves_when_every_proposal_is_refused(prob, mode):
    start = sentinel(N, g(np.zeros((1, D))))
    prior, scaler, flow, geo, x, u = prob
    r = _call(prob, lambda xx: (np.full(len(xx), -np.inf), g(xx)), start.clone(), **MODES[mode])
    assert r["steps"] == 3 and r["accept"] == 0.0
    assert np.array_equal(r["blobs"], start.cpu().numpy())
    assert np.array_equal(r["x"], x) and np.array_equal(r["u"], u) and np.array_equal(r["logl"], f_np(x))
    assert np.array_equal(r["logp"], prior.logpdf(x)) and np.array_equal(r["logdetj"], scaler.inverse(u)[1])


# ---------------------------------------------------------------------------------------------------------------- Sampler
DS = 4


def gauss(x):
    acc = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        acc = acc + (x[:, j] - 0.5) ** 2
    return -0.5 * acc / 0.25


def _sampler(blobs, options, **kw):
    from scipy.stats import uniform
    import pocomc_amd as pc
    prior = pc.Prior([uniform(-5, 10)] * DS)
    like = (lambda x: (gauss(x), g(x))) if blobs else gauss
    return pc.Sampler(prior=prior, likelihood=like, vectorize=True, blobs_dtype=float if blobs else None, flow="maf3",
                      n_active=64, n_effective=128, random_state=3, train_config={"epochs": 30}, mcmc_options=options, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("options", [dict(x_order="F", lanes=2), dict()], ids=["pipelined-2-lanes", "one-engine"])
def test_sampler_with_blobs_of_a_vectorised_host_likelihood(options):
    """With ``blobs_dtype=float`` and without: samples, weights, logl, evidence and calls bit for bit; the posterior's blobs
    and ``results["blobs"]`` are g of the rows they belong to, and the pool's blobs live on the device."""
    out = []
    for blobs in (False, True):
        s = _sampler(blobs, options)
        s.run(progress=False, n_total=256, n_evidence=256)
        x, w, logl, logp = s.posterior(trim_importance_weights=False)
        out.append((x, w, logl, s.evidence(), s.calls))
    (xa, wa, la, za, ca), (xb, wb, lb, zb, cb) = out
    assert np.array_equal(xa, xb) and np.array_equal(wa, wb) and np.array_equal(la, lb)
    assert za == zb and ca == cb and np.isfinite(zb[0])
    x, w, logl, logp, b = s.posterior(return_blobs=True, trim_importance_weights=False)
    assert np.array_equal(x, xb) and len(x) == s.particles.P and b.shape == (len(x), 3) and b.dtype == np.float64
    assert np.array_equal(b, g(x))
    res = s.results
    T = res["x"].shape[0]
    assert res["blobs"].shape == (T, 64, 3) and np.array_equal(res["blobs"].reshape(-1, 3), g(res["x"].reshape(-1, DS)))
    assert s.particles.blob_rows().is_cuda and s.walkers["blobs"].is_cuda


@pytest.mark.gpu
def test_resumed_run_keeps_the_blobs(tmp_path):
    s = _sampler(True, dict(x_order="F", lanes=2), output_dir=tmp_path, output_label="r")
    s.run(progress=False, n_total=256, n_evidence=0, save_every=2)
    mid = sorted(tmp_path.glob("r_[0-9]*.state"), key=lambda p: int(p.stem.split("_")[1]))
    assert len(mid) >= 2
    s2 = _sampler(True, dict(x_order="F", lanes=2))
    s2.run(progress=False, n_total=256, n_evidence=0, resume_state_path=mid[len(mid) // 2])
    assert s2.particles.T > int(mid[len(mid) // 2].stem.split("_")[1]) and s2.particles.blob_rows().is_cuda
    res = s2.results
    assert np.array_equal(res["blobs"].reshape(-1, 3), g(res["x"].reshape(-1, DS)))
    wx, wb = s2.walkers["x"].cpu().numpy(), s2.walkers["blobs"].cpu().numpy()
    assert wb.shape == (64, 3) and np.array_equal(wb, g(wx))
    x, _, _, _, b = s2.posterior(return_blobs=True)
    assert np.array_equal(b, g(x))


@pytest.mark.gpu
def test_contract_errors(prob):
    """Unsupported dtypes at construction; a likelihood that returns logl alone, the wrong number of rows, another
    blob_shape on a later call, a row wider than PMC_BLOB_ROW_BYTES_MAX; tensor blobs with replayed variates or a trace."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    prior = pc.Prior([uniform(-5, 10)] * DS)
    for dt in (object, np.dtype([("a", "f8"), ("b", "i4")]), np.float16, bool):
        with pytest.raises(ValueError, match="float64, float32, int64 or int32.*vectorize=False"):
            pc.Sampler(prior=prior, likelihood=gauss, vectorize=True, blobs_dtype=dt, random_state=0)
    mk = lambda like: pc.Sampler(prior=prior, likelihood=like, vectorize=True, blobs_dtype=float, flow="maf3", n_active=64,
                                 n_effective=128, random_state=0, train_config={"epochs": 5})
    with pytest.raises(ValueError, match=r"tuple \(logl, blobs\), got ndarray"):
        mk(gauss).run(progress=False, n_total=128, n_evidence=0)
    with pytest.raises(ValueError, match=r"shape \(64, ...\), got \(63, 3\)"):
        mk(lambda x: (gauss(x), g(x)[:-1])).run(progress=False, n_total=128, n_evidence=0)
    wide = pmcmc.PMC_BLOB_ROW_BYTES_MAX // 8 + 1
    with pytest.raises(ValueError, match="PMC_BLOB_ROW_BYTES_MAX"):
        mk(lambda x: (gauss(x), np.zeros((len(x), wide)))).run(progress=False, n_total=128, n_evidence=0)
    n_calls = []

    def changes_shape(x):
        n_calls.append(1)
        return gauss(x), (g(x) if len(n_calls) == 1 else g(x)[:, :2])
    with pytest.raises(ValueError, match=r"blob_shape \(3,\) as in the first call, got \(2,\)"):
        mk(changes_shape).run(progress=False, n_total=128, n_evidence=0)
    assert len(n_calls) == 2

    # the kernel call: the same checks on what the likelihood returns, before anything of the step's accept is launched
    start = sentinel(N, g(np.zeros((1, D))))
    for fn, word in ((lambda x: f_np(x), r"tuple \(logl, blobs\), got ndarray"),
                     (lambda x: (f_np(x), g(x)[:-1]), "shape"),
                     (lambda x: (f_np(x), g(x)[:, :2]), r"blob_shape \(3,\) as in the first call, got \(2,\)"),
                     (lambda x: (f_np(x), None), "got None")):
        with pytest.raises(ValueError, match=word):
            _call(prob, fn, start.clone(), x_order="F")
    too_wide = torch.zeros(4, wide, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="PMC_BLOB_ROW_BYTES_MAX"):
        pmcmc.StepEngine("rwm", 4, D, None, prob[1]).set_host_blobs(too_wide)
    with pytest.raises(ValueError, match="replayed variates or traces"):
        _call(prob, with_blobs(f_np, g), start.clone(), replay=object())
    prior_, scaler, flow, geo, x, u = prob
    state = dict(u=u, x=x, logdetj=scaler.inverse(u)[1], logl=f_np(x), logp=prior_.logpdf(x), beta=0.5, blobs=start.clone())
    with pytest.raises(ValueError, match="replayed variates or traces"):
        pmcmc.rwm(state, dict(loglike=with_blobs(f_np, g), logprior=prior_.logpdf, scaler=scaler, u_geometry=geo),
                  dict(n_max=2, n_steps=10, progress_bar=None, proposal_scale=0.5), trace=[])


@pytest.mark.gpu
def test_move_entry_point_checks_its_arguments():
    """``pmc_blob_rows_move`` by itself: accepted rows move, rejected rows are not written; the size and alignment checks of
    ``pmc_step_post``'s blobs."""
    import ctypes as C
    from pocomc_amd import _lib
    lib = _lib.load()
    n, rb = 130, 12
    acc = (torch.arange(n, device="cuda") % 3 == 0).to(torch.int32)
    src = torch.arange(n * 3, dtype=torch.int32).reshape(n, 3).pin_memory()
    dst = torch.full((n, 3), -1, dtype=torch.int32, device="cuda")
    st = _lib.stream_handle()
    _lib.check(lib.pmc_blob_rows_move(acc.data_ptr(), src.data_ptr(), dst.data_ptr(), n, rb, st), "pmc_blob_rows_move")
    torch.cuda.synchronize()
    want = torch.where(acc.cpu().bool()[:, None], src, torch.full_like(src, -1))
    assert torch.equal(dst.cpu(), want)
    for args, word in (((acc.data_ptr(), src.data_ptr(), dst.data_ptr(), n, 10, st), "multiple of 4"),
                       ((acc.data_ptr(), src.data_ptr(), dst.data_ptr(), n, 0, st), "multiple of 4"),
                       ((acc.data_ptr(), src.data_ptr(), dst.data_ptr(), n, (1 << 20) + 4, st), "PMC_BLOB_ROW_BYTES_MAX"),
                       ((acc.data_ptr(), src.data_ptr() + 2, dst.data_ptr(), n, rb, st), "4-byte aligned"),
                       ((acc.data_ptr(), dst.data_ptr(), dst.data_ptr(), n, rb, st), "different buffers"),
                       ((None, src.data_ptr(), dst.data_ptr(), n, rb, st), "needs accept")):
        assert lib.pmc_blob_rows_move(*args) != 0 and word in lib.pmc_last_error().decode()
    assert lib.pmc_blob_rows_move(acc.data_ptr(), src.data_ptr(), dst.data_ptr(), 0, rb, st) == 0
    assert isinstance(C.sizeof(_lib.pmc_step_t), int) and _lib.pmc_step_t().blob_host == 0
