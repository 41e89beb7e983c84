"""The two-wave affine sweep (``csrc/maf_inverse_tri4.hip``: ``maf_inverse_tri5_kernel``) takes its constant tables -- the
tiles' degree words, the y offsets across the transform boundaries, the rank permutation of the last transform -- from an
image the host builds once per flow shape (``MAFSpec.sweep_tables``, ``PMC_MAF_TABLES``) instead of deriving them in every
workgroup.  With the image withheld (``pmc_maf_t.reserved`` without the bit: what a C caller's descriptor looks like) the
kernel builds them itself.  Both must give the same bits everywhere."""
import ctypes as C

import numpy as np
import pytest

from pocomc_amd.maf_spec import MAFSpec

# (name, D, spec): the headline shape; fewer ranks than a tile with padding groups; six transforms (the y offsets across
# five boundaries, both x arrays); an odd hidden width (padding slots inside the tiles and behind the last group -- the
# constructor never leaves a whole tile of padding, so the live tiles are all tiles for every spec it accepts)
FLOWS = [("maf3-d32", 32, lambda: MAFSpec(32, 3)), ("maf3-d6", 6, lambda: MAFSpec(6, 3)), ("maf3-d5", 5, lambda: MAFSpec(5, 3)),
         ("maf6-d16", 16, lambda: MAFSpec(16, 6)), ("maf3-d7-h41", 7, lambda: MAFSpec(7, 3, 41))]
IDS = [f[0] for f in FLOWS]
ROWS = [16, 21, 48]
TABLES = 4               # PMC_MAF_TABLES


# ------------------------------------------------------------------------------------------------------------------
# CPU: the image's shape and what its words say
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,make", FLOWS, ids=IDS)
def test_table_image_layout(name, D, make):
    spec = make()
    assert spec.has_sweep_tables
    T, nT, Dp = spec.n_transforms, spec.nT, spec.Dp
    meta = spec.device_meta()
    base = (8 + 2 * T * D + 4 * nT + 3) & ~3
    tab = spec.sweep_tables()
    assert len(meta) == base + len(tab) and np.array_equal(meta[base:], tab)
    assert np.array_equal(meta[:8 + 2 * T * D + 4 * nT], np.concatenate(
        [meta[:8], np.concatenate([np.argsort(o) for o in spec.orders]), np.concatenate(spec.orders), spec.quad_meta]))
    n_dgt, n_yt = (nT + 2) * 16, T * (nT + 2) * 4
    assert len(tab) == n_dgt + Dp + ((n_yt + T + 3) & ~3)
    dgt = tab[:n_dgt].reshape(nT + 2, 16)
    groups = spec.tile_groups()
    for tile in range(nT + 2):
        ranks = [int(g) for g in (dgt[tile, :4] & 0xffff) if g < D]
        assert ranks == (groups[tile] if tile < nT else [])
        assert all(dgt[tile, 12 + i] == 0x40000000 for i in range(4) if (dgt[tile, i] & 0xffff) >= D)
    prm = tab[n_dgt:n_dgt + Dp]
    assert np.array_equal(prm[:D], np.argsort(spec.orders[0]))
    yt = tab[n_dgt + Dp:n_dgt + Dp + n_yt].reshape(T, nT + 2, 4)
    woff = lambda r: 4 * (((r >> 4) << 8) + ((r & 3) << 6) + ((r >> 2) & 3))
    for tt in range(T):
        for tile in range(nT):
            for i in range(4):
                g = int(dgt[tile, i]) & 0xffff
                if g < D:
                    # rank g of transform tt is feature f; transform tt + 1 (which ran before) left f at ITS rank
                    f = int(np.argsort(spec.orders[tt])[g])
                    assert yt[tt, tile, i] == woff(g if tt == T - 1 else int(spec.orders[tt + 1][f]))


# ------------------------------------------------------------------------------------------------------------------
# GPU: with the image and without
# ------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _flow(D, make, tables):
    import pocomc_amd as pc
    flow = pc.Flow(D, make(), seed=1)
    assert flow._desc.reserved & TABLES
    if not tables:
        flow._desc.reserved &= ~TABLES
    return flow


def _propose_inverse(flow, D, n, kind):
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(100 * D + n)
    A = rng.normal(size=(D, D))
    cov = A @ A.T / D + np.eye(D)
    up = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    mu, icov, chol = up(rng.normal(size=D)), up(np.linalg.inv(cov)), up(np.linalg.cholesky(cov))
    cur32 = up(rng.normal(size=(n, D)), torch.float32)
    r = _lib.pmc_rng_t(gamma=None, normal=None, uniform=None, seed=1234, step=7, offset=5)
    mk = lambda *s, dt=torch.float64: torch.full(s, -7.0, dtype=dt, device="cuda")
    st = _lib.stream_handle()
    t64, qa, qb = mk(n, D), mk(n), mk(n)
    u, l = mk(n, D, dt=torch.float32), mk(n, dt=torch.float32)
    _lib.check(lib.pmc_propose_inverse(kind, _lib.ptr(cur32), _lib.ptr(mu), _lib.ptr(icov), _lib.ptr(chol), 5.0, 0.4,
                                       float((1 - 0.4 ** 2) ** 0.5), C.byref(r), _lib.ptr(t64), _lib.ptr(qa),
                                       _lib.ptr(qb), C.byref(flow._desc), _lib.ptr(u), _lib.ptr(l), n, st))
    # the plain sweep (no proposal): the inverse of the proposals just made
    t32 = t64.to(torch.float32)
    u2, l2 = mk(n, D, dt=torch.float32), mk(n, dt=torch.float32)
    _lib.check(lib.pmc_maf_inverse(C.byref(flow._desc), _lib.ptr(t32), _lib.ptr(u2), _lib.ptr(l2), n, 7, st))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(u=u, ladj=l, theta=t64, quad=qa, quad_prop=qb, u_plain=u2, ladj_plain=l2).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name,D,make", FLOWS, ids=IDS)
def test_propose_inverse_with_and_without_the_table_image(name, D, make):
    from pocomc_amd import _lib
    with_t, without = _flow(D, make, True), _flow(D, make, False)
    assert _lib.load().pmc_maf_inverse_auto_is_duo(C.byref(with_t._desc), 16) == 1
    for n in ROWS:
        for kind in (0, 1):                               # tpCN, RWM
            a, b = _propose_inverse(with_t, D, n, kind), _propose_inverse(without, D, n, kind)
            for k in a:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, n, kind)
            assert np.isfinite(a["u"]).all() and not (a["u"] == -7.0).any()        # (every row was written)
            assert np.array_equal(_bits(a["u"]), _bits(a["u_plain"])) and np.array_equal(_bits(a["ladj"]), _bits(a["ladj_plain"]))
            if kind == 0:
                assert not (a["quad"] == -7.0).any() and not (a["quad_prop"] == -7.0).any()


def _pre_step(flow, D, n):
    import torch
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd.mcmc import StepEngine
    prior = pc.Prior([uniform(-5, 10)] * D)
    rng = np.random.default_rng(10 * D + n)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    scaler.fit(rng.uniform(-5, 5, size=(2000, D)))
    x = rng.uniform(-4, 4, size=(n, D))
    u = scaler.forward(x)
    eng = StepEngine("preconditioned_pcn", n, D, flow, scaler, seed=9, x_order="F")
    assert eng.set_device_prior(prior)
    eng.load_state(u, x, scaler.inverse(u)[1], -0.5 * np.sum(x ** 2, axis=1), prior.logpdf(x))
    eng.set_geometry(mu=np.zeros(D), cov=np.eye(D))
    eng.propose(min(2.38 / D ** 0.5, 0.9), 5.0)          # (tpCN: sigma < 1)
    assert eng._direct_now and eng._step.no_fuse == 0
    eng._wait_pre_step()
    torch.cuda.synchronize()
    out = dict(u=eng.p_u, x=eng.p_x, logdetj=eng.p_logdetj, finite=eng.p_fin, logp=eng.p_logp, u32=eng.p_u32,
               ldjf=eng.p_ldjf, theta=eng.p_theta64, quad=eng.quad, quad_prop=eng.p_quad)
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out.update(host_x=np.array(eng._np_x, copy=True), host_finite=eng._np_fin.copy(), host_logp=eng._np_logp.copy(),
               clean=eng._np_clean.copy(), done=eng.h_done.numpy().copy())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,D,make", FLOWS, ids=IDS)
def test_fused_pre_step_with_and_without_the_table_image(name, D, make, monkeypatch):
    monkeypatch.setenv("PMC_NO_FUSE", "0")
    with_t, without = _flow(D, make, True), _flow(D, make, False)
    for n in ROWS:
        a, b = _pre_step(with_t, D, n), _pre_step(without, D, n)
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, n)
        clean = (a["finite"] != 0) & np.isfinite(a["logp"])
        assert a["done"][0] == 1 and a["clean"][0] == (~clean).sum() and np.array_equal(a["host_x"][clean], a["x"][clean])
