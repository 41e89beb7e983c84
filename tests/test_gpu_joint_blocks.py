"""The blocks form of ``pocomc_amd.JointPrior``: several flow priors on disjoint blocks of columns and an optional table of
scipy factors on the others, evaluated by ``pmc_joint_blocks_pre`` -> every block's forward kernel -> ``pmc_joint_blocks_post``
(``csrc/joint_prior.hip``).

The first yardstick is the set of entries the pre kernel fuses: ``pmc_flow_prior_pre`` on every gathered block and
``pmc_prior_logpdf`` on the gathered rest, bit for bit; with one block and a table the single form's own entries.  The values
are held to ``tests/joint_blocks_model.py`` at the tolerances of ``tests/test_gpu_flow_prior.py``.  Layout, row position, bad
rows, ownership and the Sampler's two routes are bit-for-bit statements."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import cases
import flow_prior_model as fpm
import joint_blocks_model as jbm
import joint_prior_model as jpm
from oracle.maf import OracleMAF
from parity import close_rel, TOL
from pocomc_amd.maf_spec import MAFSpec
from .test_gpu_flow import NSF_LADJ
from .test_gpu_flow_prior import bits, bounds_of, gauss_at, make, pre, rows_in
from .test_gpu_joint_prior import build as build_single, jpre, table_logp

pytestmark = pytest.mark.gpu

A, S = "affine", "rqs"
# (blocks' widths, their univariate maps, their transforms, Dr)
SHAPES = {"2+2": ((2, 2), (A, S), ("probit", "probit"), 0),                       # D = 4, the smallest
          "2+3+2": ((2, 3), (S, A), ("probit", "logit"), 2),
          "3+2+2+1": ((3, 2, 2), (A, A, A), ("probit",) * 3, 1),                  # every block affine: held to TOL
          "5+17+11": ((5, 17), (S, A), ("logit", "probit"), 11),                  # D = 33: 512 is not a multiple of it
          "8x2+1": ((2,) * 8, (A, S) * 4, ("probit", "logit") * 4, 1)}            # the most blocks
NS = [1, 63, 64, 65, 200]
_built = {}


def build(name, dists=None):
    """``(joint, oracle scalers, oracle flows, dists, block maps, rest_cols)`` of a shape of SHAPES, built once: every block
    the flow prior of ``test_gpu_flow_prior.make`` with parameters of its own, the columns interleaved across the blocks and
    the rest and not sorted."""
    import pocomc_amd as pc
    key = (name, None if dists is None else len(dists))
    if key not in _built:
        dims, unis, transforms, Dr = SHAPES[name]
        made = [make(Df, 3, uni, tr, seed=5 + b) for b, (Df, uni, tr) in enumerate(zip(dims, unis, transforms))]
        ds = jpm.rest_dists(Dr) if dists is None else dists
        columns = jbm.interleaved_blocks(dims, len(ds))
        joint = pc.JointPrior([m[0] for m in made], columns, pc.Prior(ds, device=True) if ds else None)
        maps, rest_cols = jbm.layout_blocks(columns, sum(dims) + len(ds))
        _built[key] = (joint, [m[1] for m in made], [m[2] for m in made], ds, maps, rest_cols)
    return _built[key]


def rows(maps, dists, rest_cols, n, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, sum(len(m) for m in maps) + len(dists)))
    for m in maps:
        x[:, m] = rows_in(bounds_of(len(m)), n, rng)
    if len(dists):
        x[:, rest_cols] = jpm.rest_rows(dists, n, rng)
    return x


def bpre(joint, xt):
    """``pmc_joint_blocks_pre`` alone on a C-contiguous tensor: ``([u32 of block b], ldj [B][n], rest_logp or None, inside)``."""
    from pocomc_amd import _lib
    n, D = xt.shape
    dims = [fp.dim for fp in joint.flow_priors]
    u32 = torch.empty(n * sum(dims), dtype=torch.float32, device=xt.device)
    ldj = torch.empty(joint.blocks, n, dtype=torch.float64, device=xt.device)
    rest_logp = torch.empty(n, dtype=torch.float64, device=xt.device) if joint.rest is not None else None
    inside = torch.empty(n, dtype=torch.int32, device=xt.device)
    _lib.check(_lib.load().pmc_joint_blocks_pre(C.byref(joint._jdesc), _lib.ptr(xt), D, 1, n, _lib.ptr(u32), _lib.ptr(ldj),
                                                _lib.ptr(rest_logp), _lib.ptr(inside), _lib.stream_handle()),
               "pmc_joint_blocks_pre")
    flat, pieces, o = u32.cpu().numpy(), [], 0
    for d in dims:
        pieces.append(flat[n * o:n * (o + d)].reshape(n, d))
        o += d
    return pieces, ldj.cpu().numpy(), None if rest_logp is None else rest_logp.cpu().numpy(), inside.cpu().numpy()


def sum_of_parts(joint, x, maps, rest_cols):
    """The left-to-right float64 sum of every block's ``FlowPrior.logpdf_device`` on its gathered columns and the table."""
    v = None
    for fp, m in zip(joint.flow_priors, maps):
        part = fp.logpdf_device(x[:, torch.from_numpy(m).to(x.device)].contiguous()).cpu().numpy()
        v = part if v is None else v + part
    if joint.rest is not None:
        v = v + table_logp(joint.rest, x[:, torch.from_numpy(rest_cols).to(x.device)].contiguous())
    return v


# ------------------------------------------------------------------------------------------------------------------
# 1. the parts' bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_fused_kernel_gives_the_bits_of_its_parts(name):
    joint, _, _, dists, maps, rest_cols = build(name)
    assert joint.blocks == len(maps) and joint.dim == sum(len(m) for m in maps) + len(dists)
    for m in maps:
        assert not np.array_equal(m, np.sort(m))
    xt = torch.from_numpy(rows(maps, dists, rest_cols, max(NS), joint.dim)).cuda()
    for n in NS:
        x = xt[:n].contiguous()
        pieces, ldj, rest_logp, inside = bpre(joint, x)
        assert inside.all()
        for b, (fp, m) in enumerate(zip(joint.flow_priors, maps)):
            fu32, fldj, finside = pre(fp, x[:, torch.from_numpy(m).cuda()].contiguous())
            assert finside.all()
            assert np.array_equal(pieces[b].view(np.int32), fu32.view(np.int32)), (n, b)
            assert np.array_equal(ldj[b].view(np.int64), fldj.view(np.int64)), (n, b)
        if dists:
            want_rest = table_logp(joint.rest, x[:, torch.from_numpy(rest_cols).cuda()].contiguous())
            assert np.isfinite(want_rest).all() and np.array_equal(rest_logp.view(np.int64), want_rest.view(np.int64)), n
        got = joint.logpdf_device(x)
        assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
        want = sum_of_parts(joint, x, maps, rest_cols)
        assert np.isfinite(want).all() and np.array_equal(bits(got), want.view(np.int64)), n


# ------------------------------------------------------------------------------------------------------------------
# 2. one block with a table through the new entries: the single form's bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Df,Dr,uni", [(3, 4, S), (17, 16, A)])
def test_one_block_with_a_table_is_the_single_form(Df, Dr, uni):
    import pocomc_amd as pc
    single, prior, rest, _, _, dists, flow_cols, rest_cols = build_single(Df, Dr, uni)
    one = pc.JointPrior([prior], [flow_cols.tolist()], rest)
    assert one.blocks == 1 and single.blocks == 0 and one.dim == single.dim and np.array_equal(one.bounds, single.bounds)
    x = rows([flow_cols], dists, rest_cols, 200, Df)
    x[[0, 63, 64, 199], flow_cols[0]] = np.nan                           # rows outside: the same zeros and -inf
    xt = torch.from_numpy(x).cuda()
    for n in NS:
        u32, ldj, rest_logp, inside = jpre(single, xt[:n].contiguous())
        pieces, bldj, brest, binside = bpre(one, xt[:n].contiguous())
        assert np.array_equal(pieces[0].view(np.int32), u32.view(np.int32)) and np.array_equal(binside, inside)
        assert np.array_equal(brest.view(np.int64), rest_logp.view(np.int64))
        ok = inside != 0                                                 # (ldj of a row outside may be NaN: not compared)
        assert np.array_equal(bldj[0][ok].view(np.int64), ldj[ok].view(np.int64)) and not inside[0]
        assert np.array_equal(bits(one.logpdf_device(xt[:n])), bits(single.logpdf_device(xt[:n])))
    # ... and one block without a table is the flow prior on permuted columns
    alone = pc.JointPrior([prior], [flow_cols.argsort().argsort().tolist()])
    perm = torch.from_numpy(flow_cols.argsort().argsort()).cuda()
    y = torch.from_numpy(rows_in(bounds_of(Df), 130, np.random.default_rng(1))).cuda()
    z = torch.empty_like(y)
    z[:, perm] = y
    assert alone.dim == Df and alone.rest is None
    assert np.array_equal(bits(alone.logpdf_device(z)), bits(prior.logpdf_device(y)))


# ------------------------------------------------------------------------------------------------------------------
# 3. values against the model
# ------------------------------------------------------------------------------------------------------------------
def against_the_model(joint, oscalers, mafs, dists, maps, x, tol, what):
    """``close_rel`` against ``joint_blocks_model``, measured against the size of the sum's terms: every block's flow
    log-determinant terms and its scaler's log-determinant, plus the rest terms' absolute values."""
    columns = [m.tolist() for m in maps]
    want, _, terms = jbm.joint_blocks_model(oscalers, mafs, dists, columns, x)
    assert np.isfinite(want).all()
    cancel = np.abs(terms).sum(axis=1)
    for s, maf, m in zip(oscalers, mafs, maps):
        xb = x[:, m]
        cancel = cancel + maf.ladj_abs_terms(s.forward(xb).astype(np.float32)) + np.abs(fpm.flow_prior_model(s, maf, xb)[1])
    got = joint.logpdf_device(torch.from_numpy(x).cuda())
    worst = close_rel(got.cpu().numpy(), want, 1.0, f"{what} measured", cancel=cancel)
    print(f"{what}: log p max relative error {worst:.3e} (bound {tol:g})")
    close_rel(got.cpu().numpy(), want, tol, what, cancel=cancel)
    return got


@pytest.mark.parametrize("name", list(SHAPES))
def test_values_match_the_model(name):
    """200 rows; the n of NS are prefixes of them and carry the same bits, so every n is held by this comparison.  Measured on
    the MI355X, relative to the size of the sum's terms (bound ``NSF_LADJ`` with a spline block, ``TOL`` for 3+2+2+1, whose blocks
    are all affine): 7.2e-6 (2+2), 4.5e-7 (2+3+2), 4.0e-7 (5+17+11), 2.3e-6 (8x2+1); 3.2e-7 (3+2+2+1)."""
    joint, oscalers, mafs, dists, maps, rest_cols = build(name)
    x = rows(maps, dists, rest_cols, max(NS), joint.dim)
    tol = TOL if all(u == A for u in SHAPES[name][1]) else NSF_LADJ
    got = against_the_model(joint, oscalers, mafs, dists, maps, x, tol, f"joint blocks log p ({name})")
    xt = torch.from_numpy(x).cuda()
    for n in NS:
        assert np.array_equal(bits(joint.logpdf_device(xt[:n])), bits(got[:n])), n


# ------------------------------------------------------------------------------------------------------------------
# 4. D = 157
# ------------------------------------------------------------------------------------------------------------------
def wide(dims, Dr):
    import pocomc_amd as pc
    priors, oscalers, mafs = [], [], []
    for b, Df in enumerate(dims):
        bounds = bounds_of(Df)
        spec = MAFSpec(Df, 2, 160)
        flat = cases.flow_params(spec, 5 + b)
        flow = pc.Flow(Df, spec)
        flow.set_params(flat)
        train = rows_in(bounds, 500, np.random.default_rng(11 + b))
        scaler = pc.Reparameterize(Df, bounds=bounds)
        scaler.fit(train)
        priors.append(pc.FlowPrior(flow, scaler))
        oscalers.append(fpm.oracle_scaler(bounds, "probit", train))
        mafs.append(OracleMAF(spec, flat))
    dists = jpm.rest_dists(Dr)
    columns = jbm.interleaved_blocks(dims, Dr)
    return pc.JointPrior(priors, columns, pc.Prior(dists, device=True)), oscalers, mafs, dists, columns


@pytest.mark.parametrize("dims,Dr", [((70, 60, 25), 2), ((2, 2), 153)])
def test_the_widest_priors_match_the_model(dims, Dr):
    """D = 157 both ways; 65 rows: a full block and a row.  Measured on the MI355X: 2.1e-7 (70 + 60 + 25 + 2), 1.3e-7
    (2 + 2 + 153)."""
    n = 65
    joint, oscalers, mafs, dists, columns = wide(dims, Dr)
    assert joint.dim == 157
    maps, rest_cols = jbm.layout_blocks(columns, 157)
    x = rows(maps, dists, rest_cols, n, Dr)
    got = against_the_model(joint, oscalers, mafs, dists, maps, x, TOL, f"joint blocks log p ({dims} + {Dr})")
    xt = torch.from_numpy(x).cuda()
    assert np.array_equal(bits(joint.logpdf_device(xt.t().contiguous().t())), bits(got))


# ------------------------------------------------------------------------------------------------------------------
# 5. layouts and row position
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2+2", "2+3+2", "5+17+11", "8x2+1"])
@pytest.mark.parametrize("n", [1, 65, 200])
def test_every_layout_gives_the_same_bits(name, n):
    joint, _, _, dists, maps, rest_cols = build(name)
    D = joint.dim
    x = torch.from_numpy(rows(maps, dists, rest_cols, n, n)).cuda()
    colmajor = x.t().contiguous().t()
    wide_ = torch.zeros(n, 2 * D + 3, dtype=torch.float64, device="cuda")
    wide_[:, 1:2 * D + 1:2] = x
    sliced = wide_[:, 1:2 * D + 1:2]
    assert x.is_contiguous() and (n == 1 or colmajor.stride() == (1, n)) and torch.equal(sliced, x)
    a = joint.logpdf_device(x)
    assert torch.isfinite(a).all()
    for other in (colmajor, sliced, x):
        assert np.array_equal(bits(joint.logpdf_device(other)), bits(a))
    # ... and a row does not depend on its place in the call or on n
    if n > 64:
        assert np.array_equal(bits(joint.logpdf_device(x[37:])), bits(a[37:]))
        assert np.array_equal(bits(joint.logpdf_device(colmajor[64:])), bits(a[64:]))
    assert np.array_equal(joint.logpdf(x.cpu().numpy()).view(np.int64), bits(a))


# ------------------------------------------------------------------------------------------------------------------
# 6. bad rows
# ------------------------------------------------------------------------------------------------------------------
HOLES = [0, 63, 64, 129]                 # first row, a block's last, the next block's first, the call's last


def test_bad_rows_are_minus_infinity_and_move_nothing_else():
    """130 rows, blocks of 3, 2 and 2 columns (affine; block 1: feature 0 two-sided on (-1, 2), 1 bounded below at 0.5) and the factors
    uniform on [-2, 3], norm and a gamma(0.5, loc=1) whose logpdf is +inf at 1.  Every kind of bad row at every one of HOLES,
    then one of each kind in one call: exactly -inf there and never NaN, every other row the bits of the call without bad
    rows, in both layouts."""
    from scipy.stats import gamma
    n = 130
    dists = jpm.rest_dists(2) + [gamma(0.5, loc=1.0)]
    joint, _, _, _, maps, rc = build("3+2+2+1", dists=dists)            # (its third block: 2 columns, affine)
    x = rows(maps, dists, rc, n, 3)
    good = bits(joint.logpdf_device(torch.from_numpy(x).cuda()))
    assert np.isfinite(good.view(np.float64)).all()
    # what: (column, value, inside)
    kinds = {"NaN in a block-0 column": (maps[0][2], np.nan, 0), "inf in a block-1 column": (maps[1][1], np.inf, 0),
             "block 1 on its lower bound": (maps[1][0], -1.0, 0), "block 1 on its upper bound": (maps[1][0], 2.0, 0),
             "block 1 on a bound below": (maps[1][1], 0.5, 0), "-inf in a block-2 column": (maps[2][0], -np.inf, 0),
             "NaN in a rest column": (rc[1], np.nan, 0), "beyond the uniform factor": (rc[0], 3.5, 1),
             "the gamma(0.5) pole": (rc[2], 1.0, 1)}

    def check(y, bad, what, inside_want):
        keep = np.setdiff1d(np.arange(n), bad)
        for yt in (torch.from_numpy(y).cuda(), torch.from_numpy(y).cuda().t().contiguous().t()):
            got = joint.logpdf_device(yt).cpu().numpy()
            assert np.isneginf(got[bad]).all(), (what, got[bad])
            assert not np.isnan(got).any() and not np.isposinf(got).any(), what
            assert np.array_equal(got[keep].view(np.int64), good[keep]), what
        pieces, ldj, rest_logp, ins = bpre(joint, torch.from_numpy(y).cuda())
        assert np.array_equal(ins[bad], inside_want) and ins[keep].all(), (what, ins[bad])
        out = np.asarray(bad)[np.asarray(inside_want) == 0]
        for p in pieces:                                                 # zeros in EVERY block's u32, not only the bad one's
            assert not p[out].any() and np.isfinite(p).all(), what
        assert np.isneginf(rest_logp[out]).all() and np.isfinite(rest_logp[keep]).all(), what
    for what, (j, v, ins) in kinds.items():
        y = x.copy()
        y[HOLES, j] = v
        check(y, HOLES, what, [ins] * len(HOLES))
    y = x.copy()
    bad = HOLES + [100, 65, 1, 62, 128]
    assert len(bad) == len(kinds)
    for r, (j, v, _) in zip(bad, kinds.values()):
        y[r, j] = v
    check(y, bad, "one of each", [k[2] for k in kinds.values()])
    # the pole is +inf in the table's own sum; the join maps it
    y = x.copy()
    y[7, rc[2]] = 1.0
    assert np.isposinf(bpre(joint, torch.from_numpy(y).cuda())[2][7])


# ------------------------------------------------------------------------------------------------------------------
# 7. a bf16 block
# ------------------------------------------------------------------------------------------------------------------
def test_a_bf16_block_keeps_its_kernel():
    """The bf16 flow of ``test_gpu_step_prior.test_a_bf16_flow_keeps_its_kernel`` as block 0 next to a float32 block and a
    factor: the block's part is its own ``FlowPrior.logpdf_device`` -- the matrix-core kernel's bits, not the float32 one's."""
    import pocomc_amd as pc
    d, n = 2, 200
    rng = np.random.default_rng(5)
    xb = rng.uniform(-0.95, 0.95, size=(n, d))
    fit = pc.Reparameterize(d, bounds=np.array([[-1.0, 1.0]] * d))
    fit.fit(xb)
    bf = pc.FlowPrior(pc.Flow(d, MAFSpec(d, 2, 16), seed=0, precision="bf16"), fit)
    f32 = pc.FlowPrior(pc.Flow(d, MAFSpec(d, 2, 16), seed=0), fit)
    other = make(3, 3, A)[0]
    dists = jpm.rest_dists(1)
    columns = [[5, 1], [3, 0, 4]]
    joint, plain = pc.JointPrior([bf, other], columns, pc.Prior(dists, device=True)), pc.JointPrior([f32, other], columns,
                                                                                                  pc.Prior(dists, device=True))
    assert joint.flow_priors[0].flow.precision == "bf16" and joint.flow_priors[1].flow.precision != "bf16"
    maps, rc = jbm.layout_blocks(columns, 6)
    x = np.empty((n, 6))
    x[:, maps[0]], x[:, maps[1]], x[:, rc] = xb, rows_in(bounds_of(3), n, rng), jpm.rest_rows(dists, n, rng)
    xt = torch.from_numpy(x).cuda()
    got = joint.logpdf_device(xt)
    part = bf.logpdf_device(xt[:, torch.from_numpy(maps[0]).cuda()].contiguous()).cpu().numpy()
    want = (part + other.logpdf_device(xt[:, torch.from_numpy(maps[1]).cuda()].contiguous()).cpu().numpy()) \
        + table_logp(joint.rest, xt[:, torch.from_numpy(rc).cuda()].contiguous())
    assert np.isfinite(want).all() and np.array_equal(bits(got), want.view(np.int64))
    assert not np.array_equal(bits(plain.logpdf_device(xt)), bits(got))           # (the bf16 kernel did run)


# ------------------------------------------------------------------------------------------------------------------
# 8. the class
# ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import pocomc_amd as pc
    from pocomc_amd import _lib
    from scipy.stats import gamma, norm, uniform
    lib = _lib.load()
    joint, _, _, dists, maps, rest_cols = build("2+3+2")
    a, b = joint.flow_priors
    cols = [m.tolist() for m in maps]
    rest = joint.rest
    # the class
    with pytest.raises(ValueError, match="block 1 must be a pocomc_amd.FlowPrior"):
        pc.JointPrior([a, rest], cols, rest)
    with pytest.raises(ValueError, match="9 flow blocks"):
        pc.JointPrior([a] * 9, [[2 * k, 2 * k + 1] for k in range(9)])
    with pytest.raises(ValueError, match="0 flow blocks"):
        pc.JointPrior([], [], rest)
    with pytest.raises(ValueError, match=r"Prior\(dists, device=True\)"):
        pc.JointPrior([a, b], cols, pc.Prior([gamma(2.0)] * 2))
    with pytest.raises(ValueError, match=r"Prior\(dists, device=True\)"):
        pc.JointPrior([a, b], cols, pc.Prior([norm()] * 2, device=False))
    with pytest.raises(ValueError, match="at least one factor"):
        pc.JointPrior([a, b], [[0, 1], [2, 3, 4]], pc.Prior([]))
    with pytest.raises(ValueError, match="pocomc_amd.Prior or None"):
        pc.JointPrior([a, b], cols, a)
    with pytest.raises(ValueError, match="blocks 0 and 1 overlap"):
        pc.JointPrior([a, b], [[0, 1], [1, 2, 3]], rest)
    with pytest.raises(ValueError, match="1 column lists for 2 blocks"):
        pc.JointPrior([a, b], [[0, 1]], rest)
    with pytest.raises(ValueError, match="must lie in"):
        pc.JointPrior([a, b], [[0, 1], [2, 3, 6]])                         # (without a rest there is no column 6)
    W = pc.JointPrior.MAX_DIM + 1
    assert W == 158 and pc.JointPrior.MAX_BLOCKS == 8
    many = pc.Prior([uniform(-1.0, 2.0)] * (W - 5))
    with pytest.raises(ValueError, match="too large"):
        pc.JointPrior([a, b], cols, many)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            far = pickle.loads(pickle.dumps(b))
        with pytest.raises(ValueError, match="different devices"):
            pc.JointPrior([a, far], cols, rest)
    assert not hasattr(joint, "device_descriptor")
    # the device function's own contract
    for bad in (torch.zeros(3, 7, device="cuda"), torch.zeros(3, 6, dtype=torch.float64, device="cuda"),
                torch.zeros(3, 7, dtype=torch.float64), np.zeros((3, 7))):
        with pytest.raises(ValueError):
            joint.logpdf_device(bad)
    assert joint.logpdf_device(torch.zeros(0, 7, dtype=torch.float64, device="cuda")).shape == (0,)
    assert joint.logpdf(np.zeros((0, 7))).shape == (0,)

    # the entries on the device: nothing is launched or written, the sentinels stay
    n = 4
    xt = torch.zeros(n, W, dtype=torch.float64, device="cuda")
    u32 = torch.full((n * 5,), 7.0, dtype=torch.float32, device="cuda")
    ldj = torch.full((2, n), 7.0, dtype=torch.float64, device="cuda")
    outs = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    ins = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = _lib.stream_handle()

    def copy_of(desc, **fields):
        c = type(desc).from_buffer_copy(desc)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def refused(text, j=None, x=xt, count=n, stride=7, out_u=u32):
        j = joint._jdesc if j is None else j
        rc = lib.pmc_joint_blocks_pre(None if j is False else C.byref(j), _lib.ptr(x), stride, 1, count, _lib.ptr(out_u),
                                      _lib.ptr(ldj), _lib.ptr(outs[0]), _lib.ptr(ins), st)
        assert rc != 0 and text in lib.pmc_last_error(), (text, rc, lib.pmc_last_error())
    refused(b"bad descriptor", j=False)
    refused(b"n_blocks must lie in", j=copy_of(joint._jdesc, n_blocks=9))
    refused(b"n_blocks must lie in", j=copy_of(joint._jdesc, n_blocks=0))
    j = copy_of(joint._jdesc)
    j.cols[1] = None
    refused(b"bad scaler descriptor", j=j)
    one = pc.Reparameterize(1, bounds=np.array([[-1.0, 1.0]]))
    one.fit(np.random.default_rng(0).uniform(-0.9, 0.9, size=(64, 1)))
    one_desc = one.device_descriptor()
    j = copy_of(joint._jdesc)
    j.scaler[0] = C.addressof(one_desc)
    refused(b"at least 2 columns", j=j)
    many_desc = many.device_descriptor()
    refused(b"n_dim too large", j=copy_of(joint._jdesc, rest=C.addressof(many_desc)))            # 2 + 3 + 153 = 158
    assert joint._rdesc.n_extended == 0
    ext = pc.Prior([gamma(2.0), gamma(3.0)], device=True).device_descriptor()
    no_par = copy_of(ext, par=None)
    refused(b"parameter table", j=copy_of(joint._jdesc, rest=C.addressof(no_par)))
    no_mu = copy_of(a._sdesc, mu=None)
    j = copy_of(joint._jdesc)
    j.scaler[0] = C.addressof(no_mu)
    refused(b"needs mu and sigma", j=j)
    refused(b"rest and rest_cols go together", j=copy_of(joint._jdesc, rest_cols=None))
    refused(b"bad argument", x=None)
    refused(b"bad argument", out_u=None)
    refused(b"bad argument", count=-1)
    refused(b"bad argument", stride=-1)
    refused(b"too many rows", count=64 * 2 ** 31)
    post = lambda *args: lib.pmc_joint_blocks_post(*args)
    lp32 = torch.zeros(2, n, dtype=torch.float32, device="cuda")
    assert post(2, None, _lib.ptr(ldj), _lib.ptr(outs[0]), _lib.ptr(ins), _lib.ptr(outs[1]), n, st) != 0
    assert b"pmc_joint_blocks_post: bad argument" in lib.pmc_last_error()
    assert post(9, _lib.ptr(lp32), _lib.ptr(ldj), _lib.ptr(outs[0]), _lib.ptr(ins), _lib.ptr(outs[1]), n, st) != 0
    assert b"pmc_joint_blocks_post: n_blocks must lie in" in lib.pmc_last_error()
    assert post(2, _lib.ptr(lp32), _lib.ptr(ldj), _lib.ptr(outs[0]), _lib.ptr(ins), _lib.ptr(outs[1]), 256 * 2 ** 31, st) != 0
    assert b"pmc_joint_blocks_post: too many rows" in lib.pmc_last_error()
    # n == 0 is no error, and reads nothing
    assert lib.pmc_joint_blocks_pre(C.byref(joint._jdesc), None, 7, 1, 0, None, None, None, None, st) == 0
    assert post(2, None, None, None, None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert (u32 == 7.0).all() and (ldj == 7.0).all() and (outs[0] == 7.0).all() and (outs[1] == 7.0).all() and (ins == 7).all()


def test_bounds_dim_pickling_ownership_and_rvs():
    import pocomc_amd as pc
    dims, unis, transforms, Dr = SHAPES["2+3+2"]
    sources = [make(Df, 3, uni, tr, seed=5 + b)[0] for b, (Df, uni, tr) in enumerate(zip(dims, unis, transforms))]
    dists = jpm.rest_dists(Dr)
    columns = jbm.interleaved_blocks(dims, Dr)
    rest = pc.Prior(dists, device=True)
    joint = pc.JointPrior(sources, columns, rest)
    maps, rc = jbm.layout_blocks(columns, 7)
    assert joint.dim == 7 and joint.blocks == 2 and isinstance(joint.flow_priors, tuple) and len(joint.flow_priors) == 2
    assert all(fp is not src for fp, src in zip(joint.flow_priors, sources))
    b = joint.bounds
    assert b.shape == (7, 2) and np.array_equal(b[rc], rest.bounds)
    for m, src in zip(maps, sources):
        assert np.array_equal(b[m], src.bounds)
    x = torch.from_numpy(rows(maps, dists, rc, 100, 1)).cuda()
    a = bits(joint.logpdf_device(x))
    back = pickle.loads(pickle.dumps(joint))
    assert isinstance(back, pc.JointPrior) and back.blocks == 2 and back.dim == 7 and np.array_equal(back.bounds, b)
    assert np.array_equal(bits(back.logpdf_device(x)), a)
    # a source block's flow changes: the source moves, the joint prior does not
    xb = x[:, torch.from_numpy(maps[1]).cuda()].contiguous()
    before = bits(sources[1].logpdf_device(xb))
    sources[1].flow.set_params(cases.flow_params(MAFSpec(3, 3, univariate=A), 9))
    assert not np.array_equal(bits(sources[1].logpdf_device(xb)), before)
    assert np.array_equal(bits(joint.logpdf_device(x)), a)
    rest.dists[1] = dists[0]
    assert np.array_equal(bits(joint.logpdf_device(x)), a) and np.array_equal(bits(back.logpdf_device(x)), a)
    # the blocks cover every column: no table
    bare = pc.JointPrior(sources, [[3, 0], [1, 4, 2]])
    assert bare.dim == 5 and bare.rest is None
    again = pickle.loads(pickle.dumps(bare))
    y = torch.from_numpy(rows([np.array([3, 0]), np.array([1, 4, 2])], [], [], 70, 2)).cuda()
    assert np.array_equal(bits(again.logpdf_device(y)), bits(bare.logpdf_device(y))) and torch.isfinite(bare.logpdf_device(y)).all()

    # draws: block 0, block 1, the rest, in this order; inside the bounds; the same seeds give the same rows
    def draw(p, size):
        torch.manual_seed(3)
        np.random.seed(3)
        return p.rvs(size)
    r = draw(joint, 300)
    assert r.shape == (300, 7) and r.dtype == np.float64
    for m in maps:
        assert (r[:, m] > b[m, 0]).all() and (r[:, m] < b[m, 1]).all()
    assert (r[:, rc] >= b[rc, 0]).all() and (r[:, rc] <= b[rc, 1]).all()
    assert np.isfinite(joint.logpdf(r)).all()
    assert np.array_equal(draw(joint, 300), r) and np.array_equal(draw(back, 300), r)
    torch.manual_seed(3)
    np.random.seed(3)
    first = joint.flow_priors[0].rvs(300)
    second = joint.flow_priors[1].rvs(300)
    assert np.array_equal(r[:, maps[0]], first) and np.array_equal(r[:, maps[1]], second)
    assert joint.rvs(1).shape == (1, 7) and draw(bare, 50).shape == (50, 5)


# ------------------------------------------------------------------------------------------------------------------
# 9. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
KW = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)


_blocks = []


def blocks_of_a_and_c():
    """Run A: a 4-D Gaussian, run C: a 3-D one, both under uniform priors; their marginal flows on A's columns 0, 1, 2 and on
    C's columns 0, 1.  Run once for every test that needs them (``tests/test_gpu_step_prior_blocks.py`` too)."""
    import pocomc_amd as pc
    from scipy.stats import uniform
    if _blocks:
        return _blocks[0]
    a = pc.Sampler(prior=pc.Prior([uniform(-10.0, 20.0)] * 4), likelihood=gauss_at(0.3), random_state=3, **KW)
    a.run(n_total=256, n_evidence=0, progress=False)
    c = pc.Sampler(prior=pc.Prior([uniform(-8.0, 16.0)] * 3), likelihood=gauss_at(-0.4), random_state=4, **KW)
    c.run(n_total=256, n_evidence=0, progress=False)
    torch.manual_seed(5)
    block_a = pc.FlowPrior.from_sampler(a, columns=[0, 1, 2], flow="maf3", train_config={"epochs": 30})
    block_c = pc.FlowPrior.from_sampler(c, columns=[0, 1], flow="maf3", train_config={"epochs": 30})
    _blocks.append((block_a, block_c))
    return _blocks[0]


@pytest.fixture(scope="module")
def runs_a_and_c():
    return blocks_of_a_and_c()


@pytest.mark.parametrize("own", [True, False])
def test_two_runs_blocks_as_the_prior_of_run_b_on_both_routes(runs_a_and_c, own, tmp_path):
    """B is 6-D: A's block on its columns 4, 0, 2, C's on 1, 5, one own factor on 3 -- or 5-D without an own factor.  Once with
    the prior inside the step and once through ``logpdf`` on the host route: the same bits."""
    import pocomc_amd as pc
    from scipy.stats import norm
    block_a, block_c = runs_a_and_c
    if own:
        prior, D = pc.JointPrior([block_a, block_c], [[4, 0, 2], [1, 5]], pc.Prior([norm(0.5, 2.0)])), 6
        box = np.array([[-10.0, 10.0], [-8.0, 8.0], [-10.0, 10.0], [-np.inf, np.inf], [-10.0, 10.0], [-8.0, 8.0]])
    else:
        prior, D = pc.JointPrior([block_a, block_c], [[3, 0, 2], [1, 4]]), 5
        box = np.array([[-10.0, 10.0], [-8.0, 8.0], [-10.0, 10.0], [-10.0, 10.0], [-8.0, 8.0]])
    assert prior.dim == D and prior.blocks == 2 and np.array_equal(prior.bounds, box)

    def run_b(on_device, **extra):
        s = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=on_device, **KW, **extra)
        s.run(n_total=256, n_evidence=0, progress=False)
        return s
    dev, host = run_b(True, output_dir=tmp_path), run_b(False)
    assert dev.device_prior is True and host.device_prior is False
    rd, rh = dev.results, host.results
    for k in ("x", "logp", "logl", "logz", "beta"):
        assert np.array_equal(np.asarray(rd[k]), np.asarray(rh[k])), k
    assert dev.evidence() == host.evidence() and dev.calls == host.calls
    assert np.isfinite(np.asarray(rd["logp"])).all() and np.asarray(rd["beta"])[-1] == 1.0
    xs = np.asarray(rd["x"]).reshape(-1, D)
    assert np.array_equal(prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    path = tmp_path / "b.state"
    dev.save_state(path)
    res = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=True, **KW)
    res.load_state(path)
    assert isinstance(res.prior, pc.JointPrior) and res.prior is not prior and res.prior.blocks == 2
    for k in ("x", "logp", "logl", "logz"):
        assert np.array_equal(np.asarray(res.results[k]), np.asarray(rd[k])), k
    assert np.array_equal(res.prior.logpdf(xs[:70]), prior.logpdf(xs[:70]))
