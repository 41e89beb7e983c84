"""The blocks form of ``JointPrior`` (several flow blocks and an optional table), what needs no GPU: ``layout_blocks`` (pure
numpy), the float64 restatement (``tests/joint_blocks_model.py``), the new structs and entries of the C ABI, every host-side
refusal of ``pmc_joint_blocks_pre`` / ``pmc_joint_blocks_post`` and of the blocks branch of ``pmc_step_prior_stage`` on fake
addresses (nothing is launched), and the hand-over decision, which does not see the new stage."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import flow_prior_model as fpm
import joint_blocks_model as jbm
import joint_prior_model as jpm
from oracle.maf import OracleMAF
from pocomc_amd.maf_spec import MAFSpec
from pocomc_amd.prior import JointPrior

from .test_step_handover_cpu import ADDR, FIELDS, STEP, descriptor, grid

SHAPES = [((2, 2), 0), ((2, 3), 2), ((3, 2, 2), 1), ((5, 17), 11), ((70, 60, 25), 2), ((2,) * 8, 1)]


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------
# layout_blocks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,Dr", SHAPES)
def test_layout_blocks_round_trips_shuffled_interleaved_maps(dims, Dr):
    D = sum(dims) + Dr
    columns = jbm.interleaved_blocks(dims, Dr)
    maps, rest_cols = JointPrior.layout_blocks(columns, dims, Dr)
    assert len(maps) == len(dims) and all(m.dtype == np.int32 for m in maps) and rest_cols.dtype == np.int32
    for m, c in zip(maps, columns):
        assert np.array_equal(m, c)                                      # the order given, not sorted
    assert len(rest_cols) == Dr and np.all(np.diff(rest_cols) > 0)      # the other positions, increasing
    assert np.array_equal(np.sort(np.concatenate(maps + [rest_cols])), np.arange(D))
    # a joint row taken apart by the maps and put together again is the row
    x = np.random.default_rng(D).normal(size=(5, D))
    y = np.empty_like(x)
    for m in maps:
        y[:, m] = x[:, m]
    y[:, rest_cols] = x[:, rest_cols]
    assert np.array_equal(x, y)
    # numpy arrays and tuples are column lists too, and the model's own statement of the layout agrees
    again = JointPrior.layout_blocks(tuple(np.asarray(c, dtype=np.int16) for c in columns), list(dims), Dr)
    assert all(np.array_equal(a, m) for a, m in zip(again[0], maps)) and np.array_equal(again[1], rest_cols)
    mm, mr = jbm.layout_blocks(columns, D)
    assert all(np.array_equal(a, m) for a, m in zip(mm, maps)) and np.array_equal(mr, rest_cols)
    # one block: the single form's layout
    if len(dims) == 2:
        one, rest1 = JointPrior.layout_blocks([columns[0]], [dims[0]], D - dims[0])
        f, r = JointPrior.layout(columns[0], dims[0], D - dims[0])
        assert np.array_equal(one[0], f) and np.array_equal(rest1, r)


@pytest.mark.parametrize("columns,what", [
    ([[0, 1, 2], [2, 4]], r"blocks 0 and 1 overlap \(column 2\)"),
    ([[0, 1, 2], [3, 4], [5, 0]], "blocks"),                             # (a third list: the count comes first)
    ([[0, 2, 2], [3, 4]], "block 0: columns are not distinct"),
    ([[0, 1, 2], [4, 4]], "block 1: columns are not distinct"),
    ([[0, 1, 7], [3, 4]], r"block 0: columns must lie in \[0, 7\)"),
    ([[0, 1, 2], [3, -1]], "block 1: columns must lie in"),
    ([[0, 1.0, 2], [3, 4]], "block 0: columns must be a sequence of integers"),
    ([[0, 1, 2], [True, False]], "block 1: columns must be a sequence of integers"),
    ([[0, 1, 2], "34"], "block 1: columns must be a sequence of integers"),
    ([[0, 1, 2], [3, None]], "block 1: columns must be a sequence of integers"),
    ([[0, 1], [3, 4]], "block 0: 2 columns for a flow prior of 3"),
    ([[0, 1, 2], [3, 4, 5]], "block 1: 3 columns for a flow prior of 2"),
    ([[0, 1, 2]], "1 column lists for 2 blocks"),
    ([[0, 1, 2], [3, 4], [5, 6]], "3 column lists for 2 blocks"),
    (5, "sequence of column lists")])
def test_layout_blocks_refuses_malformed_input(columns, what):
    with pytest.raises(ValueError, match=what):
        JointPrior.layout_blocks(columns, (3, 2), 2)


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
BOUNDS = np.array([[-1.0, 2.0], [0.5, np.inf], [-np.inf, 3.0]])


def _parts(dims=(3, 2), unis=("affine", "rqs"), transforms=("probit", "logit")):
    scalers, mafs = [], []
    for b, (Df, uni, tr) in enumerate(zip(dims, unis, transforms)):
        spec = MAFSpec(Df, 3, univariate=uni)
        mafs.append(OracleMAF(spec, cases.flow_params(spec, 5 + b)))
        scalers.append(fpm.oracle_scaler(BOUNDS[:Df], tr, jpm.flow_rows(BOUNDS[:Df], 500, np.random.default_rng(11 + b))))
    return scalers, mafs


def _rows(dims, dists, columns, n, seed):
    rng = np.random.default_rng(seed)
    D = sum(dims) + len(dists)
    maps, rest_cols = jbm.layout_blocks(columns, D)
    x = np.empty((n, D))
    for m, Df in zip(maps, dims):
        x[:, m] = jpm.flow_rows(BOUNDS[:Df], n, rng)
    if len(dists):
        x[:, rest_cols] = jpm.rest_rows(dists, n, rng)
    return x, maps, rest_cols


def test_the_model_is_the_sum_of_its_parts_and_minus_infinity_off_the_support():
    """Two blocks (3 affine probit, 2 spline logit; feature 0 of each two-sided on (-1, 2), feature 1 bounded below at 0.5)
    and four factors (0 uniform on [-2, 3], 2 a gamma with loc -1) plus a gamma(0.5, loc=1) with a pole.  One bad value per
    row; every other row keeps its bits."""
    from scipy import stats
    dims = (3, 2)
    scalers, mafs = _parts(dims)
    dists = jpm.rest_dists(4) + [stats.gamma(0.5, loc=1.0)]
    columns = jbm.interleaved_blocks(dims, len(dists))
    x, maps, rest_cols = _rows(dims, dists, columns, 40, 3)
    good, block_logp, terms = jbm.joint_blocks_model(scalers, mafs, dists, columns, x)
    assert np.isfinite(good).all() and block_logp.shape == (2, 40) and terms.shape == (40, 5)
    # the left-to-right float64 sum of flow_prior_model per block, plus scipy's terms
    parts = [np.array([fpm.flow_prior_model(s, m, x[r:r + 1, c])[0][0] for r in range(40)])
             for s, m, c in zip(scalers, mafs, maps)]
    rest = np.zeros(40)
    for j, d in zip(rest_cols, dists):
        rest = rest + d.logpdf(x[:, j])
    assert np.array_equal(good, (parts[0] + parts[1]) + rest)
    # one block with the same table is the single form's model
    single = jpm.joint_prior_model(scalers[0], mafs[0], dists[:1], [2, 0, 3], x[:, :4])[0]
    assert np.array_equal(jbm.joint_blocks_model(scalers[:1], mafs[:1], dists[:1], [[2, 0, 3]], x[:, :4])[0], single)
    assert np.isposinf(dists[4].logpdf(1.0))
    bad = {1: (maps[0][0], np.nan),                  # a NaN in a block-0 column
           7: (maps[1][1], np.inf),                  # an inf in a block-1 column
           12: (maps[1][0], -1.0), 15: (maps[1][0], 2.0), 18: (maps[1][1], 0.5),        # a bound of block 1
           21: (rest_cols[0], 3.5), 24: (rest_cols[2], -1.5),                           # outside a factor's support
           27: (rest_cols[4], 1.0)}                                                     # at a pole
    y = x.copy()
    for r, (j, v) in bad.items():
        y[r, j] = v
    got = jbm.joint_blocks_model(scalers, mafs, dists, columns, y)[0]
    rows = np.array(sorted(bad))
    keep = np.setdiff1d(np.arange(len(x)), rows)
    assert np.isneginf(got[rows]).all(), got[rows]
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    assert np.array_equal(got[keep].view(np.int64), good[keep].view(np.int64))
    alone = jbm.joint_blocks_model(scalers, mafs, dists, columns, y[keep])[0]
    assert np.array_equal(alone.view(np.int64), good[keep].view(np.int64))


def test_the_model_without_a_table():
    dims = (3, 2)
    scalers, mafs = _parts(dims)
    columns = [[4, 0, 2], [3, 1]]
    x, maps, rest_cols = _rows(dims, [], columns, 12, 5)
    good, block_logp, terms = jbm.joint_blocks_model(scalers, mafs, None, columns, x)
    assert len(rest_cols) == 0 and terms.shape == (12, 0) and np.isfinite(good).all()
    assert np.array_equal(good, block_logp[0] + block_logp[1])
    x[5, 3] = -1.0                                                       # block 1's feature 0 on its lower bound
    got = jbm.joint_blocks_model(scalers, mafs, None, columns, x)[0]
    assert np.isneginf(got[5]) and np.array_equal(np.delete(got, 5), np.delete(good, 5))


# ------------------------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------------------------
def test_the_abi_grew_by_new_entries_and_structs_only(lib):
    from pocomc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    hdr = open(os.path.join(root, "include", "pocomc_amd.h")).read()
    for text in ("#define PMC_ABI_VERSION 9", "#define PMC_JOINT_BLOCKS_MAX 8", "#define PMC_STEP_EXT2 2",
                 "} pmc_joint_blocks_t;", "} pmc_prior_blocks_stage_t;", "} pmc_step_ext2_t;",
                 "int pmc_joint_blocks_pre(const pmc_joint_blocks_t* j, const double* x, int64_t row_stride, int64_t col_stride",
                 "int pmc_joint_blocks_post(int32_t n_blocks, const float* lp32, const double* ldj, const double* rest_logp,"):
        assert text in hdr, text
    assert lib.pmc_abi_version() == 9 and _lib.PMC_STEP_EXT2 == 2 and _lib.PMC_JOINT_BLOCKS_MAX == 8
    assert hasattr(lib, "pmc_joint_blocks_pre") and hasattr(lib, "pmc_joint_blocks_post")
    J, G = _lib.pmc_joint_blocks_t, _lib.pmc_prior_blocks_stage_t
    # the sizes their field lists give: two int32, 8 + 8 pointers, 2 pointers; that, 3 x 8 words, 8 pointers
    assert C.sizeof(J) == 2 * 4 + (8 + 8 + 2) * 8 == 152
    assert J.scaler.offset == 8 and J.cols.offset == 72 and J.rest.offset == 136 and J.rest_cols.offset == 144
    assert C.sizeof(G) == C.sizeof(J) + 3 * 8 * 8 + 8 * 8 == 408
    assert G.blocks.offset == 0 and G.maf.offset == 152 and G.image16.offset == 216 and G.image_per_transform.offset == 280
    assert [getattr(G, k).offset for k in ("u32", "z", "lp32", "ldj", "rest_logp", "inside", "count", "h_count")] == \
        list(range(344, 408, 8))
    S, E, E2 = _lib.pmc_step_t, _lib.pmc_step_ext_t, _lib.pmc_step_ext2_t
    assert C.sizeof(E2) == C.sizeof(S) + 16 and E2.prior_stage.offset == C.sizeof(S) and E2.blocks_stage.offset == C.sizeof(S) + 8
    assert C.sizeof(E) == C.sizeof(S) + 8 and C.sizeof(S) == S.blob_row_bytes.offset + 8
    assert C.sizeof(_lib.pmc_prior_stage_t) == 15 * 8 and C.sizeof(_lib.pmc_scaler_t) == 7 * 8 + 4 * 4 + 8
    assert E2().blocks_stage is None and E2().prior_stage is None


# ------------------------------------------------------------------------------------------------------------------
# the entries' refusals: nothing is launched (there is no device here, and every array address is a fake)
# ------------------------------------------------------------------------------------------------------------------
def blocks_descriptor(dims=(3, 2), Dr=2):
    """A ``pmc_joint_blocks_t`` the entry accepts up to its launch: real host structs where the check follows a pointer (the
    scalers, the table), fake addresses for every device array.  Returns it with what it points to."""
    from pocomc_amd import _lib
    scalers = [_lib.pmc_scaler_t(low=0x10, high=0x20, mu=0x30, sigma=0x40, kind=0x50, log_width=0x60, D=d, scale=1)
               for d in dims]
    rest = _lib.pmc_prior_t(family=0x70, loc=0x80, scale=0x90, D=Dr, par=0xA0, n_extended=1)
    j = _lib.pmc_joint_blocks_t(n_blocks=len(dims))
    for b, s in enumerate(scalers):
        j.scaler[b] = C.addressof(s)
        j.cols[b] = 0x1000 + 0x100 * b
    if Dr:
        j.rest, j.rest_cols = C.addressof(rest), 0x2000
    return j, scalers, rest


def test_the_blocks_entries_refuse_before_any_launch(lib):
    D = 7
    seen = set()

    def refused(word, change=None, null=False, x=0x3000, n=21, rs=D, cs=1, u32=0x4000, ldj=0x5000, rl=0x6000, ins=0x7000,
                dims=(3, 2), Dr=2):
        j, scalers, rest = blocks_descriptor(dims, Dr)
        if change:
            change(j, scalers, rest)
        rc = lib.pmc_joint_blocks_pre(None if null else C.byref(j), x, rs, cs, n, u32, ldj, rl, ins, None)
        msg = lib.pmc_last_error().decode()
        assert rc != 0 and msg.startswith("pmc_joint_blocks_pre: ") and word in msg, (word, rc, msg)
        seen.add(msg)
    refused("bad descriptor", null=True)
    for n_blocks in (0, -1, 9):
        refused("n_blocks must lie in 1 .. 8", lambda j, s, r: setattr(j, "n_blocks", n_blocks))
    refused("bad scaler descriptor", lambda j, s, r: j.scaler.__setitem__(1, None))
    refused("bad scaler descriptor", lambda j, s, r: j.cols.__setitem__(0, None))
    for field in ("low", "high", "kind", "log_width"):
        refused("bad scaler descriptor", lambda j, s, r: setattr(s[1], field, None))
    refused("at least 2 columns", dims=(3, 1))
    refused("at least 2 columns", dims=(0, 2))
    refused("needs mu and sigma", lambda j, s, r: setattr(s[0], "mu", None))
    refused("needs mu and sigma", lambda j, s, r: setattr(s[1], "sigma", None))
    refused("rest and rest_cols go together", lambda j, s, r: setattr(j, "rest_cols", None))
    refused("rest and rest_cols go together", lambda j, s, r: setattr(j, "rest", None))
    for field in ("family", "loc", "scale"):
        refused("bad prior descriptor", lambda j, s, r: setattr(r, field, None))
    refused("bad prior descriptor", lambda j, s, r: setattr(r, "D", 0))
    refused("bad prior descriptor", lambda j, s, r: setattr(r, "n_extended", -1))
    refused("n_dim too large", dims=(100, 56), Dr=2)                     # 158
    refused("n_dim too large", dims=(2,) * 8, Dr=142)                    # 158
    refused("n_dim too large", dims=(100, 58), Dr=0)                     # 158 without a table
    refused("parameter table", lambda j, s, r: setattr(r, "par", None))
    for kw in (dict(x=None), dict(u32=None), dict(ldj=None), dict(rl=None), dict(ins=None), dict(n=-1), dict(rs=-1), dict(cs=-1)):
        refused("bad argument", **kw)
    refused("too many rows", n=64 * 2 ** 31)
    assert len(seen) == 11                                               # texts of their own
    # the widest descriptors pass the check: they are refused for their arguments
    refused("bad argument", dims=(70, 60, 25), Dr=2, x=None)
    refused("bad argument", dims=(2,) * 8, Dr=141, x=None)
    # without a table rest_logp is not needed; n == 0 returns 0 and reads nothing
    j, scalers, rest = blocks_descriptor((3, 2), 0)
    assert lib.pmc_joint_blocks_pre(C.byref(j), None, 5, 1, 0, None, None, None, None, None) == 0
    refused("bad argument", dims=(3, 2), Dr=0, rl=None, x=None)
    j, scalers, rest = blocks_descriptor()
    assert lib.pmc_joint_blocks_pre(C.byref(j), None, 7, 1, 0, None, None, None, None, None) == 0
    # ... but a bad descriptor is refused at n == 0 as well
    j.n_blocks = 9
    assert lib.pmc_joint_blocks_pre(C.byref(j), None, 7, 1, 0, None, None, None, None, None) != 0

    def post_refused(word, B=2, lp32=0x100, ldj=0x200, rl=0x300, ins=0x400, out=0x500, n=21):
        rc = lib.pmc_joint_blocks_post(B, lp32, ldj, rl, ins, out, n, None)
        msg = lib.pmc_last_error().decode()
        assert rc != 0 and msg.startswith("pmc_joint_blocks_post: ") and word in msg, (word, rc, msg)
    for B in (0, -2, 9):
        post_refused("n_blocks must lie in 1 .. 8", B=B)
    for kw in (dict(lp32=None), dict(ldj=None), dict(ins=None), dict(out=None), dict(n=-1)):
        post_refused("bad argument", **kw)
    post_refused("too many rows", n=256 * 2 ** 31)
    assert lib.pmc_joint_blocks_post(2, None, None, None, None, None, 0, None) == 0
    assert lib.pmc_joint_blocks_post(9, None, None, None, None, None, 0, None) != 0


def blocks_stage_struct(dims=(3, 2), Dr=2, n=21):
    """A ``pmc_step_ext2_t`` whose blocks stage the entry accepts up to its first launch."""
    from pocomc_amd import _lib
    j, scalers, rest = blocks_descriptor(dims, Dr)
    mafs = [_lib.pmc_maf_t(D=d) for d in dims]
    g = _lib.pmc_prior_blocks_stage_t(u32=0x100, z=0x200, lp32=0x300, ldj=0x400, rest_logp=0xA00 if Dr else None,
                                      inside=0x500, count=0x600, h_count=0x700)
    C.memmove(C.byref(g.blocks), C.byref(j), C.sizeof(j))
    for b, m in enumerate(mafs):
        g.maf[b] = C.addressof(m)
    s = _lib.pmc_step_ext2_t(n=n, D=sum(dims) + Dr, p_x=ADDR["p_x"], p_fin=0xB00, p_logp=ADDR["p_logp"],
                             ext=_lib.PMC_STEP_EXT2, blocks_stage=C.addressof(g))
    return s, g, (scalers, mafs, rest)


@pytest.mark.parametrize("Dr", [2, 0])
def test_the_blocks_stage_refuses_before_any_launch(lib, Dr):
    def refused(change, word, **kw):
        s, g, keep = blocks_stage_struct(Dr=Dr, **kw)
        change(s, g, keep)
        assert lib.pmc_step_prior_stage(C.byref(s), None) != 0, word
        msg = lib.pmc_last_error().decode()
        assert word in msg, (word, msg)
        return msg
    seen = set()
    seen.add(refused(lambda s, g, k: setattr(s, "prior", 0x3000), "device prior table as well"))
    seen.add(refused(lambda s, g, k: setattr(s, "prior_rows", 1), "GPU callable as well"))
    seen.add(refused(lambda s, g, k: setattr(s, "lik_x", 0x2000), "host likelihood"))
    for ws in ("u32", "z", "lp32", "ldj", "inside") + (("rest_logp",) if Dr else ()):
        refused(lambda s, g, k: setattr(g, ws, None), "pmc_step_prior_stage: null workspace")
    seen.add(refused(lambda s, g, k: setattr(g, "count", None), "device counter"))
    refused(lambda s, g, k: setattr(g, "h_count", None), "device counter")
    for n in (0, -3):
        seen.add(refused(lambda s, g, k: setattr(s, "n", n), "n < 1"))
    seen.add(refused(lambda s, g, k: setattr(s, "blocks_stage", None), "no prior_stage"))
    refused(lambda s, g, k: setattr(s, "ext", 0), "no prior_stage")               # (nothing behind the struct is read ...
    refused(lambda s, g, k: setattr(s, "ext", 1), "no prior_stage")               #  ... and with ext = 1 one word only)
    seen.add(refused(lambda s, g, k: setattr(s, "prior_stage", 0xF000), "prior_stage and blocks_stage are both set"))
    seen.add(refused(lambda s, g, k: setattr(s, "p_fin", None), "p_x, p_fin and p_logp"))
    seen.add(refused(lambda s, g, k: g.maf.__setitem__(1, None), "every block needs its scaler and its flow"))
    refused(lambda s, g, k: g.blocks.scaler.__setitem__(0, None), "every block needs its scaler and its flow")
    seen.add(refused(lambda s, g, k: g.image16.__setitem__(1, 0xC00), "image_per_transform"))
    # what pmc_joint_blocks_pre refuses, in its words
    for B in (0, 9):
        seen.add(refused(lambda s, g, k: setattr(g.blocks, "n_blocks", B), "pmc_joint_blocks_pre: n_blocks must lie in 1 .. 8"))
    seen.add(refused(lambda s, g, k: (setattr(k[0][1], "D", 1), setattr(k[1][1], "D", 1)),
                     "pmc_joint_blocks_pre: every flow block needs at least 2 columns"))
    seen.add(refused(lambda s, g, k: setattr(s, "D", 158), "pmc_joint_blocks_pre: n_dim too large", dims=(100, 58 - Dr)))
    seen.add(refused(lambda s, g, k: setattr(k[0][0], "mu", None), "pmc_joint_blocks_pre: scale=1 needs mu and sigma"))
    seen.add(refused(lambda s, g, k: g.blocks.cols.__setitem__(1, None), "pmc_joint_blocks_pre: bad scaler descriptor"))
    if Dr:
        seen.add(refused(lambda s, g, k: setattr(k[2], "par", None), "pmc_joint_blocks_pre: factors other than uniform"))
        seen.add(refused(lambda s, g, k: setattr(g.blocks, "rest_cols", None), "pmc_joint_blocks_pre: rest and rest_cols"))
    # widths
    seen.add(refused(lambda s, g, k: setattr(s, "D", 9), "the prior's width is not the step's D"))
    seen.add(refused(lambda s, g, k: setattr(k[1][1], "D", 3), "the flow's width is not the scaler's"))
    assert len(seen) == 17 + (2 if Dr else 0)                                     # texts of their own


def test_the_handover_does_not_see_the_blocks_stage(lib):
    """Every row of the hand-over grid: the struct with ``ext = 2`` and ``blocks_stage`` set equals, field for field, the
    same struct with ``ext = 0``."""
    from pocomc_amd import _lib

    def handover(s, epilogue):
        h, mode, unknown = _lib.pmc_handover_t(), C.c_int32(-7), C.c_int32(-7)
        assert lib.pmc_step_handover(C.byref(s), STEP, int(epilogue), C.byref(h), C.byref(mode), C.byref(unknown)) == 0
        return {k: getattr(h, k) or 0 for k in FIELDS}, mode.value, unknown.value
    n = 0
    for sw in grid():
        plain = descriptor(sw)
        assert plain.ext == 0
        with_stage = _lib.pmc_step_ext2_t()
        C.memmove(C.byref(with_stage), C.byref(plain), C.sizeof(plain))
        with_stage.ext, with_stage.blocks_stage = _lib.PMC_STEP_EXT2, 0xF000
        assert handover(with_stage, sw["epilogue"]) == handover(plain, sw["epilogue"]), sw
        n += 1
    assert n == 4096
