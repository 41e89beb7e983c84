"""The three kernels of one MCMC step in every width class up to their limit (``tests/step_widths.py`` has the lists, the
inputs, the references and the bounds; ``test_step_widths_cpu.py`` shows those sound).

``pmc_propose``: theta', quad and quad_prop within a first-order forward-error bound of an extended-precision reference
evaluated on the device's own variates (``pmc_rng_fill``); the inline draws, the float64 input, row shards and the rows
around the outputs bit for bit.  ``pmc_scaler_inverse[_prior]``: the row sum of the Jacobian terms in numpy's pairwise
order bit for bit, the four coordinate kinds against the float64 oracle, the three LDS plans against each other.
``pmc_accept``: alpha, the decisions, the moved state and the folded sums.  Every output is allocated with 16 guard rows
before and behind it, filled with a NaN payload (an int pattern for masks), which must come back untouched; the refusals at
the limits are argument checks on the host and must leave everything untouched.

Each ``run_*`` returns the worst ``error / bound`` it saw (``profiles/step_widths.md`` records them); a ratio above 1 fails."""
import ctypes as C

import numpy as np
import pytest

import step_widths as sw

pytestmark = pytest.mark.gpu

GUARD = 16
PATTERN = {np.dtype(np.float64): (np.uint64, 0x7FF8DEAD0000BEEF), np.dtype(np.float32): (np.uint32, 0x7FC0BEEF),
           np.dtype(np.int32): (np.uint32, 0x5A5A5A5A)}
SEED, STEP = 20241018, 5


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def up(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class Guarded:
    """A device array [rows][cols] (cols = None: a vector of ``rows`` elements) with GUARD pattern rows before and behind."""

    def __init__(self, rows, cols=None, dtype=np.float64):
        import torch
        self.vector = cols is None
        cols = 1 if cols is None else cols
        self.rows, self.cols, self.dtype = rows, cols, np.dtype(dtype)
        ut, self.pat = PATTERN[self.dtype]
        host = np.full((rows + 2 * GUARD) * cols, self.pat, dtype=ut).view(self.dtype)
        self.t = torch.from_numpy(host).cuda()
        self.ptr = C.c_void_p(self.t.data_ptr() + GUARD * cols * self.dtype.itemsize)

    def _split(self):
        full = bits(self.t.cpu().numpy())
        a, b = GUARD * self.cols, (GUARD + self.rows) * self.cols
        return full[:a], full[a:b], full[b:]

    def get(self):
        """The body; the guards must be untouched."""
        before, body, behind = self._split()
        assert (before == self.pat).all(), "rows before the output were written"
        assert (behind == self.pat).all(), "rows behind the output were written"
        out = body.view(self.dtype).reshape(self.rows, self.cols)
        return out[:, 0].copy() if self.vector else out.copy()

    def untouched(self):
        return all((p == self.pat).all() for p in self._split())


def lib_and_stream():
    import torch
    from pocomc_amd import _lib
    _lib.require_gpu()
    return _lib.load(), _lib, _lib.stream_handle(), torch


def last_error(lib):
    m = lib.pmc_last_error()
    return m.decode() if m else ""


# ----------------------------------------------------------------------------------------------------------------------
# 1. proposal
# ----------------------------------------------------------------------------------------------------------------------
def rng_fill(n, D, gamma_shape, offset=0, uniform=False):
    lib, _lib, st, torch = lib_and_stream()
    z = torch.empty(n, D, dtype=torch.float64, device="cuda")
    g = torch.empty(n, dtype=torch.float64, device="cuda")
    u = torch.empty(n, dtype=torch.float64, device="cuda") if uniform else None
    r = _lib.pmc_rng_t(gamma=None, normal=None, uniform=None, seed=SEED, step=STEP, offset=offset)
    _lib.check(lib.pmc_rng_fill(C.byref(r), float(gamma_shape), _lib.ptr(z), _lib.ptr(g), _lib.ptr(u), n, D, st), "pmc_rng_fill")
    return z, g, u


def propose(case, tpcn, z=None, g=None, lo=0, use64=False, expect_refusal=False):
    """One ``pmc_propose`` of rows [lo, n) with ``rng.offset = lo``; z / g: the supplied variates of those rows (device
    tensors) or None for the inline draws.  RWM gets no quadratic-form outputs."""
    lib, _lib, st, torch = lib_and_stream()
    D, n = case["D"], case["n"] - lo
    cur = case["cur32"][lo:]
    cur_d = up(cur.astype(np.float64)) if use64 else up(cur, np.float32)
    mu, S, L = up(case["mu"]), up(case["inv_cov"]), up(case["chol"])
    out = dict(theta=Guarded(n, D), theta32=Guarded(n, D, np.float32))
    if tpcn:
        out.update(quad=Guarded(n), quad_prop=Guarded(n))
    r = _lib.pmc_rng_t(gamma=g.data_ptr() if g is not None else None, normal=z.data_ptr() if z is not None else None,
                       uniform=None, seed=SEED, step=STEP, offset=lo)
    rc = lib.pmc_propose(0 if tpcn else 1, None if use64 else _lib.ptr(cur_d), _lib.ptr(cur_d) if use64 else None,
                         _lib.ptr(mu) if tpcn else None, _lib.ptr(S) if tpcn else None, _lib.ptr(L), case["nu"], case["sigma"],
                         case["cn_a"], C.byref(r), out["theta"].ptr, out["theta32"].ptr,
                         out["quad"].ptr if tpcn else None, out["quad_prop"].ptr if tpcn else None, n, D, st)
    torch.cuda.synchronize()
    if expect_refusal:
        return rc, last_error(lib), all(o.untouched() for o in out.values())
    _lib.check(rc, "pmc_propose")
    return {k: o.get() for k, o in out.items()}


def run_propose_width(D):
    worst = {}
    for n in sw.propose_rows(D):
        for cond in sw.CONDS:
            for nu in sw.NUS:
                if n != 81 and (cond, nu) != (1e4, 5.0):
                    continue                                   # (the row tails: one geometry is enough)
                case = sw.propose_case(D, n, cond, nu, seed=11)
                z, g, _ = rng_fill(n, D, 0.5 * (D + nu))
                zh, gh = z.cpu().numpy(), g.cpu().numpy()
                assert np.isfinite(zh).all() and (gh > 0).all()
                for tpcn in (True, False):
                    if not tpcn and nu != 5.0:
                        continue                               # (RWM does not read nu)
                    tag = (n, cond, nu, "tpcn" if tpcn else "rwm")
                    a = propose(case, tpcn, z, g)
                    ref = sw.propose_reference(case, zh, gh, tpcn)
                    for k, v in sw.propose_ratios(ref, a).items():
                        worst[k] = max(worst.get(k, 0.0), v)
                        assert v <= 1.0, (D, tag, k, v)
                    assert same_bits(a["theta32"], a["theta"].astype(np.float32)), (D, tag)
                    b = propose(case, tpcn)                    # inline draws
                    for k in a:
                        assert same_bits(a[k], b[k]), (D, tag, k, "inline draws != supplied draws")
                    c = propose(case, tpcn, use64=True)
                    for k in a:
                        assert same_bits(b[k], c[k]), (D, tag, k, "cur64 != cur32")
                    for lo in (16, 37):
                        if lo < n:
                            s = propose(case, tpcn, lo=lo)
                            for k in a:
                                assert same_bits(s[k], b[k][lo:]), (D, tag, k, f"shard from row {lo}")
                            s = propose(case, tpcn, z[lo:].contiguous(), g[lo:].contiguous(), lo=lo)
                            for k in a:
                                assert same_bits(s[k], b[k][lo:]), (D, tag, k, f"shard from row {lo}, supplied draws")
    return worst


@pytest.mark.parametrize("D", sw.PROPOSE_D)
def test_proposal_in_every_width_class(D):
    worst = run_propose_width(D)
    print(f"pmc_propose D = {D} ({'MFMA' if D <= 128 else 'LDS-staged VALU'} kernel): worst error / bound {worst}")
    assert set(worst) == {"theta", "quad", "quad_prop"}


def test_proposal_is_refused_above_its_limit():
    """D = 157 runs (above); D = 158 needs more than 160 KiB of LDS: the host refuses before any launch."""
    for tpcn in (True, False):
        case = sw.propose_case(sw.PROPOSE_D_MAX + 1, 17, 1.0, 5.0, seed=11)
        rc, msg, untouched = propose(case, tpcn, expect_refusal=True)
        assert rc != 0 and "n_dim too large" in msg, (rc, msg)
        assert untouched


# ----------------------------------------------------------------------------------------------------------------------
# 2. scaler
# ----------------------------------------------------------------------------------------------------------------------
PLANS = ("plain", "colmajor", "prior")


def plan_runs(plan, D):
    return D <= (sw.SCALER_D_MAX_PLAIN if plan == "plain" else sw.SCALER_D_MAX_KEEP_X)


def scaler_descriptor(low, high, mu, sigma, kind, bc, logit, sum_log_sigma):
    _, _lib, _, _ = lib_and_stream()
    D = len(kind)
    both = np.asarray(kind) == 3
    with np.errstate(invalid="ignore", divide="ignore"):
        log_width = np.where(both, np.log(high - low), 0.0)
    dev = dict(low=up(low), high=up(high), mu=up(mu), sigma=up(sigma), kind=up(kind, np.int32), log_width=up(log_width),
               bc=up(bc, np.int32) if bc is not None else None)
    desc = _lib.pmc_scaler_t(low=dev["low"].data_ptr(), high=dev["high"].data_ptr(), mu=dev["mu"].data_ptr(),
                             sigma=dev["sigma"].data_ptr(), kind=dev["kind"].data_ptr(),
                             bc=dev["bc"].data_ptr() if bc is not None else None, log_width=dev["log_width"].data_ptr(),
                             D=D, logit=int(logit), scale=1, reserved=0, sum_log_sigma=float(sum_log_sigma))
    return desc, dev


def prior_descriptor(D):
    _, _lib, _, _ = lib_and_stream()
    family, loc, scale = sw.plan_prior(D)
    dev = dict(family=up(family, np.int32), loc=up(loc), scale=up(scale))
    return _lib.pmc_prior_t(family=dev["family"].data_ptr(), loc=dev["loc"].data_ptr(), scale=dev["scale"].data_ptr(), D=D,
                            reserved=0, par=None, n_extended=0, reserved2=0), dev


def scaler_inverse(desc, u, plan):
    """One launch through the plan; None when the call is refused (asserted: the message, nothing written)."""
    lib, _lib, st, torch = lib_and_stream()
    n, D = u.shape
    ud = up(u)
    out = dict(u=Guarded(n, D), x=Guarded(n, D), logdetj=Guarded(n), finite=Guarded(n, dtype=np.int32))
    if plan == "colmajor":
        out["xT"] = Guarded(D, n)
    pd = keep = None
    if plan == "prior":
        out["logp"] = Guarded(n)
        pd, keep = prior_descriptor(D)
    rc = lib.pmc_scaler_inverse_prior(C.byref(desc), C.byref(pd) if pd is not None else None, None, _lib.ptr(ud), out["u"].ptr,
                                      out["x"].ptr, out["xT"].ptr if plan == "colmajor" else None, out["logdetj"].ptr,
                                      out["finite"].ptr, out["logp"].ptr if plan == "prior" else None, None, None, None, n, st)
    torch.cuda.synchronize()
    if not plan_runs(plan, D):
        assert rc != 0 and "n_dim too large" in last_error(lib), (plan, D, rc, last_error(lib))
        assert all(o.untouched() for o in out.values()), (plan, D)
        return None
    _lib.check(rc, f"pmc_scaler_inverse_prior ({plan}, D = {D})")
    res = {k: o.get() for k, o in out.items()}
    if plan == "prior":
        # logp is pmc_prior_logpdf's on the same x', bit for bit
        xd, fd = up(res["x"]), up(res["finite"], np.int32)
        lp = torch.empty(n, dtype=torch.float64, device="cuda")
        _lib.check(lib.pmc_prior_logpdf(C.byref(pd), _lib.ptr(xd), _lib.ptr(fd), _lib.ptr(lp), n, st), "pmc_prior_logpdf")
        assert same_bits(res["logp"], lp.cpu().numpy()), (plan, D)
    return res


def through_the_plans(desc, u):
    """The plain plan's result; the other plans must give its bits (x_colmajor: the transpose), or be refused."""
    D = u.shape[1]
    plain = scaler_inverse(desc, u, "plain")
    ran = ["plain"]
    for plan in PLANS[1:]:
        r = scaler_inverse(desc, u, plan)
        if r is None:
            continue
        ran.append(plan)
        for k in ("u", "x", "logdetj", "finite"):
            assert same_bits(r[k], plain[k]), (plan, D, k)
        if plan == "colmajor":
            assert same_bits(r["xT"], np.ascontiguousarray(plain["x"].T)), (plan, D)
        else:
            plain["logp"] = r["logp"]
    assert ran == [p for p in PLANS if plan_runs(p, D)]
    return plain


@pytest.mark.parametrize("D", sw.SCALER_D)
def test_scaler_row_sum_is_numpys_tree_in_every_plan(D):
    for n in sw.SCALER_N:
        c = sw.sum_tree_case(D, n)
        desc, keep = scaler_descriptor(c["low"], c["high"], c["mu"], c["sigma"], c["kind"], None, 0, c["sum_log_sigma"])
        got = through_the_plans(desc, c["u"])
        assert same_bits(got["logdetj"], c["logdetj"]), (D, n, int((got["logdetj"] != c["logdetj"]).sum()))
        assert same_bits(got["u"], c["u"]) and (got["finite"] == 1).all()
        np.testing.assert_allclose(got["x"], c["x"], rtol=1e-12)


# (boundary conditions sit on coordinates with both bounds: the first is coordinate 3)
MIXED = [(D, t, bc) for D in sw.SCALER_D for t in ("probit", "logit") for bc in (False, True) if not (bc and D < 4)]


@pytest.mark.parametrize("D,transform,bc", MIXED, ids=[f"{D}-{t}-{'bc' if bc else 'no-bc'}" for D, t, bc in MIXED])
def test_scaler_mixed_kinds_match_the_oracle(D, transform, bc):
    """Kinds cycling through none / low / high / both against ``oracle/scaler.py`` in float64, with the comparison of
    ``test_gpu_tools.py::test_scaler_matches_reference`` (x: 1e-12, logdetj: rtol 1e-12, atol 1e-11; u' after the
    boundary-condition round trip: 1e-11 like ``forward``)."""
    from oracle.mcmc import _scaler_step
    from oracle.scaler import Reparameterize
    periodic, reflective = sw.mixed_bc(D) if bc else (None, None)
    rng = np.random.default_rng([D, int(bc), transform == "logit"])
    osc = Reparameterize(D, sw.mixed_bounds(D), periodic=periodic, reflective=reflective, transform=transform)
    osc.fit(sw.mixed_samples(D, 600, rng))
    bcs = None
    if bc:
        bcs = np.zeros(D, dtype=np.int32)
        for i in periodic or []:
            bcs[i] |= 1
        for i in reflective or []:
            bcs[i] |= 2
    kind = np.where(osc.mask_left, 1, np.where(osc.mask_right, 2, np.where(osc.mask_both, 3, 0))).astype(np.int32)
    desc, keep = scaler_descriptor(osc.low, osc.high, osc.mu, osc.sigma, kind, bcs, transform == "logit",
                                   float(np.sum(np.log(osc.sigma))))
    for n in sw.SCALER_N:
        u = rng.uniform(-2.5, 2.5, size=(n, D))
        want_u, want_x, want_l = _scaler_step(osc, u)
        got = through_the_plans(desc, u)
        np.testing.assert_allclose(got["x"], want_x, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got["logdetj"], want_l, rtol=1e-12, atol=1e-11)
        np.testing.assert_allclose(got["u"], want_u, rtol=1e-11, atol=1e-11)
        assert (got["finite"] == 1).all()
        if n >= 65 and "logp" in got:
            assert 0 < np.isfinite(got["logp"]).sum() < n      # (the fused prior saw rows inside and outside its support)


def test_scaler_is_refused_above_its_limits():
    """The last widths that run are in SCALER_D (158 with x_colmajor / a fused prior, 319 without); one more is refused by
    the host's LDS arithmetic ahead of any launch, and nothing is written."""
    for plan, D in (("colmajor", sw.SCALER_D_MAX_KEEP_X + 1), ("prior", sw.SCALER_D_MAX_KEEP_X + 1),
                    ("plain", sw.SCALER_D_MAX_PLAIN + 1)):
        c = sw.sum_tree_case(D, 65)
        desc, keep = scaler_descriptor(c["low"], c["high"], c["mu"], c["sigma"], c["kind"], None, 0, c["sum_log_sigma"])
        assert not plan_runs(plan, D) and scaler_inverse(desc, c["u"], plan) is None


# ----------------------------------------------------------------------------------------------------------------------
# 3. accept
# ----------------------------------------------------------------------------------------------------------------------
def accept(case):
    lib, _lib, st, torch = lib_and_stream()
    D, n, pre = case["D"], case["n"], case["pre"]
    cur = {k: up(v, v.dtype) for k, v in case["cur"].items()}
    prop = {k: up(v, v.dtype) for k, v in case["prop"].items()}
    p = lambda d, k: d[k].data_ptr() if k in d else None
    state = _lib.pmc_state_t(theta32=p(cur, "theta32"), u=p(cur, "u"), x=p(cur, "x"), logdetj=p(cur, "logdetj"),
                             logl=p(cur, "logl"), logp=p(cur, "logp"), logdetj_flow=p(cur, "logdetj_flow"))
    proposal = _lib.pmc_proposal_t(theta64=p(prop, "theta64"), u=p(prop, "u"), x=p(prop, "x"), logdetj=p(prop, "logdetj"),
                                   logl=p(prop, "logl"), logp=p(prop, "logp"), logdetj_flow=p(prop, "logdetj_flow"),
                                   quad=p(prop, "quad"), quad_prop=p(prop, "quad_prop"))
    uni = up(case["uniform"])
    r = _lib.pmc_rng_t(gamma=None, normal=None, uniform=uni.data_ptr(), seed=SEED, step=STEP, offset=0)
    alpha, acc, sums = Guarded(n), Guarded(n, dtype=np.int32), Guarded(D + 4)
    ws = torch.zeros(int(lib.pmc_accept_workspace_bytes(n, D)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.pmc_accept(0 if case["tpcn"] else 1, int(pre), C.byref(state), C.byref(proposal), case["beta"], case["nu"],
                              C.byref(r), alpha.ptr, acc.ptr, sums.ptr, _lib.ptr(ws), n, D, st), "pmc_accept")
    torch.cuda.synchronize()
    return dict(alpha=alpha.get(), accept=acc.get(), sums=sums.get(), post={k: v.cpu().numpy() for k, v in cur.items()})


def run_accept_width(D):
    worst = 0.0
    for pre, tpcn in ((1, 1), (1, 0), (0, 1), (0, 0)):
        for n in sw.accept_rows(D):
            case = sw.accept_case(D, n, pre, tpcn)
            assert sw.accept_knife_edges(case) == 0
            got = accept(case)
            tag = (D, n, pre, tpcn)
            np.testing.assert_allclose(got["alpha"], case["alpha"], rtol=1e-9, atol=1e-300, err_msg=str(tag))
            assert (got["alpha"][case["neg"] | case["nan"]] == 0.0).all(), tag
            want_acc, want_post = sw.accept_post_state(case)
            assert np.array_equal(got["accept"], want_acc.astype(np.int32)), tag
            assert set(got["post"]) == set(want_post)
            for k, v in want_post.items():
                assert same_bits(got["post"][k], v), (tag, k)
            sums = got["sums"]
            assert sums[3] == want_acc.sum(), tag
            for j, t in sw.accept_sum_terms(case, got["alpha"], got["post"]).items():
                exact, bound = sw.fsum_and_bound(t)
                err = abs(float(sums[j]) - exact)
                assert err <= bound, (tag, j, err, bound)
                if bound > 0.0:
                    worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("D", sw.ACCEPT_D)
def test_accept_in_every_width_class(D):
    worst = run_accept_width(D)
    print(f"pmc_accept D = {D} (S = {max(1, 256 // min(256, D + 4))}, {1 + (D + 4 > 256)} column pass(es)): "
          f"worst sum error / bound {worst:.3g}")


# ----------------------------------------------------------------------------------------------------------------------
# 4. the oracle's step with all three kernels on their wide paths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pcn", "rwm"])
def test_unfused_step_above_128_follows_the_oracle(kind):
    from test_gpu_mcmc import teacher_forced
    teacher_forced(f"{kind}_d130", case=dict(kind=kind, N=80, D=130, T=3, beta=0.5, nu=5.0, prior="mixed", target="gauss",
                                             seed=300, n_max=2))
