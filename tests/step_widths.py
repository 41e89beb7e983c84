"""Inputs, references and bounds for the width classes of the MCMC step's three kernels (``pmc_propose``,
``pmc_scaler_inverse[_prior]``, ``pmc_accept``).  Pure numpy: ``test_step_widths_cpu.py`` shows that the references and
bounds are sound without a GPU, ``test_gpu_step_widths.py`` holds the kernels to them.

The width lists are the edges of the kernels' own classes:

* proposal: f64-MFMA instances M = 4 / 8 / 16 / 32 for D <= 16 / 32 / 64 / 128 (``csrc/propose_body.h``), the LDS-staged
  VALU kernel for 128 < D <= 157 (``csrc/mcmc_kernels.hip``: 2 * D * 65 * 8 bytes of LDS, 160 KiB at most);
* scaler: numpy's pairwise sum has a leaf of <= 128 terms (8 accumulators + tail) and halves above (first half rounded down
  to a multiple of 8); 64 * D * 8 + 256 bytes of LDS (D <= 319), plus D * 65 * 8 with ``x_colmajor`` or a fused prior
  (D <= 158);
* accept: columns in chunks of 32; the fold of the W = D + 4 per-block partials has S = 256 // W threads per column and
  16 blocks in flight per thread; W > 256 takes a second pass over the columns.
"""
import math

import numpy as np

PROPOSE_D = (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 130, 157)
PROPOSE_D_MAX = 157                     # 2 * 158 * 65 * 8 > 160 KiB
ROWS = (1, 15, 16, 17, 63, 64, 65, 81)  # tile edges of the 16-walker MFMA wave and of the 64-row VALU block
ROWS_D = (17, 65, 129)                  # the widths at which every n of ROWS runs; n = 81 elsewhere
CONDS = (1.0, 1e4)
NUS = (0.1, 5.0, 1e6)
SIGMA = 0.4
CN_A = (1.0 - SIGMA ** 2.0) ** 0.5      # include/pocomc_amd.h: evaluated by the caller as mcmc.py:85 does

SCALER_D = (1, 7, 8, 9, 16, 127, 128, 129, 130, 136, 137, 144, 157, 158, 200, 256, 257, 319)
SCALER_N = (1, 65, 130)
SCALER_D_MAX_PLAIN = 319                # 64 * 320 * 8 + 256 > 160 KiB
SCALER_D_MAX_KEEP_X = 158               # (64 + 65) * 159 * 8 + 256 > 160 KiB

ACCEPT_D = (1, 28, 29, 32, 33, 60, 61, 64, 65, 124, 125, 128, 129, 157, 252, 253, 300)

U = 2.0 ** -53                          # unit roundoff of float64
SAFETY = 2.0                            # every bound below is multiplied by it


def propose_rows(D):
    return ROWS if D in ROWS_D else (81,)


def accept_rows(D):
    ns = [1, 64, 65, 64 * 7 + 5]
    if D == 1:
        ns.append(64 * 817)             # 817 blocks: S = 51 threads per column, 16 in flight each -> a second round
    if D == 124:
        ns.append(64 * 33)              # S = 2: 33 blocks are a second round as well
    return tuple(ns)


# ----------------------------------------------------------------------------------------------------------------------
# extended precision: numpy.longdouble where it is wider than float64 (x87: 64-bit significand), mpmath otherwise
# ----------------------------------------------------------------------------------------------------------------------
if np.finfo(np.longdouble).eps < 2.0 ** -53:
    EXT_EPS = float(np.finfo(np.longdouble).eps)

    def ext(a):
        return np.asarray(a).astype(np.longdouble)

    def ext_sqrt(a):
        return np.sqrt(a)
else:                                                                        # pragma: no cover (platform dependent)
    import mpmath
    mpmath.mp.prec = 113
    EXT_EPS = 2.0 ** -112

    def ext(a):
        return np.vectorize(mpmath.mpf, otypes=[object])(np.asarray(a, dtype=np.float64))

    def ext_sqrt(a):
        return np.vectorize(mpmath.sqrt, otypes=[object])(a)


def f64(a):
    return np.asarray(a).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# 1. proposal
# ----------------------------------------------------------------------------------------------------------------------
def propose_case(D, n, cond, nu, seed):
    """Geometry and current rows of one proposal call: a covariance with a random orthogonal basis and eigenvalues
    log-spaced over ``cond``, ``mu ~ 3 N(0, 1)``, rows ``mu + L N(0, 1) {0.01, 1, 30}`` (scale per row) rounded to float32."""
    rng = np.random.default_rng([int(seed), int(D), int(n), int(round(math.log10(cond))), int(round(math.log10(nu) * 10)) + 100])
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    ev = cond ** np.linspace(-0.5, 0.5, D) if D > 1 else np.ones(1)
    cov = (Q * ev) @ Q.T
    cov = 0.5 * (cov + cov.T)
    inv_cov = (Q / ev) @ Q.T
    inv_cov = 0.5 * (inv_cov + inv_cov.T)
    chol = np.linalg.cholesky(cov)
    mu = 3.0 * rng.normal(size=D)
    row_scale = rng.choice([0.01, 1.0, 30.0], size=n)
    cur32 = (mu + (rng.normal(size=(n, D)) @ chol.T) * row_scale[:, None]).astype(np.float32)
    return dict(D=D, n=n, cond=cond, nu=float(nu), sigma=SIGMA, cn_a=CN_A, mu=mu, inv_cov=np.ascontiguousarray(inv_cov),
                chol=np.ascontiguousarray(chol), cur32=cur32, row_scale=row_scale)


def host_variates(case, seed=0):
    """Variates for the CPU checks (the GPU tests take the device's own, ``pmc_rng_fill``)."""
    rng = np.random.default_rng([int(seed), case["D"], case["n"]])
    z = rng.normal(size=(case["n"], case["D"]))
    g = rng.gamma(0.5 * (case["D"] + case["nu"]), size=case["n"])
    return z, g


def propose_reference(case, z, g, tpcn=True):
    """The proposal in extended precision (mcmc.py:77-85 / :251-253) on the given variates, and the first-order
    forward-error bounds of a float64 evaluation with any summation order (u = 2^-53, SAFETY included):

        |dq|        <= 2 (D + 2) u sum_ij |d_i| |S_ij| |d_j|
        rel(scale)  <= 0.5 |dq| / (nu + q) + 4 u
        |dtheta'_i| <= 3 u (|mu_i| + |a d_i|) + |scale| ((D + 4) u sum_j |L_ij z_j| + rel(scale) |(L z)_i|) + u |theta'_i|
        |dq'|       <= 2 (D + 2) u sum_ij |dp_i| |S_ij| |dp_j| + 2 sum_ij dtheta'_i |S_ij| |dp_j|,   dp widened by dtheta'

    RWM: scale = sigma exactly, mu = 0, a = 1, no quadratic forms."""
    D = case["D"]
    cur = ext(case["cur32"].astype(np.float64))
    L = ext(case["chol"])
    zz = ext(z)
    sigma = ext(np.float64(case["sigma"]))
    Lz = zz @ L.T
    absLz = f64(abs(zz) @ abs(L).T)
    out = {}
    if tpcn:
        mu, S, a, nu = ext(case["mu"]), ext(case["inv_cov"]), ext(np.float64(case["cn_a"])), ext(np.float64(case["nu"]))
        d = cur - mu
        q = ((d @ S.T) * d).sum(axis=1)
        absS = abs(S)
        dq = 2.0 * (D + 2) * U * f64(((abs(d) @ absS.T) * abs(d)).sum(axis=1))
        s = 1 / ((2 / (nu + q)) * ext(g))
        scale = sigma * ext_sqrt(s)
        rel_scale = 0.5 * dq / f64(nu + q) + 4.0 * U
        theta = mu + a * d + scale[:, None] * Lz
        dtheta = (3.0 * U * (np.abs(case["mu"])[None, :] + f64(abs(a * d)))
                  + f64(abs(scale))[:, None] * ((D + 4) * U * absLz + rel_scale[:, None] * f64(abs(Lz)))
                  + U * f64(abs(theta)))
        dp = theta - mu
        qp = ((dp @ S.T) * dp).sum(axis=1)
        wide = f64(abs(dp)) + dtheta
        aS = f64(absS)
        dqp = 2.0 * (D + 2) * U * ((wide @ aS.T) * wide).sum(axis=1) + 2.0 * ((dtheta @ aS.T) * wide).sum(axis=1)
        out.update(quad=q, quad_prop=qp, quad_bound=SAFETY * dq, quad_prop_bound=SAFETY * dqp, scale=scale)
    else:
        theta = cur + sigma * Lz
        dtheta = 3.0 * U * f64(abs(cur)) + case["sigma"] * (D + 4) * U * absLz + U * f64(abs(theta))
    out.update(theta=theta, theta_bound=SAFETY * dtheta)
    return out


def propose_float64(case, z, g, tpcn=True, reverse=False):
    """A plain float64 restatement with every D-term sum taken one term after the other, first to last or last to first."""
    D, n = case["D"], case["n"]
    order = range(D - 1, -1, -1) if reverse else range(D)
    cur = case["cur32"].astype(np.float64)

    def matvec(M, v):                        # out[:, i] = sum_j M[i, j] v[:, j]
        acc = np.zeros((n, D))
        for j in order:
            acc = acc + v[:, j:j + 1] * M[:, j][None, :]
        return acc

    def dot(a, b):
        acc = np.zeros(n)
        for i in order:
            acc = acc + a[:, i] * b[:, i]
        return acc

    Lz = matvec(case["chol"], z)
    if not tpcn:
        return dict(theta=cur + case["sigma"] * Lz)
    mu, S, nu = case["mu"], case["inv_cov"], case["nu"]
    d = cur - mu
    q = dot(d, matvec(S, d))
    s = 1.0 / ((2.0 / (nu + q)) * g)
    scale = case["sigma"] * np.sqrt(s)
    theta = (mu + case["cn_a"] * d) + scale[:, None] * Lz
    dp = theta - mu
    return dict(theta=theta, quad=q, quad_prop=dot(dp, matvec(S, dp)))


def propose_ratios(ref, got):
    """Worst ``|got - reference| / bound`` of theta', quad and quad_prop (the keys ``got`` has)."""
    out = {}
    for k, b in (("theta", "theta_bound"), ("quad", "quad_bound"), ("quad_prop", "quad_prop_bound")):
        if k in got and k in ref:
            err = f64(abs(ext(np.asarray(got[k], dtype=np.float64)) - ref[k]))
            out[k] = float(np.max(err / ref[b]))
    return out


def propose_bound_sizes(ref):
    """Worst bound relative to the value it bounds: the quadratic forms per row, theta' per row against its largest
    coordinate (a coordinate of theta' may cancel to nothing, the row does not)."""
    out = {"theta": float(np.max(ref["theta_bound"].max(axis=1) / f64(abs(ref["theta"])).max(axis=1)))}
    for k in ("quad", "quad_prop"):
        if k in ref:
            out[k] = float(np.max(ref[k + "_bound"] / f64(abs(ref[k]))))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# 2. scaler
# ----------------------------------------------------------------------------------------------------------------------
def sum_tree_case(D, n, seed=0):
    """Every coordinate half-bounded below at 0 (kind 1), scale = 1: the Jacobian term is t = mu + sigma u, two float64
    roundings, and the row's logdetj is ``sum_log_sigma + np.sum(t_row)`` -- numpy's pairwise sum, bit for bit.  u has terms
    of very different size so that another association of the sum shows; |t| stays far below exp's overflow."""
    rng = np.random.default_rng([int(seed), int(D), int(n), 1])
    mu = rng.uniform(-1.0, 1.0, size=D)
    sigma = rng.uniform(0.25, 1.0, size=D)
    u = np.clip(rng.normal(size=(n, D)) * np.exp(rng.normal(size=(n, D)) * 3.0), -500.0, 500.0)
    t = mu + sigma * u
    sum_log_sigma = float(np.sum(np.log(sigma)))
    logdetj = np.array([sum_log_sigma + np.sum(np.ascontiguousarray(t[r])) for r in range(n)])
    return dict(D=D, n=n, mu=mu, sigma=sigma, u=u, t=t, sum_log_sigma=sum_log_sigma, logdetj=logdetj,
                low=np.zeros(D), high=np.full(D, np.inf), kind=np.ones(D, dtype=np.int32), x=np.exp(t) + 0.0)


def sequential_sum(row):
    acc = np.float64(0.0)
    for v in row:
        acc = acc + v
    return acc


def numpy_pairwise(a):
    """numpy's pairwise sum of a contiguous float64 vector, restated (umath loops, PW_BLOCKSIZE = 128)."""
    n = len(a)
    if n < 8:
        return sequential_sum(a)
    if n <= 128:
        r = [np.float64(a[i]) for i in range(8)]
        n8 = n - n % 8
        for i in range(8, n8, 8):
            for k in range(8):
                r[k] = r[k] + a[i + k]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(n8, n):
            res = res + a[i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return numpy_pairwise(a[:n2]) + numpy_pairwise(a[n2:])


def mixed_bounds(D):
    """Coordinate kinds cycle through 0, 1, 2, 3 (none / low / high / both)."""
    return np.array([[(-np.inf, np.inf), (0.0, np.inf), (-np.inf, 2.0), (-1.0, 3.0)][j % 4] for j in range(D)], dtype=float)


def mixed_bc(D):
    """Boundary conditions on two coordinates that have both bounds: periodic on 3, reflective on 7."""
    return ([3] if D > 3 else None), ([7] if D > 7 else None)


def mixed_samples(D, n, rng):
    x = np.empty((n, D))
    for j in range(D):
        k = j % 4
        x[:, j] = (rng.normal(0.7, 1.0, n) if k == 0 else rng.gamma(2.0, 0.7, n) if k == 1
                   else 2.0 - rng.gamma(2.0, 0.7, n) if k == 2 else rng.uniform(-1.0, 3.0, n))
    return x


def plan_prior(D):
    """(family, loc, scale) of a uniform / normal prior for the fused-prior plan: coordinate 0 is a uniform that about half
    of the rows of ``plan_u`` miss (logp = -inf), the others alternate wide uniforms and normals."""
    family = np.array([1 if j % 2 == 0 else 2 for j in range(D)], dtype=np.int32)
    loc = np.where(family == 1, -1e3, 0.5)
    scale = np.where(family == 1, 2e3, 2.0)
    loc[0], scale[0] = -0.5, 1.2
    return family, loc, scale


# ----------------------------------------------------------------------------------------------------------------------
# 3. accept
# ----------------------------------------------------------------------------------------------------------------------
BETA, ACCEPT_NU = 0.7, 5.0


def _wide(rng, size):
    """Random values of magnitude 0.1 .. 1e3, either sign."""
    return rng.choice([-1.0, 1.0], size=size) * 10.0 ** rng.uniform(-1.0, 3.0, size=size)


def accept_case(D, n, pre, tpcn, seed=0):
    """Synthetic current and proposed states of ``n`` walkers.  One row in eight has logl' = -inf (alpha = 0), one in sixteen
    an inf - inf exponent (logl' = -inf, logdetj' = +inf: NaN, alpha = 0); of the others half have an exponent of order one
    and half one of order 1e3.  The uniforms are redrawn wherever they came within 1e-6 alpha of alpha."""
    rng = np.random.default_rng([int(seed), int(D), int(n), int(pre), int(tpcn)])
    cur = dict(u=rng.normal(size=(n, D)) * 3.0, x=rng.normal(size=(n, D)) * 3.0, logdetj=_wide(rng, n), logl=_wide(rng, n),
               logp=_wide(rng, n))
    near = rng.random(n) < 0.5
    step = lambda: np.where(near, rng.normal(size=n), rng.normal(size=n) * 300.0)
    prop = dict(u=rng.normal(size=(n, D)) * 3.0, x=rng.normal(size=(n, D)) * 3.0, logdetj=cur["logdetj"] + step(),
                logl=cur["logl"] + step(), logp=cur["logp"] + step())
    if pre:
        cur["theta32"] = (rng.normal(size=(n, D)) * 3.0).astype(np.float32)
        cur["logdetj_flow"] = _wide(rng, n).astype(np.float32)
        prop["theta64"] = rng.normal(size=(n, D)) * 3.0
        prop["logdetj_flow"] = (cur["logdetj_flow"] + step()).astype(np.float32)
    if tpcn:
        prop["quad"] = D * np.exp(rng.normal(size=n))
        prop["quad_prop"] = prop["quad"] * np.exp(rng.normal(size=n) * np.where(near, 0.1, 1.0))
    k = np.arange(n)
    neg = k % 8 == 3
    nan = k % 16 == 5
    prop["logl"][neg | nan] = -np.inf
    prop["logdetj"][nan] = np.inf
    case = dict(D=D, n=n, pre=bool(pre), tpcn=bool(tpcn), beta=BETA, nu=ACCEPT_NU, cur=cur, prop=prop, neg=neg, nan=nan)
    alpha = accept_alpha(case)
    uni = rng.random(n)
    for _ in range(64):
        close = np.abs(uni - alpha) <= 1e-6 * alpha
        close &= alpha > 0.0
        if not close.any():
            break
        uni[close] = rng.random(int(close.sum()))
    case["uniform"] = uni
    case["alpha"] = alpha
    return case


def accept_alpha(case):
    """mcmc.py:124-134 left to right in float64 (the variants without the flow / without the Student-t terms alike)."""
    c, p, beta, nu, D = case["cur"], case["prop"], case["beta"], case["nu"], case["D"]
    with np.errstate(all="ignore"):
        e = p["logl"] * beta - c["logl"] * beta + p["logp"] - c["logp"] + p["logdetj"] - c["logdetj"]
        if case["pre"]:
            e = e + p["logdetj_flow"].astype(np.float64) - c["logdetj_flow"].astype(np.float64)
        if case["tpcn"]:
            A = -(D + nu) / 2 * np.log(1 + p["quad_prop"] / nu)
            B = -(D + nu) / 2 * np.log(1 + p["quad"] / nu)
            e = e - A + B
        alpha = np.minimum(np.ones(case["n"]), np.exp(e))
    alpha[np.isnan(alpha)] = 0.0
    return alpha


def accept_knife_edges(case):
    """Rows whose decision depends on the last bits of exp: |u - alpha| <= 1e-6 alpha."""
    a = case["alpha"]
    return int(((np.abs(case["uniform"] - a) <= 1e-6 * a) & (a > 0.0)).sum())


def accept_post_state(case):
    """The state arrays after the accept: the proposal on accepted rows, the previous state elsewhere."""
    acc = case["uniform"] < case["alpha"]
    c, p = case["cur"], case["prop"]
    post = {k: np.where(acc[:, None] if c[k].ndim == 2 else acc, p[k], c[k]) for k in ("u", "x", "logdetj", "logl", "logp")}
    if case["pre"]:
        post["theta32"] = np.where(acc[:, None], p["theta64"].astype(np.float32), c["theta32"])
        post["logdetj_flow"] = np.where(acc, p["logdetj_flow"], c["logdetj_flow"])
    return acc, post


def accept_sum_terms(case, alpha, post):
    """The terms of sums[0 .. D + 4) other than the count, from the device's own alpha and post state: list of 1-D arrays."""
    lp = post["logl"] + post["logp"]
    moved = post["theta32"].astype(np.float64) if case["pre"] else post["u"]
    return {0: alpha, 1: lp, 2: lp + post["logdetj"], **{4 + j: moved[:, j] for j in range(case["D"])}}


def fsum_and_bound(terms):
    """(exact sum, n u sum |terms|): any float64 summation order of n terms is within the bound (first order)."""
    t = np.asarray(terms, dtype=np.float64)
    return math.fsum(t.tolist()), len(t) * U * math.fsum(np.abs(t).tolist())
