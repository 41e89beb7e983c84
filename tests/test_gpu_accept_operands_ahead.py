"""``pmc_step_post`` on prepared device inputs against the float64 restatement of ``mcmc.py:124-156`` (the accept formula of
``oracle/mcmc.py``, the updates of ``Adaptation.update``): the decisions, the moved rows bit for bit, the sums, their host
copy with the other row ranges' sums added, the adapted sigma / mu, and the ticket word back at zero (a second call on
the same workspace gives the same result).  Written for a variant of ``accept_kernel`` (``csrc/mcmc_kernels.hip``) that
requested the row move's operands ahead of the decisions and the last block's operands ahead of its fold (DESIGN.md
appendix A, A1: not faster, taken out); it holds any order of those requests to the same results.

n in {1, 63, 64, 65, 193} (a partly filled block, more than one block, the last block's fold over several partials);
D in {1, 32, 33, 70} (33 and 70 reach the second 32-column chunk, 70 a width W = D + 4 > 64); one and two row ranges
(``adapt_n_other`` 0 and 1); tpCN and RWM adaptation, with and without the flow's theta; every row accepted, no row
accepted, and a mixture with NaN / -inf logl' and -inf logp'."""
import ctypes as C

import numpy as np
import pytest

NS = (1, 63, 64, 65, 193)
DS = (1, 32, 33, 70)
BETA, NU = 0.37, 3.5
STEP = 4
N_TOTAL_EXTRA = 100            # rows of the other range
ADAPT_TPCN, ADAPT_RWM, ADAPT_MU = 1, 3, 8          # include/pocomc_amd.h


def _case(n, D, pre, tpcn, regime, seed):
    rng = np.random.default_rng([seed, n, D, int(pre), int(tpcn)])
    cur = dict(u=rng.normal(size=(n, D)) * 3.0, x=rng.normal(size=(n, D)) * 3.0, logdetj=rng.normal(size=n) * 5.0,
               logl=rng.normal(size=n) * 20.0, logp=rng.normal(size=n) * 5.0)
    d = lambda s: rng.normal(size=n) * s
    prop = dict(u=rng.normal(size=(n, D)) * 3.0, x=rng.normal(size=(n, D)) * 3.0, logdetj=cur["logdetj"] + d(0.5),
                logl=cur["logl"] + d(2.0), logp=cur["logp"] + d(0.5))
    if pre:
        cur["theta32"] = (rng.normal(size=(n, D)) * 3.0).astype(np.float32)
        cur["logdetj_flow"] = (rng.normal(size=n) * 5.0).astype(np.float32)
        prop["theta64"] = rng.normal(size=(n, D)) * 3.0
        prop["logdetj_flow"] = (cur["logdetj_flow"] + d(0.5)).astype(np.float32)
    if tpcn:
        prop["quad"] = D * np.exp(rng.normal(size=n) * 0.3)
        prop["quad_prop"] = prop["quad"] * np.exp(rng.normal(size=n) * 0.1)
    uni = rng.random(n)
    k = np.arange(n)
    if regime == "all":
        prop["logl"] = cur["logl"] + 1e4                   # exp overflows: alpha = 1 > u
    elif regime == "none":
        prop["logl"] = cur["logl"] - 1e4                   # alpha = 0
    else:
        prop["logl"][k % 7 == 2] = np.nan                  # alpha = NaN -> 0 (mcmc.py:134)
        prop["logl"][k % 7 == 4] = -np.inf
        prop["logp"][k % 7 == 5] = -np.inf
    return dict(n=n, D=D, pre=pre, tpcn=tpcn, cur=cur, prop=prop, uniform=uni)


def _alpha(case):
    """mcmc.py:124-134, left to right in float64."""
    c, p, D = case["cur"], case["prop"], case["D"]
    with np.errstate(all="ignore"):
        e = p["logl"] * BETA - c["logl"] * BETA + p["logp"] - c["logp"] + p["logdetj"] - c["logdetj"]
        if case["pre"]:
            e = e + p["logdetj_flow"].astype(np.float64) - c["logdetj_flow"].astype(np.float64)
        if case["tpcn"]:
            A = -(D + NU) / 2 * np.log(1 + p["quad_prop"] / NU)
            B = -(D + NU) / 2 * np.log(1 + p["quad"] / NU)
            e = e - A + B
        alpha = np.minimum(np.ones(case["n"]), np.exp(e))
    alpha[np.isnan(alpha)] = 0.0
    return alpha


def _post(case, acc):
    c, p = case["cur"], case["prop"]
    post = {k: np.where(acc[:, None] if c[k].ndim == 2 else acc, p[k], c[k]) for k in ("u", "x", "logdetj", "logl", "logp")}
    if case["pre"]:
        post["theta32"] = np.where(acc[:, None], p["theta64"].astype(np.float32), c["theta32"])
        post["logdetj_flow"] = np.where(acc, p["logdetj_flow"], c["logdetj_flow"])
    return post


def _sums(case, alpha, post, acc):
    """sums[0 .. D + 4) of mcmc.py:152-156's means in float64 (math.fsum: the order does not enter), and the sums of the
    terms' magnitudes: a float64 sum in any order is within n u sum|terms| of the exact one, so "1e-12 relative" is taken
    of that magnitude (a column of theta may sum to nearly zero)."""
    import math
    lp = post["logl"] + post["logp"]
    moved = post["theta32"].astype(np.float64) if case["pre"] else post["u"]
    cols = [alpha, lp, lp + post["logdetj"], acc.astype(np.float64)] + [moved[:, j] for j in range(case["D"])]
    assert all(np.isfinite(c).all() for c in cols)
    return (np.array([math.fsum(c.tolist()) for c in cols]), np.array([math.fsum(np.abs(c).tolist()) for c in cols]))


def _adapt(state0, total, mode, c_sigma, c_mu, cap, n_total, D):
    """Adaptation.update's expressions (mcmc.py:152-156) on the total sums; and the magnitude of each word's operands, of
    which "1e-12 relative" is taken (mu + c (mean - mu) may cancel)."""
    mean_alpha = float(total[0]) / n_total
    sn = float(state0[0]) + c_sigma * (mean_alpha - 0.234)
    how = mode & 7
    if how == ADAPT_TPCN:
        sn = abs(min(sn, cap))
    elif how == ADAPT_RWM:
        sn = abs(sn)
    out = np.array(state0, dtype=np.float64)
    mag = np.maximum(np.abs(out), 1.0)
    out[0] = sn
    out[1] = (1.0 - sn * sn) ** 0.5 if how == ADAPT_TPCN else 0.0
    if mode & ADAPT_MU:
        mean_theta = (np.asarray(total[4:4 + D]) / n_total).astype(np.float32).astype(np.float64)
        out[2:2 + D] = state0[2:2 + D] + c_mu * (mean_theta - state0[2:2 + D])
        mag[2:2 + D] = np.maximum(mag[2:2 + D], np.abs(mean_theta))
    return out, mag


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _run(case, n_other, other_sums, mode, state0, twice=True):
    """pmc_step_post (host_direct: logl' / logp' read from pinned host memory, sums and the completion word written there)."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    n, D, pre, tpcn = case["n"], case["D"], case["pre"], case["tpcn"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    ws = torch.zeros(int(lib.pmc_accept_workspace_bytes(n, D)), dtype=torch.uint8, device="cuda")       # zeroed once
    cap = min(2.38 / D ** 0.5, 0.99)
    c_sigma, c_mu = 1 / (STEP + 2) ** 0.75, 1.0 / (STEP + 2.0)
    n_total = float(n + (N_TOTAL_EXTRA if n_other else 0))
    outs = []
    for call in range(2 if twice else 1):
        cur = {k: up(v) for k, v in case["cur"].items()}
        prop = {k: up(v) for k, v in case["prop"].items() if k not in ("logl", "logp")}
        h_logl, h_logp = pin(case["prop"]["logl"]), pin(case["prop"]["logp"])
        p_logl, p_logp = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        uni = up(case["uniform"])
        alpha = torch.empty(n, dtype=torch.float64, device="cuda")
        acc = torch.empty(n, dtype=torch.int32, device="cuda")
        sums = torch.full((D + 4,), -1.0, dtype=torch.float64, device="cuda")
        h_sums = pin(np.full(D + 4, -1.0))
        h_done = pin(np.zeros(2, dtype=np.int64))
        state = up(state0)
        other = up(other_sums) if n_other else None
        g = lambda d, k: d[k].data_ptr() if k in d else None
        s = _lib.pmc_step_t()
        s.kind, s.preconditioned, s.n, s.D = (0 if tpcn else 1), int(pre), n, D
        s.cur = _lib.pmc_state_t(theta32=g(cur, "theta32"), u=g(cur, "u"), x=g(cur, "x"), logdetj=g(cur, "logdetj"),
                                 logl=g(cur, "logl"), logp=g(cur, "logp"), logdetj_flow=g(cur, "logdetj_flow"))
        s.p_theta64, s.p_u, s.p_x, s.p_logdetj = g(prop, "theta64"), g(prop, "u"), g(prop, "x"), g(prop, "logdetj")
        s.p_ldjf, s.quad, s.p_quad = g(prop, "logdetj_flow"), g(prop, "quad"), g(prop, "quad_prop")
        s.p_logl, s.p_logp = p_logl.data_ptr(), p_logp.data_ptr()
        s.h_logl, s.h_logp, s.h_sums, s.h_done = h_logl.data_ptr(), h_logp.data_ptr(), h_sums.data_ptr(), h_done.data_ptr()
        s.alpha, s.accept, s.sums, s.ws = alpha.data_ptr(), acc.data_ptr(), sums.data_ptr(), ws.data_ptr()
        s.host_direct = 1
        s.adapt_state, s.adapt_mode = state.data_ptr(), mode
        s.adapt_c_sigma, s.adapt_c_mu, s.adapt_cap, s.adapt_n_total = c_sigma, c_mu, cap, n_total
        if n_other:
            s.adapt_other[0] = other.data_ptr()
        s.adapt_n_other = n_other
        r = _lib.pmc_rng_t(gamma=None, normal=None, uniform=uni.data_ptr(), seed=1, step=STEP, offset=0)
        _lib.check(lib.pmc_step_post(C.byref(s), C.byref(r), BETA, NU, 0, 1, _lib.stream_handle()), "pmc_step_post")
        torch.cuda.synchronize()
        outs.append(dict(alpha=alpha.cpu().numpy(), accept=acc.cpu().numpy(), sums=sums.cpu().numpy(),
                         h_sums=h_sums.numpy().copy(), done=h_done.numpy().copy(), state=state.cpu().numpy(),
                         ticket=int(ws[:4].cpu().numpy().view(np.uint32)[0]),
                         post={k: v.cpu().numpy() for k, v in cur.items()}))
    return outs, (c_sigma, c_mu, cap, n_total)


@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_step_post_equals_the_float64_restatement(n, D):
    seen = dict(acc=0, rej=0, nan=0)
    variants = [(1, 1, ADAPT_TPCN | ADAPT_MU), (0, 1, ADAPT_TPCN), (0, 0, ADAPT_RWM), (1, 0, ADAPT_RWM)]
    for vi, (pre, tpcn, mode) in enumerate(variants):
        for regime in ("all", "none", "mixed"):
            n_other = (vi + ("all", "none", "mixed").index(regime)) % 2          # one and two row ranges, in every variant
            case = _case(n, D, pre, tpcn, regime, seed=11)
            tag = (n, D, pre, tpcn, regime, n_other)
            rng = np.random.default_rng([5, n, D, vi])
            other = np.concatenate([[40.0, -900.0, -950.0, 37.0], rng.normal(size=D) * N_TOTAL_EXTRA])
            state0 = np.concatenate([[0.4, (1.0 - 0.4 ** 2.0) ** 0.5], rng.normal(size=D)])
            outs, (c_sigma, c_mu, cap, n_total) = _run(case, n_other, other, mode, state0)
            got = outs[0]
            # ---- decisions: u < alpha of the restatement wherever alpha is not within 1e-12 of u
            alpha = _alpha(case)
            sure = np.abs(alpha - case["uniform"]) > 1e-12
            want_acc = case["uniform"] < alpha
            assert np.array_equal(got["accept"][sure] != 0, want_acc[sure]), tag
            np.testing.assert_allclose(got["alpha"], alpha, rtol=1e-9, atol=1e-300, err_msg=str(tag))
            acc = got["accept"] != 0
            if regime == "all":
                assert acc.all(), tag
            if regime == "none":
                assert not acc.any(), tag
            if regime == "mixed":
                bad = ~np.isfinite(case["prop"]["logl"]) | ~np.isfinite(case["prop"]["logp"])
                assert not acc[bad].any() and (got["alpha"][bad] == 0.0).all(), tag
                seen["nan"] += int(np.isnan(case["prop"]["logl"]).sum())
            seen["acc"] += int(acc.sum())
            seen["rej"] += int((~acc).sum())
            # ---- accepted rows are bit copies of the proposal's, rejected rows untouched
            want = _post(case, acc)
            assert set(want) == set(got["post"])
            for k, v in want.items():
                assert np.array_equal(_bits(got["post"][k]), _bits(np.ascontiguousarray(v, dtype=got["post"][k].dtype))), (tag, k)
            # ---- sums, host copy, adapted state: 1e-12 relative of the restatement
            own, mag = _sums(case, got["alpha"], got["post"], acc)
            total, mag_total = (own + other, mag + np.abs(other)) if n_other else (own, mag)
            scale = lambda a: np.maximum(np.abs(a), 1e-300)
            assert (np.abs(got["sums"] - own) <= 1e-12 * scale(mag)).all(), (tag, got["sums"], own)
            assert (np.abs(got["h_sums"] - total) <= 1e-12 * scale(mag_total)).all(), (tag, got["h_sums"], total)
            assert got["sums"][3] == acc.sum(), tag
            want_state, mag_state = _adapt(state0, total, mode, c_sigma, c_mu, cap, n_total, D)
            assert (np.abs(got["state"] - want_state) <= 1e-12 * mag_state).all(), (tag, got["state"], want_state)
            if not (mode & ADAPT_MU):
                assert np.array_equal(_bits(got["state"][2:]), _bits(state0[2:])), tag
            assert got["done"][1] == STEP + 1 and got["done"][0] == 0, tag
            # ---- the ticket is back at zero: the second call on the same workspace gives the same result
            assert got["ticket"] == 0 and outs[1]["ticket"] == 0, tag
            for k in ("alpha", "accept", "sums", "h_sums", "state", "done"):
                assert np.array_equal(_bits(outs[1][k]), _bits(got[k])), (tag, k)
            for k in got["post"]:
                assert np.array_equal(_bits(outs[1]["post"][k]), _bits(got["post"][k])), (tag, k)
    assert seen["acc"] > 0 and seen["rej"] > 0 and (seen["nan"] > 0 or n < 3), seen
