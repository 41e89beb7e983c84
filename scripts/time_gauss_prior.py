"""What a correlated normal prior (pocomc_amd.GaussianPrior as a block of a pocomc_amd.JointPrior) costs next to the same prior
written as a ``DevicePrior`` in torch: 1e4 walkers x 32 dimensions, a 24-dimensional normal block on interleaved columns and
uniform factors on the other 8.

    python scripts/time_gauss_prior.py [--walkers 10000] [--dim 32] [--gauss-dim 24] [--steps 200] [--repeats 3] [--calls 200]
                                       [--flows maf3,nsf6] [--out profiles/gauss_prior.txt]

The two priors compute the same density:
  * ``gauss``:  ``JointPrior([GaussianPrior(mean, cov)], [columns], Prior(uniform factors)).logpdf_device`` -- one launch
                (``pmc_gauss_blocks_logpdf``), one pass over x;
  * ``torch``:  a ``DevicePrior`` whose function gathers the block's columns, subtracts the mean, multiplies by the transposed
                inverse Cholesky factor (a matmul), squares, sums the rows, and restates the uniform factors.
Measured:
  * microseconds per ``logpdf_device`` call on the MCMC step's column-major view and on a C-contiguous block: device events
    around --calls calls in a row, median of --repeats windows;
  * per flow (the step's own flow over all 32 dimensions): steps per second of one preconditioned tpCN kernel call of --steps
    steps with the torch Rosenbrock on the device (``device_likelihood=True``), the prior inside the step
    (``device_logprior``) for both, next to the uniform(-10, 20)^32 ``Prior`` from the device's table: host clock around a
    synchronised call, the modes alternate, one warm-up call each, median of --repeats.
One JSON line; --out writes a readable table as well."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_joint_prior import event_us                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--gauss-dim", type=int, default=24)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--flows", default="maf3,nsf6")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from time_device_likelihood import rosenbrock_torch

    N, D, K = args.walkers, args.dim, args.gauss_dim
    Dr = D - K
    rng = np.random.default_rng(0)
    columns = rng.permutation(D)[:K]                                      # the block: interleaved, not sorted
    (cols,), rest_cols = pc.JointPrior.layout_blocks([columns], [K], Dr)
    # a covariance with a random orthogonal basis and eigenvalues log-spaced over a condition number of 100, around 4
    Q, _ = np.linalg.qr(rng.normal(size=(K, K)))
    cov = (Q * (4.0 * np.logspace(0.5, -1.5, K))) @ Q.T
    cov = 0.5 * (cov + cov.T)
    mean = rng.normal(size=K) * 0.5
    planck = pc.GaussianPrior(mean, cov)
    own = pc.Prior([uniform(-10.0, 20.0)] * Dr)
    gauss = pc.JointPrior([planck], [cols.tolist()], own)
    table = pc.Prior([uniform(-10, 20)] * D)

    blk = planck.device_block()
    LinvT = torch.from_numpy(np.linalg.inv(np.linalg.cholesky(cov)).T.copy()).cuda()
    mean_t = torch.from_numpy(blk["mean"]).cuda()
    logc = float(blk["logc"])
    ci, ri = torch.from_numpy(cols).long().cuda(), torch.from_numpy(rest_cols).long().cuda()
    log_w = -Dr * math.log(20.0)

    def torch_device(t):
        y = (t[:, ci] - mean_t) @ LinvT
        g = -0.5 * (y * y).sum(dim=1) - logc
        r = t[:, ri]
        inside = ((r >= -10.0) & (r <= 10.0)).all(dim=1)
        return torch.where(inside, g + log_w, torch.full_like(g, -math.inf))
    composed = pc.DevicePrior(torch_device, gauss.bounds, gauss.rvs)

    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))                          # (the scaler's standardisation: the walkers' region)
    xt = torch.from_numpy(x).cuda()
    colmajor = xt.t().contiguous().t()
    a, b = gauss.logpdf_device(xt), composed.logpdf_device(xt)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, gauss.logpdf_device(colmajor))
    assert float((a - b).abs().max()) <= 1e-9 * float(a.abs().max())      # the same density
    out = dict(walkers=N, dim=D, gauss_dim=K, rest_dim=Dr, steps=args.steps, repeats=args.repeats, calls=args.calls,
               kind="preconditioned_pcn", gpu=torch.cuda.get_device_name(0), flows={})
    for who, prior in (("gauss", gauss), ("torch", composed)):
        for lay, t in (("colmajor", colmajor), ("contiguous", xt)):
            key = f"{who}_{lay}_us"
            out[key], out[key + "_all"] = event_us(lambda: prior.logpdf_device(t), args.calls, args.repeats)
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    for name in args.flows.split(","):
        # the step: all D dimensions under the Sampler's own scaler and flow
        scaler = pc.Reparameterize(D, bounds=gauss.bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(D, name, seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        modes = dict(gauss=(gauss.logpdf_device, dict(device_logprior=True), gauss.logpdf(x)),
                     torch=(composed.logpdf_device, dict(device_logprior=True), composed.logpdf(x)),
                     uniform_table=(table.logpdf, {}, table.logpdf(x)))

        def call(mode):
            logprior, extra, logp0 = modes[mode]
            state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=logp0.copy(), beta=0.5,
                         blobs=None)
            funcs = dict(loglike=like, logprior=logprior, scaler=scaler, flow=flow, theta_geometry=geo)
            opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                        device_likelihood=True, **extra)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pmcmc.preconditioned_pcn(state, funcs, opts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res["steps"] == args.steps
            return res["steps"] / dt, res
        last = {m: call(m)[1] for m in modes}                             # warm-up
        rates = {m: [] for m in modes}
        for _ in range(args.repeats):                                     # the modes alternate
            for m in modes:
                r, last[m] = call(m)
                rates[m].append(r)
        row = {}
        for m, rs in rates.items():
            row[m] = dict(steps_per_s_median=float(np.median(rs)), us_per_step_median=1e6 / float(np.median(rs)), all=rs,
                          accept=float(last[m]["accept"]), calls=int(last[m]["calls"]))
            assert np.isfinite(last[m]["logp"]).all()
        row["gauss_over_torch"] = row["gauss"]["steps_per_s_median"] / row["torch"]["steps_per_s_median"]
        row["gauss_over_uniform_table"] = row["gauss"]["steps_per_s_median"] / row["uniform_table"]["steps_per_s_median"]
        out["flows"][name] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_gauss_prior.py --walkers {N} --dim {D} --gauss-dim {K} --steps {args.steps} "
                    f"--repeats {args.repeats} --calls {args.calls}   ({out['gpu']})\n")
            f.write(f"{D} columns: a {K}-dimensional normal block on interleaved columns (condition number 100), {Dr} uniform factors\n")
            f.write("medians of the repeats; us per call from device events, steps/s from a host clock around a synchronised call\n")
            f.write("gauss: JointPrior([GaussianPrior], ...).logpdf_device, one launch; torch: a DevicePrior with a gather, a "
                    "subtraction, a matmul, a square, a row sum and the factors restated in torch\n\n")
            f.write(f"{'one logpdf_device call':24s} {'col-major':>12s} {'C-contig.':>12s}\n")
            for who in ("gauss", "torch"):
                f.write(f"{who:24s} {out[who + '_colmajor_us']:9.1f} us {out[who + '_contiguous_us']:9.1f} us\n")
            f.write(f"\n{'flow':6s} {'step, gauss':>16s} {'step, torch':>16s} {'step, uniform table':>20s} {'gauss / torch':>14s} "
                    f"{'gauss / table':>14s}\n")
            for name, r in out["flows"].items():
                f.write(f"{name:6s} {r['gauss']['steps_per_s_median']:11.1f} st/s {r['torch']['steps_per_s_median']:11.1f} st/s "
                        f"{r['uniform_table']['steps_per_s_median']:15.1f} st/s {r['gauss_over_torch']:14.3f} "
                        f"{r['gauss_over_uniform_table']:14.3f}\n")
            f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
