"""What a mixture of correlated normals as a prior (pocomc_amd.GaussianMixturePrior as a block of a pocomc_amd.JointPrior) costs
next to the same prior written as a ``DevicePrior`` in torch, next to the one-component ``GaussianPrior`` of the same shape and
next to a ``FlowPrior`` on the same columns: 1e4 walkers x 32 dimensions, a 24-column mixture block of 8 components on
interleaved columns and uniform factors on the other 8.

    python scripts/time_gauss_mix_prior.py [--walkers 10000] [--dim 32] [--mix-dim 24] [--components 8] [--steps 200]
                                           [--repeats 5] [--calls 2000] [--flows maf3,nsf6] [--step-flow maf3]
                                           [--out profiles/gauss_mix_prior.txt]

The priors, all in one process:
  * ``mix``:    ``JointPrior([GaussianMixturePrior(weights, means, covs)], [columns], Prior(uniform factors)).logpdf_device`` --
                one launch (``pmc_gauss_mix_logpdf``), one pass over x;
  * ``torch``:  ``mix``'s density as a ``DevicePrior``: a gather, a batched product with the components' transposed inverse
                Cholesky factors, squares, row sums, ``torch.logsumexp``, the uniform factors restated;
  * ``gauss``:  the same joint with the one-component ``GaussianPrior`` (component 0) -- one launch (``pmc_gauss_blocks_logpdf``);
  * ``flow_<name>``: the same joint with a ``FlowPrior`` (an untrained flow of --flows on the block's columns);
  * ``mix_alone``: the 24-column mixture by itself on the block's own (n, 24) array.
Measured:
  * microseconds per ``logpdf_device`` call on the MCMC step's column-major view and on a C-contiguous block: device events
    around --calls calls in a row after ten warm-up calls; the priors alternate, --repeats windows each, median and all;
  * steps per second of one preconditioned tpCN kernel call of --steps steps with the torch Rosenbrock on the device
    (``device_likelihood=True``), the prior inside the step (``device_logprior``), the step's own flow --step-flow over all 32
    dimensions: host clock around a synchronised call, the modes alternate, one warm-up call each, median of --repeats.
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
    ap.add_argument("--mix-dim", type=int, default=24)
    ap.add_argument("--components", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--flows", default="maf3,nsf6")
    ap.add_argument("--step-flow", default="maf3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from time_device_likelihood import rosenbrock_torch

    N, D, K, Cn = args.walkers, args.dim, args.mix_dim, args.components
    Dr = D - K
    rng = np.random.default_rng(0)
    columns = rng.permutation(D)[:K]                                      # the block: interleaved, not sorted
    (cols,), rest_cols = pc.JointPrior.layout_blocks([columns], [K], Dr)
    # per component time_gauss_prior.py's covariance: a random orthogonal basis, eigenvalues log-spaced over a condition
    # number of 100; the means a unit apart, the weights uneven
    covs = []
    for _ in range(Cn):
        Q, _ = np.linalg.qr(rng.normal(size=(K, K)))
        cov = (Q * (4.0 * np.logspace(0.5, -1.5, K))) @ Q.T
        covs.append(0.5 * (cov + cov.T))
    covs = np.stack(covs)
    means = rng.normal(size=(Cn, K)) * 0.5
    weights = rng.uniform(0.2, 1.0, size=Cn)
    mixture = pc.GaussianMixturePrior(weights, means, covs)
    plain = pc.GaussianPrior(means[0], covs[0])
    own = pc.Prior([uniform(-10.0, 20.0)] * Dr)
    mix = pc.JointPrior([mixture], [cols.tolist()], own)
    gauss = pc.JointPrior([plain], [cols.tolist()], own)

    blk = mixture.device_block()
    LinvT = torch.from_numpy(np.stack([np.linalg.inv(np.linalg.cholesky(c)).T for c in covs])).cuda()      # (C, K, K)
    means_t, logc_t, logw_t = (torch.from_numpy(blk[f]).cuda() for f in ("mean", "logc", "logw"))
    ci, ri = torch.from_numpy(cols).long().cuda(), torch.from_numpy(rest_cols).long().cuda()
    log_w = -Dr * math.log(20.0)

    def torch_device(t):
        xb = t[:, ci]
        y = torch.bmm(xb[None, :, :] - means_t[:, None, :], LinvT)        # (C, n, K)
        tc = (-0.5 * (y * y).sum(dim=2) - logc_t[:, None]) + logw_t[:, None]
        v = torch.logsumexp(tc, dim=0)
        r = t[:, ri]
        inside = ((r >= -10.0) & (r <= 10.0)).all(dim=1)
        return torch.where(inside, v + log_w, torch.full_like(v, -math.inf))
    composed = pc.DevicePrior(torch_device, mix.bounds, mix.rvs)

    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))                          # (the scaler's standardisation: the walkers' region)
    xt = torch.from_numpy(x).cuda()
    colmajor = xt.t().contiguous().t()
    xb = xt[:, ci].contiguous()
    xb_colmajor = xb.t().contiguous().t()
    flows = {}
    for name in args.flows.split(","):
        block_scaler = pc.Reparameterize(K, bounds=np.array([[-10.0, 10.0]] * K))
        block_scaler.fit(xs[:, cols])
        flows[name] = pc.JointPrior([pc.FlowPrior(pc.Flow(K, name, seed=0), block_scaler)], [cols.tolist()], own)
    a, b = mix.logpdf_device(xt), composed.logpdf_device(xt)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, mix.logpdf_device(colmajor))
    assert float((a - b).abs().max()) <= 1e-9 * float(a.abs().max())      # the same density
    out = dict(walkers=N, dim=D, mix_dim=K, components=Cn, rest_dim=Dr, steps=args.steps, repeats=args.repeats,
               calls=args.calls, kind="preconditioned_pcn", step_flow=args.step_flow, gpu=torch.cuda.get_device_name(0))
    timed = {"mix": (mix, colmajor, xt), "torch": (composed, colmajor, xt), "gauss": (gauss, colmajor, xt)}
    for name, joint in flows.items():
        timed["flow_" + name] = (joint, colmajor, xt)
    timed["mix_alone"] = (mixture, xb_colmajor, xb)
    windows = {f"{who}_{lay}_us": [] for who in timed for lay in ("colmajor", "contiguous")}
    for _ in range(args.repeats):                                         # the priors alternate
        for who, (prior, cm, cc) in timed.items():
            for lay, t in (("colmajor", cm), ("contiguous", cc)):
                windows[f"{who}_{lay}_us"].append(event_us(lambda: prior.logpdf_device(t), args.calls, 1)[0])
    for key, w in windows.items():
        out[key], out[key + "_all"] = float(np.median(w)), w
    out["mix_not_slower_than_torch"] = bool(out["mix_colmajor_us"] <= out["torch_colmajor_us"]
                                            and out["mix_contiguous_us"] <= out["torch_contiguous_us"])
    # the step: all D dimensions under the Sampler's own scaler and flow (the mixture joint's bounds for every mode)
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    scaler = pc.Reparameterize(D, bounds=mix.bounds)
    scaler.fit(xs)
    u = scaler.forward(x)
    flow = pc.Flow(D, args.step_flow, seed=0)
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    modes = {who: (prior.logpdf_device, prior.logpdf(x)) for who, (prior, _, _) in timed.items() if who != "mix_alone"}

    def call(mode):
        logprior, logp0 = modes[mode]
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=logp0.copy(), beta=0.5,
                     blobs=None)
        funcs = dict(loglike=like, logprior=logprior, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                    device_likelihood=True, device_logprior=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res
    last = {m: call(m)[1] for m in modes}                                 # warm-up
    rates = {m: [] for m in modes}
    for _ in range(args.repeats):                                         # the modes alternate
        for m in modes:
            r, last[m] = call(m)
            rates[m].append(r)
    row = {}
    for m, rs in rates.items():
        row[m] = dict(steps_per_s_median=float(np.median(rs)), us_per_step_median=1e6 / float(np.median(rs)), all=rs,
                      accept=float(last[m]["accept"]), calls=int(last[m]["calls"]))
        assert np.isfinite(last[m]["logp"]).all()
    for m in modes:
        if m != "mix":
            row["mix_over_" + m] = row["mix"]["steps_per_s_median"] / row[m]["steps_per_s_median"]
    out["step"] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_gauss_mix_prior.py --walkers {N} --dim {D} --mix-dim {K} --components {Cn} --steps {args.steps} "
                    f"--repeats {args.repeats} --calls {args.calls} --step-flow {args.step_flow}   ({out['gpu']})\n")
            f.write(f"{D} columns: a {K}-column mixture block of {Cn} components on interleaved columns (condition number 100 "
                    f"each), {Dr} uniform factors\n")
            f.write("medians of the repeats (all windows in the JSON line); us per call from device events around --calls calls, "
                    "the priors alternating; steps/s from a host clock around a synchronised call\n")
            f.write("mix: JointPrior([GaussianMixturePrior], ...), one launch; torch: mix's density as a DevicePrior; gauss: "
                    "JointPrior([GaussianPrior], ...), one component, one launch; flow_*: JointPrior([FlowPrior], ...); mix_alone: "
                    "the mixture by itself on its own columns\n\n")
            f.write(f"{'one logpdf_device call':24s} {'col-major':>12s} {'min .. max':>18s} {'C-contig.':>12s} {'min .. max':>18s}\n")
            for who in timed:
                cm, cc = out[who + "_colmajor_us_all"], out[who + "_contiguous_us_all"]
                f.write(f"{who:24s} {out[who + '_colmajor_us']:9.2f} us {min(cm):8.2f} .. {max(cm):6.2f} "
                        f"{out[who + '_contiguous_us']:9.2f} us {min(cc):8.2f} .. {max(cc):6.2f}\n")
            f.write(f"the hand kernel's call is {'not slower' if out['mix_not_slower_than_torch'] else 'SLOWER'} than the torch "
                    "statement in both layouts\n")
            f.write(f"\n{args.steps}-step device-likelihood call, the step's flow {args.step_flow}\n")
            f.write(f"{'prior':24s} {'steps/s':>12s} {'min .. max':>20s} {'mix / this':>12s}\n")
            for m in modes:
                r = row[m]
                ratio = "" if m == "mix" else f"{row['mix_over_' + m]:12.3f}"
                f.write(f"{m:24s} {r['steps_per_s_median']:12.1f} {min(r['all']):9.1f} .. {max(r['all']):8.1f} {ratio}\n")
            f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
