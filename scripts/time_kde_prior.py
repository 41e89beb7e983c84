"""What a kernel density estimate as a prior (pocomc_amd.KDEPrior as a block of a pocomc_amd.JointPrior) costs next to the same
prior written as a ``DevicePrior`` in torch, next to a ``GaussianMixturePrior`` fitted to the same samples and next to a
``FlowPrior`` on the same columns: 1e4 walkers x 32 dimensions, a 4-column KDE block on interleaved columns and uniform factors
on the other 28 (a ``JointPrior``'s table takes every column its blocks leave).

    python scripts/time_kde_prior.py [--walkers 10000] [--dim 32] [--kde-dim 4] [--samples 512,4096]
                                     [--steps 200] [--repeats 5] [--calls 300] [--flow nsf6] [--step-flow maf3]
                                     [--out profiles/kde_prior.txt]

The priors, per sample count M, all in one process:
  * ``kde``:    ``JointPrior([KDEPrior(samples)], [columns], Prior(uniform factors)).logpdf_device`` -- one launch
                (``pmc_kde_logpdf``), one pass over x;
  * ``torch``:  ``kde``'s density as a ``DevicePrior``: a gather, the whitening product, ``torch.cdist`` squared against the
                whitened samples, ``torch.logsumexp``, the uniform factors restated;
  * ``gmix``:   the same joint with ``GaussianMixturePrior.from_samples(samples, n_components=8)`` (another density: what a user
                without the KDE would fit);
  * ``flow``:   the same joint with a ``FlowPrior`` (an untrained flow of --flow on the block's columns).
Measured as ``scripts/time_gauss_mix_prior.py`` measures: microseconds per ``logpdf_device`` call on the MCMC step's
column-major view and on a C-contiguous block (device events around --calls calls, the priors alternating, --repeats windows,
median and all), and steps per second of one preconditioned tpCN kernel call of --steps steps with the torch Rosenbrock on the
device and the prior inside the step.  One JSON line; --out writes a readable table as well."""
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


def banana(M, k, rng):
    """A banana in the first two columns, correlated normals behind them, inside (-2, 2) mostly."""
    z = rng.normal(size=(M, k))
    s = np.array(z) * 0.4
    s[:, 0] = 0.8 * z[:, 0]
    if k > 1:
        s[:, 1] = 0.2 * z[:, 1] + 0.6 * s[:, 0] ** 2 - 0.5
    for j in range(2, k):
        s[:, j] = 0.3 * z[:, j] + 0.4 * s[:, j - 1]
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--kde-dim", type=int, default=4)
    ap.add_argument("--samples", default="512,4096")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--flow", default="nsf6")
    ap.add_argument("--step-flow", default="maf3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from time_device_likelihood import rosenbrock_torch

    N, D, K = args.walkers, args.dim, args.kde_dim
    Dr = Dj = D - K
    Dj = D
    rng = np.random.default_rng(0)
    jcols = rng.permutation(D)[:K]                                        # the block: interleaved, not sorted
    own = pc.Prior([uniform(-10.0, 20.0)] * Dr)
    log_w = -Dr * math.log(20.0)
    x = rng.uniform(-2.0, 2.0, size=(N, Dj))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, Dj))
    xt = torch.from_numpy(x).cuda()
    colmajor = xt.t().contiguous().t()
    out = dict(walkers=N, dim=D, joint_dim=Dj, kde_dim=K, rest_dim=Dr, steps=args.steps, repeats=args.repeats, calls=args.calls,
               kind="preconditioned_pcn", step_flow=args.step_flow, flow=args.flow, gpu=torch.cuda.get_device_name(0), runs={})
    block_scaler = pc.Reparameterize(K, bounds=np.array([[-10.0, 10.0]] * K))
    block_scaler.fit(xs[:, jcols])
    flow_joint = pc.JointPrior([pc.FlowPrior(pc.Flow(K, args.flow, seed=0), block_scaler)], [jcols.tolist()], own)
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    for M in [int(m) for m in args.samples.split(",")]:
        samples = banana(M, K, np.random.default_rng(M))
        kde_block = pc.KDEPrior(samples)
        kde = pc.JointPrior([kde_block], [jcols.tolist()], own)
        try:
            gmix = pc.JointPrior([pc.GaussianMixturePrior.from_samples(samples, n_components=8)], [jcols.tolist()], own)
        except ValueError as e:
            gmix, out.setdefault("gmix_refused", {})[str(M)] = None, str(e)
        blk = kde_block.device_block()
        Linv = np.zeros((K, K))
        Linv[np.tril_indices(K)] = blk["linv_packed"]
        LinvT, center, tt, logw = (torch.from_numpy(np.ascontiguousarray(a)).cuda()
                                   for a in (Linv.T, blk["center"], blk["t"], blk["logw"]))
        logc = float(blk["logc"])
        ci = torch.from_numpy(jcols).long().cuda()
        ri = torch.from_numpy(np.setdiff1d(np.arange(Dj), jcols)).long().cuda()

        def torch_device(t):
            y = (t[:, ci] - center) @ LinvT
            e = -0.5 * torch.cdist(y, tt) ** 2 + logw
            v = torch.logsumexp(e, dim=1) - logc
            r = t[:, ri]
            inside = ((r >= -10.0) & (r <= 10.0)).all(dim=1)
            return torch.where(inside, v + log_w, torch.full_like(v, -math.inf))
        composed = pc.DevicePrior(torch_device, kde.bounds, kde.rvs)
        a, b = kde.logpdf_device(xt), composed.logpdf_device(xt)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, kde.logpdf_device(colmajor))
        run = dict(torch_max_abs_difference=float((a - b).abs().max()))   # (cdist's |y|^2 + |t|^2 - 2 y.t cancels: reported)
        timed = {"kde": kde, "torch": composed, "flow": flow_joint}
        if gmix is not None:
            timed["gmix"] = gmix
        windows = {f"{who}_{lay}_us": [] for who in timed for lay in ("colmajor", "contiguous")}
        for _ in range(args.repeats):                                     # the priors alternate
            for who, prior in timed.items():
                for lay, t in (("colmajor", colmajor), ("contiguous", xt)):
                    windows[f"{who}_{lay}_us"].append(event_us(lambda: prior.logpdf_device(t), args.calls, 1)[0])
        for key, w in windows.items():
            run[key], run[key + "_all"] = float(np.median(w)), w
        # the step: all columns under the Sampler's own scaler and flow
        scaler = pc.Reparameterize(Dj, bounds=kde.bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(Dj, args.step_flow, seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        modes = {who: (prior.logpdf_device, prior.logpdf(x)) for who, prior in timed.items()}

        def call(mode):
            logprior, logp0 = modes[mode]
            state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=logp0.copy(), beta=0.5,
                         blobs=None)
            funcs = dict(loglike=like, logprior=logprior, scaler=scaler, flow=flow, theta_geometry=geo)
            opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / Dj ** 0.5, seed=3,
                        device_likelihood=True, device_logprior=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pmcmc.preconditioned_pcn(state, funcs, opts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res["steps"] == args.steps
            return res["steps"] / dt
        for m in modes:
            call(m)                                                       # warm-up
        rates = {m: [] for m in modes}
        for _ in range(args.repeats):                                     # the modes alternate
            for m in modes:
                rates[m].append(call(m))
        run["step"] = {m: dict(steps_per_s_median=float(np.median(rs)), all=rs) for m, rs in rates.items()}
        out["runs"][str(M)] = run
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_kde_prior.py --walkers {N} --dim {D} --kde-dim {K} --samples {args.samples} "
                    f"--steps {args.steps} --repeats {args.repeats} --calls {args.calls} --flow {args.flow} "
                    f"--step-flow {args.step_flow}   ({out['gpu']})\n")
            f.write(f"{Dj} columns: a {K}-column KDE block on interleaved columns, {Dr} uniform factors; medians of the repeats "
                    "(all windows in the JSON line); us per call from device events around --calls calls, the priors "
                    "alternating; steps/s from a host clock around a synchronised call\n")
            f.write("kde: JointPrior([KDEPrior], ...), one launch; torch: kde's density as a DevicePrior (cdist, logsumexp); gmix: "
                    "JointPrior([GaussianMixturePrior.from_samples(n_components=8)], ...); flow: JointPrior([FlowPrior], ...)\n")
            for M, run in out["runs"].items():
                f.write(f"\nM = {M} samples   (torch's value differs from the kernel's by at most {run['torch_max_abs_difference']:.2e})\n")
                f.write(f"{'one logpdf_device call':24s} {'col-major':>12s} {'min .. max':>20s} {'C-contig.':>12s} {'min .. max':>20s}\n")
                for who in run["step"]:
                    cm, cc = run[who + "_colmajor_us_all"], run[who + "_contiguous_us_all"]
                    f.write(f"{who:24s} {run[who + '_colmajor_us']:9.2f} us {min(cm):9.2f} .. {max(cm):7.2f} "
                            f"{run[who + '_contiguous_us']:9.2f} us {min(cc):9.2f} .. {max(cc):7.2f}\n")
                f.write(f"{args.steps}-step device-likelihood call, the step's flow {args.step_flow}\n")
                f.write(f"{'prior':24s} {'steps/s':>12s} {'min .. max':>20s}\n")
                for m, r in run["step"].items():
                    f.write(f"{m:24s} {r['steps_per_s_median']:12.1f} {min(r['all']):9.1f} .. {max(r['all']):8.1f}\n")
            f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
