"""The device likelihood on sharded walkers, one process per GPU (``option_dict["device_likelihood"]`` with a ``group``,
``Sampler(device_likelihood=True)`` with more than one rank): per step and rank  pre-step -> the user's GPU callable ->
accept of this rank's rows (no adaptation, no host copy of the sums) -> ONE exchange of the D + 4 sums, added in rank
order, with the sigma / mu update behind it -> the next pre-step -> one host wait.  A sharded device-likelihood call is the
sharded host-likelihood call bit for bit, whichever tier carried the sums, and the one-rank call up to the order of the sums.

The GPU box has one device: the ranks share it and talk over ``gloo``; what is rehearsed is the rank plumbing, the mailbox
exchange and the rank-ordered sums, not a link between two GPUs.  Every worker passes ``wait_timeout=60``: a rank that
loses its peer ends with an error instead of waiting."""
import os
import socket

import numpy as np
import pytest
import torch

from .test_gpu_device_likelihood import _assert_same, _call, _problem, device_like, f_torch, host_like
from .test_gpu_sharded_sampler import D as DS, ICOV, NORM, TRUE_LOGZ, _kernel_case

FIELDS = ("u", "x", "logl", "logp", "logdetj")
SCALARS = ("steps", "calls", "proposal_scale", "accept", "evaluations")
WAIT = 60


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# GPU nodes shared between users cap the processes that hold one device open; this suite keeps to PROCS_PER_GPU per
# device.  The ranks are placed on the devices round robin (all on device 0 of a one-GPU node), so device 0 holds the test
# process and ceil(world / GPUs) ranks.
PROCS_PER_GPU = 6


def _rank_device(rank):
    torch.cuda.set_device(rank % torch.cuda.device_count())


def skip_unless_gpus_for(world):
    n = max(torch.cuda.device_count(), 1)
    on_device0 = -(-world // n) + 1
    if on_device0 > PROCS_PER_GPU:
        need = -(-world // (PROCS_PER_GPU - 1))
        pytest.skip(f"needs {need} GPUs, found {n}: {world} ranks would put {on_device0} processes on one GPU "
                    f"(at most {PROCS_PER_GPU})")


def _init(rank, world, port, **env):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), **env)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _rank_device(rank)
    return dist


def _done(dist):
    from pocomc_amd import mcmc as pmcmc
    pmcmc.drop_comms()
    dist.barrier()
    dist.destroy_process_group()


def _shard(prob, rank, world):
    """This rank's rows of a problem (geometry, scaler and flow are those of the whole set: replicated) and their bounds."""
    prior, scaler, flow, geo, x, u = prob
    lo, hi = rank * len(x) // world, (rank + 1) * len(x) // world
    return (prior, scaler, flow, geo, x[lo:hi], u[lo:hi]), lo, hi


def _logl0(prob, f=f_torch):
    return f(torch.from_numpy(prob[4]).cuda()).cpu().numpy()


def _pack(store, tag, r):
    for k in FIELDS:
        store[f"{tag}/{k}"] = r[k]
    for k in SCALARS:
        store[f"{tag}/{k}"] = np.float64(r[k])


def _unpack(z, tag):
    out = {k: z[f"{tag}/{k}"] for k in FIELDS}
    out.update({k: float(z[f"{tag}/{k}"]) for k in SCALARS})
    return out


def _spawn(worker, world, out, *args):
    import torch.multiprocessing as mp
    mp.spawn(worker, args=(world, _free_port(), out) + args, nprocs=world, join=True)
    return [np.load(out % r) for r in range(world)]


# ------------------------------------------------------------------------------------------------------------------
# 1. sharded device call = sharded host call, bit for bit
# ------------------------------------------------------------------------------------------------------------------
FLOWS = [("maf3", 6), ("nsf3", 6), ("maf6", 50)]       # fused affine sweep, spline sweep, lane sweep + scaler launch
PRE = ["preconditioned_pcn", "preconditioned_rwm"]


def _kinds_of(flow_name):
    return PRE + (["pcn", "rwm"] if flow_name == "maf3" else [])          # (pcn / rwm use no flow: covered once)


def _host_device_worker(rank, world, port, out, flow_name, D):
    dist = _init(rank, world, port)
    part, lo, hi = _shard(_problem(D, 1024, flow_name, seed=D), rank, world)
    logl0 = _logl0(part)
    store = {}
    for kind in _kinds_of(flow_name):
        common = dict(group=None, shard_offset=lo, wait_timeout=WAIT)
        _pack(store, f"{kind}/host", _call(kind, part, host_like(f_torch), logl0, device=False, **common))
        _pack(store, f"{kind}/device", _call(kind, part, device_like(f_torch), logl0, device=True, **common))
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("flow_name,D", FLOWS)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_device_likelihood_call_equals_the_sharded_host_call_bit_for_bit(tmp_path, world, flow_name, D):
    """The one-rank contract of ``test_device_likelihood_call_equals_the_host_call_bit_for_bit`` carried to ranks: each
    rank's device-likelihood result against the same rank's host-likelihood result (the pipelined host call, same group,
    shard offset and seed).  No tolerance: both sides add the same per-rank sums in rank order."""
    skip_unless_gpus_for(world)
    rs = _spawn(_host_device_worker, world, str(tmp_path / "r%d.npz"), flow_name, D)
    n_local = 1024 // world
    for kind in _kinds_of(flow_name):
        calls = 0
        for z in rs:
            a, b = _unpack(z, f"{kind}/host"), _unpack(z, f"{kind}/device")
            _assert_same(a, b)
            assert b["steps"] == 8 and b["evaluations"] == 8 * n_local          # every step handed over all local rows
            assert b["proposal_scale"] == _unpack(rs[0], f"{kind}/device")["proposal_scale"]      # one sigma on all ranks
            calls += b["calls"]
        assert calls < 8 * 1024, (kind, calls)                                   # some proposals left the support
        print(f"{kind} {flow_name} world {world}: rows that reached the likelihood {int(calls)} of {8 * 1024}")


# ------------------------------------------------------------------------------------------------------------------
# 2. both exchange tiers give the same bits
# ------------------------------------------------------------------------------------------------------------------
def _tier_worker(rank, world, port, out, mailbox):
    dist = _init(rank, world, port, PMC_COMM_MAILBOX=mailbox)
    from pocomc_amd import mcmc as pmcmc
    store = {}
    for flag in ("1", "0"):
        os.environ["PMC_C_ALLREDUCE"] = flag              # (read again at every small_comm())
        for D in (6, 32):
            part, lo, hi = _shard(_problem(D, 1024, "maf3", seed=D), rank, world)
            r = _call("preconditioned_pcn", part, device_like(f_torch), _logl0(part), device=True, group=None,
                      shard_offset=lo, wait_timeout=WAIT)
            _pack(store, f"{flag}/{D}", r)
        store[f"{flag}/used"] = np.bool_(any(v[0] for v in pmcmc._COMMS.values()))
        store[f"{flag}/kinds"] = np.array(sorted({int(pmcmc._lib.load().pmc_comm_kind(v[0]))
                                                  for v in pmcmc._COMMS.values() if v[0]}), dtype=np.int64)
        pmcmc.drop_comms()
        assert not pmcmc._COMMS
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("mailbox", ["device", "host"])
@pytest.mark.parametrize("world", [2, 4])
def test_both_exchange_tiers_give_the_same_bits(tmp_path, world, mailbox):
    """``pmc_comm_adapt_update`` on device or host mailboxes (``PMC_C_ALLREDUCE=1``) against ``allreduce_sums`` +
    ``pmc_adapt_update`` through the process group (``=0``), D = 6 and 32: the assertions of
    ``test_the_sharded_step_behind_the_c_abi_equals_the_torch_distributed_path``."""
    skip_unless_gpus_for(world)
    rs = _spawn(_tier_worker, world, str(tmp_path / "t%d.npz"), mailbox)
    assert all(bool(z["1/used"]) for z in rs)                               # the communicator was created and connected
    assert all(z["1/kinds"].tolist() == [0 if mailbox == "device" else 1] for z in rs)
    assert not any(bool(z["0/used"]) for z in rs)
    for D in (6, 32):
        for z in rs:
            a, b = _unpack(z, f"1/{D}"), _unpack(z, f"0/{D}")
            assert a["steps"] == b["steps"] == 8
            assert a["proposal_scale"] == b["proposal_scale"] and a["accept"] == b["accept"]
            for k in ("u", "x", "logl"):
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
            assert a["proposal_scale"] == _unpack(rs[0], f"1/{D}")["proposal_scale"]


# ------------------------------------------------------------------------------------------------------------------
# 3. sharded = one rank, up to the order of the sums
# ------------------------------------------------------------------------------------------------------------------
def _kernel_call_device(lo, hi, group_opts, Dk=6):
    """``_kernel_call`` of tests/test_gpu_sharded_sampler.py (N = 640, D = 6, n_max = 6, seed 21) with the likelihood on the
    device."""
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, x, u, like, flow, geo = _kernel_case(Dk)
    sl = slice(lo, hi)
    state = dict(u=u[sl].copy(), x=x[sl].copy(), logdetj=scaler.inverse(u[sl])[1], logl=like(x[sl])[0],
                 logp=prior.logpdf(x[sl]), beta=0.5, blobs=None)
    funcs = dict(loglike=lambda xt: (-0.5 * (xt ** 2).sum(dim=1), None), logprior=prior.logpdf, scaler=scaler, flow=flow,
                 theta_geometry=geo)
    opts = dict(n_max=6, n_steps=10 ** 6, progress_bar=None, proposal_scale=2.38 / Dk ** 0.5, seed=21,
                device_likelihood=True, wait_timeout=WAIT, **group_opts)
    return pmcmc.preconditioned_pcn(state, funcs, opts)


def _one_rank_worker(rank, world, port, out):
    dist = _init(rank, world, port)
    lo, hi = rank * 640 // world, (rank + 1) * 640 // world
    r = _kernel_call_device(lo, hi, dict(group=None, shard_offset=lo))
    np.savez(out % rank, u=r["u"], logl=r["logl"], sigma=r["proposal_scale"], accept=r["accept"], steps=r["steps"])
    _done(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_device_likelihood_call_equals_one_rank(tmp_path, world):
    """Criteria and numbers of ``test_sharded_pipelined_kernel_call_equals_one_rank``, for its reason: rank-ordered
    partial sums differ from the one-rank sum in the last bits, so sigma differs in the last bits and a walker whose u sits
    on alpha may flip.  The 0.5 % is a cap, not a measurement; the observed share is printed."""
    skip_unless_gpus_for(world)
    rs = _spawn(_one_rank_worker, world, str(tmp_path / "k%d.npz"))
    whole = _kernel_call_device(0, 640, {})
    for r in rs:
        assert float(r["sigma"]) == float(rs[0]["sigma"]) and int(r["steps"]) == whole["steps"] == 6
    np.testing.assert_allclose(float(rs[0]["sigma"]), whole["proposal_scale"], rtol=1e-12)
    np.testing.assert_allclose(float(rs[0]["accept"]), whole["accept"], rtol=1e-12)
    u2 = np.concatenate([r["u"] for r in rs])
    same = np.isclose(u2, whole["u"], rtol=1e-9, atol=1e-12).all(axis=1)
    print(f"world {world}: rows on the one-rank trajectory {same.mean():.4%} ({int(same.sum())} of {same.size})")
    assert same.mean() >= 0.995, same.mean()
    np.testing.assert_allclose(np.concatenate([r["logl"] for r in rs])[same], whole["logl"][same], rtol=1e-8)


# ------------------------------------------------------------------------------------------------------------------
# 4. gated rows and NaN
# ------------------------------------------------------------------------------------------------------------------
def strict(xt):
    assert bool(torch.isfinite(xt).all()) and float(xt.abs().max()) <= 3.0
    return f_torch(xt)


def holes(x):
    ll = f_torch(x)
    return torch.where(x[:, 1] < -0.4, torch.full_like(ll, float("nan")), ll)


# The random-walk kinds: their proposal scale is not capped, so one step at 2.38 / sqrt(D) sends rows out of the support and
# the gate has work to do.  tpCN caps sigma at 0.99 (mcmc.py:54) and a single step of it leaves every row of this problem
# inside the support (1024 of 1024 reached the likelihood on the MI355X): it cannot show a gated row in one step, and its
# exchange is covered by the other tests of this file.
GATED = [(kind, f) for kind in ("preconditioned_rwm", "rwm") for f in (strict, holes)]


def _gated_calls(part, lo, group_opts):
    # (the walkers' own logl comes from f_torch for both: `holes` only bites on the proposals)
    return {f"{kind}/{f.__name__}": _call(kind, part, device_like(f), _logl0(part), device=True, n_max=1, scale=2.38,
                                          wait_timeout=WAIT, **group_opts)
            for kind, f in GATED}


def _gated_worker(rank, world, port, out):
    dist = _init(rank, world, port)
    part, lo, hi = _shard(_problem(5, 1024, "maf3", seed=3), rank, world)
    store = {}
    for tag, r in _gated_calls(part, lo, dict(group=None, shard_offset=lo)).items():
        _pack(store, tag, r)
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
def test_gated_rows_and_nan_on_two_ranks_equal_the_one_rank_call(tmp_path):
    """One step (no sum feeds back, no row can flip) at a proposal scale that sends many proposals out of the support: the
    ranks' rows concatenated are the one-rank device-likelihood call bit for bit, and the ranks' rows that reached the
    likelihood add up to the one-rank count, which is below N."""
    skip_unless_gpus_for(2)
    rs = _spawn(_gated_worker, 2, str(tmp_path / "g%d.npz"))
    whole = _gated_calls(_problem(5, 1024, "maf3", seed=3), 0, {})
    for tag, w in whole.items():
        parts = [_unpack(z, tag) for z in rs]
        for k in FIELDS:
            assert np.array_equal(np.concatenate([p[k] for p in parts]), w[k]), (tag, k)
        calls = sum(p["calls"] for p in parts)
        print(f"{tag}: rows that reached the likelihood {int(calls)} of 1024")
        assert calls == w["calls"] and w["calls"] < 1024, (tag, calls, w["calls"])
        assert all(p["steps"] == 1 for p in parts) and w["steps"] == 1
        assert np.isfinite(w["logl"]).all()


# ------------------------------------------------------------------------------------------------------------------
# 5. host prior
# ------------------------------------------------------------------------------------------------------------------
HOST_PRIOR = [(kind, how) for kind in ("preconditioned_pcn", "rwm") for how in ("gamma", "device_prior_off")]


def _host_prior_worker(rank, world, port, out):
    from scipy.stats import gamma, uniform
    import pocomc_amd as pc
    dist = _init(rank, world, port)
    D = 5
    store = {}
    for kind, how in HOST_PRIOR:
        extra = {}
        if how == "gamma":
            prior = pc.Prior([uniform(-3, 6)] * (D - 1) + [gamma(2.0, loc=-3.0)])
            assert prior.device_descriptor(torch.device("cuda", torch.cuda.current_device())) is None
        else:
            prior = pc.Prior([uniform(-3, 6)] * D)
            extra = dict(device_prior=False)
        part, lo, hi = _shard(_problem(D, 1024, "maf3", seed=4, prior=prior), rank, world)

        def finite_rows(xt):
            assert bool(torch.isfinite(xt).all())
            if how != "gamma":
                assert float(xt.abs().max()) <= 3.0
            return f_torch(xt)
        common = dict(scale=1.0, group=None, shard_offset=lo, wait_timeout=WAIT, **extra)
        logl0 = _logl0(part)
        _pack(store, f"{kind}/{how}/host", _call(kind, part, host_like(f_torch), logl0, device=False, **common))
        _pack(store, f"{kind}/{how}/device", _call(kind, part, device_like(finite_rows), logl0, device=True, **common))
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
def test_host_prior_on_two_ranks_equals_the_sharded_host_call(tmp_path):
    """A prior the device does not evaluate (a gamma factor), or ``device_prior=False``: x' goes to the host for Prior.logpdf
    only (``pmc_step_lik_rows``), the likelihood stays on the device -- each rank's call is the same rank's host call bit
    for bit."""
    skip_unless_gpus_for(2)
    rs = _spawn(_host_prior_worker, 2, str(tmp_path / "p%d.npz"))
    for kind, how in HOST_PRIOR:
        calls = 0
        for z in rs:
            a, b = _unpack(z, f"{kind}/{how}/host"), _unpack(z, f"{kind}/{how}/device")
            _assert_same(a, b)
            assert b["steps"] == 8
            calls += b["calls"]
        assert calls < 8 * 1024, (kind, how, calls)                           # rows were gated


# ------------------------------------------------------------------------------------------------------------------
# 6. Sampler
# ------------------------------------------------------------------------------------------------------------------
def _torch_gaussian(counter=None):
    """The Gaussian of tests/test_gpu_sharded_sampler.py on this rank's device."""
    icov = torch.tensor(ICOV, dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))

    def like(xt):
        if counter is not None:
            counter[0] += len(xt)
        return NORM - 0.5 * torch.einsum("ni,ij,nj->n", xt, icov, xt)
    return like


def _sampler_worker(rank, world, port, out):
    dist = _init(rank, world, port)
    from scipy.stats import norm
    import pocomc_amd as pc
    calls = [0]
    prior = pc.Prior([norm(0.0, 5.0)] * DS)
    s = pc.Sampler(prior=prior, likelihood=_torch_gaussian(calls), vectorize=True, flow="maf3", n_active=256,
                   n_effective=512, random_state=4, train_config=dict(fit_parallel="auto"), device_likelihood=True,
                   mcmc_options=dict(wait_timeout=WAIT))
    assert s.world == world and s.rank == rank
    s.run(n_total=1024, n_evidence=1024, progress=False)
    logz, err = s.evidence()
    x, w, logl, logp = s.posterior()
    np.savez(out % rank, logz=logz, beta=np.asarray(s.particles.get("beta")), x=x, w=w, calls=s.calls,
             own_calls=calls[0], params=s.flow.params.cpu().numpy())
    _done(dist)


@pytest.mark.gpu
def test_two_rank_sampler_with_a_device_likelihood(tmp_path):
    """Assertions and thresholds of ``test_two_rank_sampler``: replicated bookkeeping identical on both ranks, the
    likelihood work shared, the answer right."""
    skip_unless_gpus_for(2)
    r0, r1 = _spawn(_sampler_worker, 2, str(tmp_path / "rank%d.npz"))
    assert np.array_equal(r0["beta"], r1["beta"])
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["w"], r1["w"])
    assert float(r0["logz"]) == float(r1["logz"])
    assert np.array_equal(r0["params"], r1["params"])
    # the likelihood work is shared: each rank made about half of the calls
    assert int(r0["calls"]) == int(r1["calls"])
    assert abs(int(r0["own_calls"]) + int(r1["own_calls"]) - int(r0["calls"])) <= 0.02 * int(r0["calls"])
    assert 0.4 < int(r0["own_calls"]) / int(r0["calls"]) < 0.6
    # and the answer is right
    assert abs(float(r0["logz"]) - TRUE_LOGZ) < 0.35, (float(r0["logz"]), TRUE_LOGZ)
    m = np.average(r0["x"], weights=r0["w"], axis=0)
    c = np.cov(r0["x"].T, aweights=r0["w"])
    post = np.linalg.inv(ICOV + np.eye(DS) / 25.0)
    assert np.abs(m).max() < 0.25
    assert np.abs(c - post).max() < 0.35


def _ckpt_worker(rank, world, port, out_dir):
    dist = _init(rank, world, port)
    from scipy.stats import norm
    import pocomc_amd as pc
    prior = pc.Prior([norm(0.0, 5.0)] * DS)
    mk = lambda: pc.Sampler(prior=prior, likelihood=_torch_gaussian(), vectorize=True, flow="maf3", n_active=128,
                            n_effective=256, random_state=9, train_config=dict(epochs=20), output_dir=out_dir,
                            output_label="sh", device_likelihood=True, mcmc_options=dict(wait_timeout=WAIT))
    s = mk()
    s.run(n_total=512, n_evidence=0, progress=False, save_every=2)
    dist.barrier()
    files = sorted(p_ for p_ in os.listdir(out_dir) if p_.endswith(".state"))
    assert "sh_final.state" in files and not any(p_.endswith(".temp") for p_ in os.listdir(out_dir))
    # every rank loads the file rank 0 wrote and keeps ITS OWN rank: a resumed run shards the walkers correctly
    first = sorted(f for f in files if "final" not in f)[0]
    s2 = mk()
    s2.run(n_total=512, n_evidence=0, progress=False, resume_state_path=os.path.join(out_dir, first))
    assert s2.rank == rank and s2.world == world and s2.device_likelihood is True
    x, w, _, _ = s2.posterior()
    np.savez(os.path.join(out_dir, f"resumed{rank}.npz"), x=x, w=w, logz=s2.evidence()[0], t=s2.t)
    _done(dist)


@pytest.mark.gpu
def test_two_rank_checkpoint_and_resume_with_a_device_likelihood(tmp_path):
    """``test_two_rank_checkpoint_and_resume`` with the likelihood on the device."""
    skip_unless_gpus_for(2)
    import torch.multiprocessing as mp
    mp.spawn(_ckpt_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "resumed0.npz"), np.load(tmp_path / "resumed1.npz")
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["w"], r1["w"]) and float(r0["logz"]) == float(r1["logz"])
    # the resumed walker sets were assembled from two DIFFERENT shards: no duplicated block of rows
    tail = r0["x"][-128:]
    assert len(np.unique(tail.round(12), axis=0)) > 64
    m = np.average(r0["x"], weights=r0["w"], axis=0)
    assert np.abs(m).max() < 0.4


# ------------------------------------------------------------------------------------------------------------------
# 7. what stays refused
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["blobs", "replay", "trace"])
def test_sharded_device_likelihood_still_refuses(what, monkeypatch):
    """Blobs, replayed variates and traces raise ValueError for sharded walkers as for one rank -- before any collective and
    before the device is touched (no process group exists here: a collective would fail otherwise)."""
    from pocomc_amd import mcmc as pmcmc
    monkeypatch.setattr(pmcmc, "_sharded", lambda group: True)
    N, D = 64, 3
    z = np.zeros((N, D))
    state = dict(u=z, x=z, logdetj=np.zeros(N), logl=np.zeros(N), logp=np.zeros(N), beta=0.5,
                 blobs=np.zeros(N) if what == "blobs" else None)
    funcs = dict(loglike=device_like(f_torch), logprior=lambda x: np.zeros(len(x)), scaler=None, u_geometry=None)
    opts = dict(n_max=2, n_steps=10, progress_bar=None, proposal_scale=0.5, device_likelihood=True, group=None,
                shard_offset=0, seed=1)
    kw = dict(replay=object()) if what == "replay" else dict(trace=[]) if what == "trace" else {}
    with pytest.raises(ValueError, match="blobs" if what == "blobs" else "replayed variates and traces"):
        pmcmc.rwm(state, funcs, opts, **kw)
