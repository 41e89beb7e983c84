"""Blobs of a device likelihood on sharded walkers, one process per GPU: each rank's accept launch moves the blob rows of
its own walkers, the Sampler's ranks all-gather the walkers' blobs (and the warm-up block's) as tensors so that every rank
holds the same pool.  The invariant of ``tests/test_gpu_device_blobs.py``: a walker that moved carries g(x), bit for bit.

Two ranks on one GPU over ``gloo``, started like the ranks of ``tests/test_gpu_sharded_device_likelihood.py``; every rank's
process ends itself after ``LIMIT`` seconds (SIGALRM), and the parent stops waiting for the ranks soon after."""
import signal
import time

import numpy as np
import pytest
import torch

from .test_gpu_device_blobs import _assert_same, _call, _g_of, check_invariant, g, sentinel, with_blobs, without_blobs
from .test_gpu_device_likelihood import _problem, f_torch
from .test_gpu_sharded_device_likelihood import WAIT, _done, _free_port, _init, _logl0, _shard, skip_unless_gpus_for

LIMIT = 420          # seconds a rank's process may live


def _spawn(worker, world, *args):
    """The ranks as fresh processes, each under its own time limit (the worker arms it); the parent gives up a little later
    and ends what is left."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(worker, args=(world, _free_port()) + args, nprocs=world, join=False)
    deadline = time.monotonic() + LIMIT + 30
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p_ in ctx.processes:
                if p_.is_alive():
                    p_.kill()
            pytest.fail(f"the ranks did not finish within {LIMIT + 30} s")


def _kernel_worker(rank, world, port, out):
    signal.alarm(LIMIT)
    dist = _init(rank, world, port)
    store = {}
    for kind, flow_name, D in (("preconditioned_pcn", "maf3", 6), ("preconditioned_rwm", "nsf3", 6), ("rwm", "maf3", 6)):
        part, lo, hi = _shard(_problem(D, 1000, flow_name, seed=D), rank, world)
        n = hi - lo
        logl0 = _logl0(part)
        start = sentinel(n, g(torch.zeros(1, D, dtype=torch.float64, device="cuda")))
        common = dict(group=None, shard_offset=lo, wait_timeout=WAIT)
        a = _call(kind, part, without_blobs(f_torch), logl0, None, n_max=2, **common)
        b = _call(kind, part, with_blobs(f_torch, g), logl0, start.clone(), n_max=2, **common)
        _assert_same(a, b)
        moved = check_invariant(b, part[4], start, g, f"rank {rank} {kind} {flow_name}")
        store[f"{kind}/moved"], store[f"{kind}/sigma"] = np.int64(moved.sum()), np.float64(b["proposal_scale"])
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
def test_each_rank_moves_the_blobs_of_its_rows(tmp_path):
    """A kernel call per rank (500 rows each: a tail block on both): the call with blobs is the same rank's call without
    them bit for bit, the moved walkers carry g(x), the others their sentinel; both sets are non-empty on every rank."""
    skip_unless_gpus_for(2)
    out = str(tmp_path / "k%d.npz")
    _spawn(_kernel_worker, 2, out)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    for kind in ("preconditioned_pcn", "preconditioned_rwm", "rwm"):
        assert float(r0[f"{kind}/sigma"]) == float(r1[f"{kind}/sigma"])          # one sigma on both ranks
        assert 0 < int(r0[f"{kind}/moved"]) < 500 and 0 < int(r1[f"{kind}/moved"]) < 500


def _sampler_worker(rank, world, port, out):
    signal.alarm(LIMIT)
    dist = _init(rank, world, port)
    from scipy.stats import uniform
    import pocomc_amd as pc
    D = 5
    prior = pc.Prior([uniform(-5, 10)] * D)
    mk = lambda blobs: pc.Sampler(prior=prior, likelihood=with_blobs(f_torch, g) if blobs else f_torch, vectorize=True,
                                  flow="maf3", n_active=256, n_effective=512, random_state=4,
                                  train_config=dict(epochs=30), device_likelihood=True, device_blobs=blobs,
                                  mcmc_options=dict(wait_timeout=WAIT))
    s = mk(True)
    assert s.world == world and s.rank == rank
    s.run(n_total=1024, n_evidence=0, progress=False)
    x, w, logl, logp, b = s.posterior(return_blobs=True)
    assert s.particles.blob_rows().is_cuda
    res = s.results
    plain = mk(False)
    plain.run(n_total=1024, n_evidence=0, progress=False)
    xp, wp, _, _ = plain.posterior()
    np.savez(out % rank, x=x, w=w, b=b, calls=s.calls, rx=res["x"], rb=res["blobs"], xp=xp, wp=wp, callsp=plain.calls)
    _done(dist)


@pytest.mark.gpu
def test_two_rank_sampler_with_device_blobs(tmp_path):
    """Every rank returns the same posterior and the same blobs, g of the samples; the run without blobs is the same run."""
    skip_unless_gpus_for(2)
    out = str(tmp_path / "rank%d.npz")
    _spawn(_sampler_worker, 2, out)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    for k in ("x", "w", "b", "rx", "rb"):
        assert np.array_equal(r0[k], r1[k]), k
    assert r0["b"].shape == (len(r0["x"]), 2) and r0["b"].dtype == np.float64
    assert np.array_equal(r0["b"], _g_of(g, r0["x"]))
    assert np.array_equal(r0["rb"].reshape(-1, 2), _g_of(g, r0["rx"].reshape(-1, 5)))
    assert np.array_equal(r0["x"], r0["xp"]) and np.array_equal(r0["w"], r0["wp"]) and int(r0["calls"]) == int(r0["callsp"])
