"""The prior as a GPU callable on sharded walkers, one process per GPU (``option_dict["device_logprior"]`` with a ``group``,
``Sampler(device_likelihood=True, device_prior=True)`` with two ranks): the callable sees this rank's rows only, like the
likelihood, and each rank's call is the same rank's call with the numpy prior on the host, bit for bit -- whichever tier
carried the sums.

The GPU box has one device: two ranks and the test process share it and talk over ``gloo`` (three processes on the device).
Every worker passes ``wait_timeout=60``: a rank that loses its peer ends with an error instead of waiting."""

import numpy as np
import pytest

from .test_gpu_device_likelihood import _assert_same
from .test_gpu_device_prior_callable import (DS, HALF, Seen, _call, _problem, box_results, box_sampler, prior_np)
from .test_gpu_sharded_device_likelihood import WAIT, _done, _init, _pack, _spawn, _unpack, skip_unless_gpus_for

KINDS = ["preconditioned_pcn", "rwm"]
N, D = 96, 5


def _shard(prob, rank, world):
    scaler, flow, geo, x, u = prob
    lo, hi = rank * len(x) // world, (rank + 1) * len(x) // world
    return (scaler, flow, geo, x[lo:hi], u[lo:hi]), lo, hi


def _call_worker(rank, world, port, out, mailbox, c_allreduce):
    dist = _init(rank, world, port, PMC_COMM_MAILBOX=mailbox, PMC_C_ALLREDUCE=c_allreduce)
    from pocomc_amd import mcmc as pmcmc
    part, lo, hi = _shard(_problem(D, N, "maf3", seed=1), rank, world)
    store = {}
    for kind in KINDS:
        common = dict(group=None, shard_offset=lo, wait_timeout=WAIT)
        seen = Seen()
        _pack(store, f"{kind}/host", _call(kind, part, prior_np, False, **common))
        _pack(store, f"{kind}/device", _call(kind, part, seen, True, **common))
        store[f"{kind}/seen"] = np.array([seen.calls, seen.rows, seen.ninf, seen.nan, seen.bad_input], dtype=np.int64)
    store["comm_used"] = np.bool_(any(v[0] for v in pmcmc._COMMS.values()))
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["device-mailbox", "process-group"])
def test_two_rank_device_prior_call_equals_the_two_rank_host_prior_call(tmp_path, tier):
    """Per rank, on the library's own exchange over device mailboxes and on the process group's all-reduce."""
    skip_unless_gpus_for(2)
    rs = _spawn(_call_worker, 2, str(tmp_path / "r%d.npz"), "device", "1" if tier == "device-mailbox" else "0")
    assert all(bool(z["comm_used"]) == (tier == "device-mailbox") for z in rs)
    for kind in KINDS:
        rows = ninf = nan = 0
        for z in rs:
            a, b = _unpack(z, f"{kind}/host"), _unpack(z, f"{kind}/device")
            _assert_same(a, b)
            assert a["evaluations"] == b["evaluations"] == 6 * (N // 2) and b["steps"] == 6
            assert b["calls"] < b["evaluations"]
            assert b["proposal_scale"] == _unpack(rs[0], f"{kind}/device")["proposal_scale"]       # one sigma on both ranks
            calls, r, i, n, bad = (int(v) for v in z[f"{kind}/seen"])
            assert calls == 6 and r == 6 * (N // 2) and bad == 0                # this rank's rows only, every step
            rows, ninf, nan = rows + r, ninf + i, nan + n
        print(f"{kind} {tier}: {ninf} -inf ({ninf / rows:.1%}) and {nan} NaN of {rows} rows")
        assert ninf >= 0.1 * rows and nan >= 1                                   # the holes opened


def _sampler_worker(rank, world, port, out):
    dist = _init(rank, world, port)
    store = {}
    for tag, on_device in (("host", False), ("device", True)):
        s = box_sampler(on_device, mcmc_options=dict(wait_timeout=WAIT))
        assert s.world == world and s.rank == rank
        s.run(n_total=256, n_evidence=256, progress=False)
        res, (x, w, logl, logp), (logz, err), calls = box_results(s)
        store.update({f"{tag}/x": x, f"{tag}/w": w, f"{tag}/logl": logl, f"{tag}/logp": logp, f"{tag}/logz": np.float64(logz),
                      f"{tag}/err": np.float64(err), f"{tag}/calls": np.int64(calls), f"{tag}/beta": np.asarray(res["beta"]),
                      f"{tag}/pool_x": res["x"], f"{tag}/pool_logp": res["logp"]})
    np.savez(out % rank, **store)
    _done(dist)


@pytest.mark.gpu
def test_two_rank_sampler_with_a_device_prior(tmp_path):
    """The Sampler of ``test_sampler_with_a_device_prior_equals_the_sampler_with_the_host_prior`` on two ranks: warm-up and
    evidence evaluate each rank's share through ``logpdf_device`` and gather the values.  Both ranks hold the same results,
    and they are the two-rank run's with the host prior."""
    skip_unless_gpus_for(2)
    r0, r1 = _spawn(_sampler_worker, 2, str(tmp_path / "s%d.npz"))
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), k                                   # replicated bookkeeping
    for k in ("x", "w", "logl", "logp", "logz", "err", "calls", "beta", "pool_x", "pool_logp"):
        assert np.array_equal(r0[f"host/{k}"], r0[f"device/{k}"]), k
    x = r0["device/x"]
    assert len(x) > 0 and x.shape[1] == DS and (x[:, 0] < x[:, 1]).all() and (np.abs(x) <= HALF).all()
    assert r0["device/beta"][-1] == 1.0 and np.isfinite(float(r0["device/logz"]))
