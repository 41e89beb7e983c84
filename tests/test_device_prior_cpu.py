"""What a prior on the device checks before it touches one (no GPU): the option and the Sampler's arguments, the values a
prior callable may return, ``DevicePrior``'s own arguments, and the C ABI's new pieces."""
import ctypes

import numpy as np
import pytest
import torch


def test_device_logprior_needs_device_likelihood():
    """``option_dict["device_logprior"]`` without ``device_likelihood``: ValueError before the device is touched, in every
    kernel."""
    from pocomc_amd import mcmc as pmcmc
    N, D = 64, 3
    z = np.zeros((N, D))
    for kind in pmcmc.KINDS:
        state = dict(u=z, x=z, logdetj=np.zeros(N), logl=np.zeros(N), logp=np.zeros(N), beta=0.5, blobs=None)
        funcs = dict(loglike=lambda x: (np.zeros(len(x)), None), logprior=lambda xt: torch.zeros(len(xt), dtype=torch.float64),
                     scaler=None, flow=None, u_geometry=None, theta_geometry=None)
        opts = dict(n_max=2, n_steps=10, progress_bar=None, proposal_scale=0.5, seed=1, device_logprior=True)
        with pytest.raises(ValueError, match="device_logprior.*device_likelihood"):
            getattr(pmcmc, kind)(state, funcs, opts)


def _host_prior(D=3):
    from scipy.stats import uniform
    import pocomc_amd as pc
    return pc.Prior([uniform(-5, 10)] * D)


def _device_prior(D=3):
    import pocomc_amd as pc
    return pc.DevicePrior(lambda xt: torch.zeros(len(xt), dtype=torch.float64, device=xt.device),
                          np.array([[-5.0, 5.0]] * D), lambda size: np.random.uniform(-5, 5, size=(size, D)))


def test_sampler_device_prior_arguments():
    """``device_prior=True`` without ``device_likelihood``, or with a prior that has no ``logpdf_device``: ValueError (raised
    before the flow, the first thing that needs the device, is built)."""
    import pocomc_amd as pc
    like = lambda xt: torch.zeros(len(xt), dtype=torch.float64, device=xt.device)
    with pytest.raises(ValueError, match="device_prior=True needs device_likelihood=True"):
        pc.Sampler(prior=_device_prior(), likelihood=like, vectorize=True, device_prior=True, random_state=0)
    with pytest.raises(ValueError, match="logpdf_device.*got Prior"):
        pc.Sampler(prior=_host_prior(), likelihood=like, vectorize=True, device_likelihood=True, device_prior=True,
                   random_state=0)

    class Attr:                                              # an attribute of that name that is no method
        logpdf_device, bounds, dim = None, np.array([[-5.0, 5.0]] * 3), 3
        logpdf = rvs = staticmethod(lambda *a: None)
    with pytest.raises(ValueError, match="logpdf_device.*got Attr"):
        pc.Sampler(prior=Attr(), likelihood=like, vectorize=True, device_likelihood=True, device_prior=True, random_state=0)


def test_device_prior_result_is_checked():
    """``device_logp``: the device likelihood's checks, with messages that name the prior."""
    from pocomc_amd.mcmc import device_logp
    ok = torch.zeros(4, dtype=torch.float64)
    assert device_logp(ok, 4, "cpu") is ok
    assert device_logp(ok.float(), 4, "cpu").dtype == torch.float32
    holes = torch.tensor([0.0, float("-inf"), float("nan"), 1.0], dtype=torch.float64)
    assert device_logp(holes, 4, "cpu") is holes                          # -inf and NaN are values
    for out, word in ((np.zeros(4), "device prior: .*ndarray"), (None, "device prior: .*NoneType"),
                      ((ok, None), "device prior: .*tuple"),
                      (torch.zeros(3, dtype=torch.float64), r"device prior: expected shape \(4,\), got \(3,\)"),
                      (torch.zeros(4, 1, dtype=torch.float64), "device prior: expected shape"),
                      (torch.zeros(4, dtype=torch.int64), "device prior: .*int64"),
                      (torch.zeros(4, dtype=torch.float16), "device prior: .*float16"),
                      (ok, "device prior: expected a tensor on device cuda:0, got one on cpu")):
        with pytest.raises(ValueError, match=word):
            device_logp(out, 4, "cuda:0")


def test_device_prior_arguments():
    import pocomc_amd as pc
    f = lambda xt: torch.zeros(len(xt), dtype=torch.float64, device=xt.device)
    rvs = lambda size: np.zeros((size, 2))
    b = np.array([[-1.0, 1.0], [0.0, np.inf]])
    p = pc.DevicePrior(f, b, rvs)
    assert p.dim == 2 and p.logpdf_device is f and not hasattr(p, "device_descriptor")
    assert np.array_equal(p.bounds, b) and p.bounds.dtype == np.float64
    p.bounds[0, 0] = 7.0
    assert p.bounds[0, 0] == -1.0                                         # a copy each time
    assert pc.DevicePrior(f, [[-1, 1], [0, 2]], rvs, dim=2).bounds.dtype == np.float64
    assert pc.DevicePrior(f, [[np.nan, 1.0], [-np.inf, np.inf]], rvs).dim == 2          # NaN / inf: unbounded
    assert p.rvs(5).shape == (5, 2) and p.rvs(5).dtype == np.float64
    for args, word in (((None, b, rvs), "logpdf_device must be callable"), ((f, b, None), "rvs must be callable"),
                       ((f, np.zeros(3), rvs), r"shape \(D, 2\)"), ((f, np.zeros((2, 3)), rvs), r"shape \(D, 2\)"),
                       ((f, np.zeros((0, 2)), rvs), r"shape \(D, 2\)"), ((f, "box", rvs), "array of floats"),
                       ((f, [[1.0, 1.0], [0.0, 1.0]], rvs), "dimension 0"), ((f, [[0.0, 1.0], [2.0, -2.0]], rvs), "dimension 1"),
                       ((f, b, rvs, 3), "dim = 3 but bounds has 2 rows"), ((f, b, rvs, 2.5), "dim = 2.5")):
        with pytest.raises(ValueError, match=word):
            pc.DevicePrior(*args)
    with pytest.raises(ValueError, match=r"expected shape \(5, 2\) from rvs, got \(5, 3\)"):
        pc.DevicePrior(f, b, lambda size: np.zeros((size, 3))).rvs(5)


def _named_log_density(xt):
    return -0.5 * (xt * xt).sum(dim=1)


def test_device_prior_survives_a_checkpoint():
    """The prior is the user's object, pickled with the rest of a Sampler's state."""
    import dill
    import pocomc_amd as pc
    p = pc.DevicePrior(_named_log_density, np.array([[-1.0, 1.0]] * 2), lambda size: np.zeros((size, 2)), dim=2)
    q = dill.loads(dill.dumps(p))
    x = torch.tensor([[0.5, -0.5], [1.0, 0.0]], dtype=torch.float64)
    assert torch.equal(q.logpdf_device(x), p.logpdf_device(x)) and q.dim == 2 and np.array_equal(q.bounds, p.bounds)
    assert q.rvs(3).shape == (3, 2)


def test_the_c_abi_of_the_device_prior():
    """``pmc_step_prior_rows`` is declared, bound and exported; the mode word took the reserved padding behind
    ``fill_rejected``, so no offset and no size of ``pmc_step_t`` changed and the ABI version stays 9."""
    import os
    from pocomc_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "pocomc_amd.h")).read()
    assert "int pmc_step_prior_rows(const pmc_step_t* s, const void* logp, int logp_is_f32, void* stream);" in hdr
    assert "#define PMC_ABI_VERSION 9" in hdr
    res, args = _lib.SIGNATURES["pmc_step_prior_rows"]
    assert res is ctypes.c_int and len(args) == 4
    S = _lib.pmc_step_t
    assert S.prior_rows.offset == S.fill_rejected.offset + 4 and S.prior_rows.size == 4
    assert S.lik_x.offset == S.fill_rejected.offset + 8 and ctypes.sizeof(S) == S.blob_row_bytes.offset + 8
    assert S().prior_rows == 0                                            # zero: a prior the device does not know runs on the host
    lib = _lib.load()
    assert lib.pmc_abi_version() == 9
    # argument checks of the entry point itself run on the host: no launch happens for any of these
    s = S()
    assert lib.pmc_step_prior_rows(None, None, 0, None) != 0
    assert lib.pmc_step_prior_rows(ctypes.byref(s), None, 0, None) != 0
    assert b"pmc_step_prior_rows" in lib.pmc_last_error()
