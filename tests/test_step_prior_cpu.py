"""A flow / joint prior inside the step of a host likelihood (``pmc_step_ext_t.prior_stage``, kernel option ``step_prior``),
what needs no GPU: the hand-over decision does not see the stage, the option's refusals come before any device call, and
``pmc_step_prior_stage`` checks its struct on the host before it launches anything."""
import ctypes as C
import os

import numpy as np
import pytest

from .test_step_handover_cpu import ADDR, FIELDS, STEP, grid


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


def ext_descriptor(sw, stage):
    """``test_step_handover_cpu.descriptor`` as the head of a ``pmc_step_ext_t``: the same fields from the same switches, the
    extension flag set, ``prior_stage`` a fake address or NULL."""
    from pocomc_amd import _lib
    s = _lib.pmc_step_ext_t(n=21, D=5, h_fin=ADDR["h_fin"], h_logp_out=ADDR["h_logp_out"], h_logp=ADDR["h_logp"],
                            p_x=ADDR["p_x"], p_logp=ADDR["p_logp"], ext=_lib.PMC_STEP_EXT, prior_stage=stage)
    s.cur.x = ADDR["cur_x"]
    for k in ("host_direct", "prior_rows", "fill_rejected"):
        setattr(s, k, int(sw[k]))
    for k in ("p_xT", "lik_x", "prior", "h_done", "done_ticket", "h_clean", "clean_count", "h_x"):
        setattr(s, k, ADDR[k] if sw[k] else None)
    return s


def handover(lib, s, epilogue):
    from pocomc_amd import _lib
    h, mode, unknown = _lib.pmc_handover_t(), C.c_int32(-7), C.c_int32(-7)
    assert lib.pmc_step_handover(C.byref(s), STEP, int(epilogue), C.byref(h), C.byref(mode), C.byref(unknown)) == 0
    return {k: getattr(h, k) or 0 for k in FIELDS}, mode.value, unknown.value


def test_the_handover_does_not_see_the_stage(lib):
    """Every row of the hand-over grid: the struct with ``prior_stage`` set equals, field for field, the same struct
    without it (and the plain ``pmc_step_t`` of the existing test) -- with ``prior`` NULL, which is where the stage runs, and
    with it set as well."""
    from .test_step_handover_cpu import query
    n = with_null_prior = 0
    for sw in grid():
        with_stage = handover(lib, ext_descriptor(sw, 0xF000), sw["epilogue"])
        without = handover(lib, ext_descriptor(sw, None), sw["epilogue"])
        assert with_stage == without == query(lib, sw), sw
        n += 1
        with_null_prior += not sw["prior"]
    assert n == 4096 and with_null_prior == 2048


def test_the_struct_grew_behind_its_end():
    """``pmc_step_t`` keeps its size and its fields; the stage pointer is the first field behind it, in ``pmc_step_ext_t``,
    and the word that says so is the reserved padding behind ``adapt_mode``."""
    from pocomc_amd import _lib
    S, E = _lib.pmc_step_t, _lib.pmc_step_ext_t
    assert C.sizeof(S) == S.blob_row_bytes.offset + 8
    assert E.prior_stage.offset == C.sizeof(S) and C.sizeof(E) == C.sizeof(S) + 8
    assert S.ext.offset == S.adapt_mode.offset + 4 and S.ext.size == 4 and S.adapt_c_sigma.offset == S.ext.offset + 4
    assert S().ext == 0 and E().prior_stage is None and _lib.PMC_STEP_EXT == 1
    assert C.sizeof(_lib.pmc_prior_stage_t) == 15 * 8
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    hdr = open(os.path.join(root, "include", "pocomc_amd.h")).read()
    assert "int pmc_step_prior_stage(const pmc_step_t* s, void* stream);" in hdr and "#define PMC_ABI_VERSION 9" in hdr


# ------------------------------------------------------------------------------------------------------------------
# the option's refusals
# ------------------------------------------------------------------------------------------------------------------
class StagePrior:
    """Has ``step_stage``; anything that touched the device would call it."""
    dim = 3

    def logpdf(self, x):
        raise AssertionError("the host prior must not be called")

    def step_stage(self, n, device=None):
        raise AssertionError("the device must not be touched")


class HostPrior:
    dim = 3

    def logpdf(self, x):
        raise AssertionError("the host prior must not be called")


def kernel_call(kind, logprior, replay=None, trace=None, **opts):
    from pocomc_amd import mcmc as pmcmc
    N, D = 64, 3
    z = np.zeros((N, D))
    state = dict(u=z, x=z, logdetj=np.zeros(N), logl=np.zeros(N), logp=np.zeros(N), beta=0.5, blobs=None)
    funcs = dict(loglike=lambda x: (np.zeros(len(x)), None), logprior=logprior, scaler=None, flow=None, u_geometry=None,
                 theta_geometry=None)
    opts = dict(dict(n_max=2, n_steps=10, progress_bar=None, proposal_scale=0.5, seed=1, step_prior=True), **opts)
    return getattr(pmcmc, kind)(state, funcs, opts, replay=replay, trace=trace)


def test_the_options_refusals_come_before_the_device():
    """No GPU here: a call that got past its refusal would fail in another way (``PocomcAmdError``, AttributeError)."""
    from pocomc_amd import mcmc as pmcmc
    stage = StagePrior()
    for kind in pmcmc.KINDS:
        with pytest.raises(ValueError, match="step_prior.*device_prior=True"):
            kernel_call(kind, stage.logpdf, device_likelihood=True)
        with pytest.raises(ValueError, match="step_prior.*process group"):
            kernel_call(kind, stage.logpdf, group=object())
        with pytest.raises(ValueError, match="step_prior.*replayed variates and traces"):
            kernel_call(kind, stage.logpdf, replay=object())
        with pytest.raises(ValueError, match="step_prior.*replayed variates and traces"):
            kernel_call(kind, stage.logpdf, trace=[])
        with pytest.raises(ValueError, match="step_prior.*step_stage.*got HostPrior"):
            kernel_call(kind, HostPrior().logpdf)
        with pytest.raises(ValueError, match="step_prior.*step_stage.*got <lambda>"):
            kernel_call(kind, lambda x: np.zeros(len(x)))


def test_sampler_step_prior_arguments():
    """``Sampler(step_prior=True)``: refused with a device likelihood (the message names ``device_prior=True``) and with a
    prior that has no ``step_stage``, before the flow -- the first thing that needs the device -- is built;
    ``device_prior=True`` without a device likelihood raises as it did."""
    import torch
    import pocomc_amd as pc
    from scipy.stats import uniform

    class Stage(StagePrior):
        bounds = np.array([[-5.0, 5.0]] * 3)
        rvs = staticmethod(lambda size: np.zeros((size, 3)))
        logpdf_device = staticmethod(lambda xt: torch.zeros(len(xt), dtype=torch.float64))
    like = lambda x: np.zeros(len(x))
    with pytest.raises(ValueError, match="step_prior=True.*device_prior=True"):
        pc.Sampler(prior=Stage(), likelihood=like, vectorize=True, device_likelihood=True, step_prior=True, random_state=0)
    with pytest.raises(ValueError, match="step_prior=True needs a prior with a step_stage method.*got Prior"):
        pc.Sampler(prior=pc.Prior([uniform(-5, 10)] * 3), likelihood=like, vectorize=True, step_prior=True, random_state=0)
    with pytest.raises(ValueError, match="device_prior=True needs device_likelihood=True"):
        pc.Sampler(prior=Stage(), likelihood=like, vectorize=True, device_prior=True, step_prior=True, random_state=0)


# ------------------------------------------------------------------------------------------------------------------
# the entry's own checks
# ------------------------------------------------------------------------------------------------------------------
def stage_struct(joint=False, n=21):
    """A struct the entry accepts up to its first launch: real (host) descriptors where the check follows a pointer -- the
    scaler, the flow and the table, for their widths -- fake addresses everywhere else.  Returns it with what it points to."""
    from pocomc_amd import _lib
    Df, Dr = 3, (2 if joint else 0)
    scaler, maf, rest = _lib.pmc_scaler_t(D=Df), _lib.pmc_maf_t(D=Df), _lib.pmc_prior_t(D=Dr)
    g = _lib.pmc_prior_stage_t(scaler=C.addressof(scaler), maf=C.addressof(maf), u32=0x100, z=0x200, lp32=0x300, ldj=0x400,
                               inside=0x500, count=0x600, h_count=0x700)
    if joint:
        g.flow_cols, g.rest, g.rest_cols, g.rest_logp = 0x800, C.addressof(rest), 0x900, 0xA00
    s = _lib.pmc_step_ext_t(n=n, D=Df + Dr, p_x=ADDR["p_x"], p_fin=0xB00, p_logp=ADDR["p_logp"], ext=_lib.PMC_STEP_EXT,
                            prior_stage=C.addressof(g))
    return s, g, (scaler, maf, rest)


@pytest.mark.parametrize("joint", [False, True])
def test_the_stage_refuses_before_any_launch(lib, joint):
    """Each refusal with a text of its own.  None of these calls reaches a launch: there is no device here, and every
    address but the three descriptors' is a fake."""
    def refused(change, word):
        s, g, keep = stage_struct(joint)
        change(s, g, keep)
        assert lib.pmc_step_prior_stage(C.byref(s), None) != 0, word
        msg = lib.pmc_last_error().decode()
        assert word in msg, (word, msg)
        return msg
    seen = set()
    seen.add(refused(lambda s, g, k: setattr(s, "prior", 0x3000), "device prior table as well"))
    seen.add(refused(lambda s, g, k: setattr(s, "prior_rows", 1), "GPU callable as well"))
    seen.add(refused(lambda s, g, k: setattr(s, "lik_x", 0x2000), "host likelihood"))
    for ws in ("u32", "z", "lp32", "ldj", "inside") + (("rest_logp",) if joint else ()):
        refused(lambda s, g, k: setattr(g, ws, None), "null workspace")
    seen.add(refused(lambda s, g, k: setattr(g, "count", None), "device counter"))
    refused(lambda s, g, k: setattr(g, "h_count", None), "device counter")
    for n in (0, -3):
        seen.add(refused(lambda s, g, k: setattr(s, "n", n), "n < 1"))
    refused(lambda s, g, k: setattr(s, "prior_stage", None), "no prior_stage")
    refused(lambda s, g, k: setattr(s, "ext", 0), "no prior_stage")                # (the extension is not read without the flag)
    refused(lambda s, g, k: setattr(s, "p_fin", None), "p_x, p_fin and p_logp")
    # a width the two *_pre entries refuse, in their words; and one that is not the step's
    if joint:
        refused(lambda s, g, k: (setattr(k[0], "D", 1), setattr(k[1], "D", 1)), "pmc_joint_prior_pre: the flow block needs at least 2")
        refused(lambda s, g, k: setattr(k[2], "D", 0), "pmc_joint_prior_pre: the rest needs at least 1")
        refused(lambda s, g, k: (setattr(k[2], "D", 155), setattr(s, "D", 158)), "pmc_joint_prior_pre: n_dim too large")
        refused(lambda s, g, k: setattr(g, "rest", None), "flow_cols, rest and rest_cols")
    else:
        refused(lambda s, g, k: (setattr(k[0], "D", 158), setattr(k[1], "D", 158), setattr(s, "D", 158)),
                "pmc_flow_prior_pre: n_dim too large")
        refused(lambda s, g, k: setattr(k[0], "D", 0), "pmc_flow_prior_pre: bad descriptor")
    refused(lambda s, g, k: setattr(s, "D", 7), "not the step's D")
    refused(lambda s, g, k: setattr(g, "image16", 0xC00), "image_per_transform")
    assert len(seen) == 5                                                          # texts of their own
    assert lib.pmc_step_prior_stage(None, None) != 0 and b"pmc_step_prior_stage" in lib.pmc_last_error()
