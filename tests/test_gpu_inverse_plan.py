"""What ``pmc_maf_inverse(AUTO)`` and the fused pre-step launch is what the inverse plan (``csrc/inverse_plan.hip``) names:
AUTO and TRIANGULAR give, bit for bit, the result of the explicit algo constant of the plan's sweep (the sweeps have no
atomics and a fixed order), and the step with the plan's fused instance gives the bits of the stages launched one by one.

One flow per class of ``tests/inverse_plan_cases.py``.  Left out, because ``MAFSpec`` cannot build them (it pads every
degree group to a quad, so D features have at least ``ceil((D - 1) / 4)`` hidden tiles, and ``tri_ok`` allows 16 units per
degree): D = 64 and D = 65 with fewer than 16 hidden tiles, the spline flow of D = 1, a D <= 64 flow whose two-wave
tables exceed the LDS, the flows without room for the epilogue's scratch -- the ``*_hand`` cases, which only the CPU test
sees.  Left out as well: 64 / 65 hidden tiles with float32 helpers and 65 with a 16-bit image, where AUTO and TRIANGULAR
both fail before any launch (``tests/test_inverse_plan_cpu.py`` has the messages); 64 tiles with a bfloat16 image, the
widest flow the lane sweep covers, runs here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_plan_cases as ic  # noqa: E402
from test_gpu_epilogue_rows import _bits, _pre_step  # noqa: E402

AUTO, TRI, NAIVE, SOLO, DUO, LANE, LANE16 = 0, 1, 2, 6, 7, 8, 9
S_NONE, S_DPASS_AFFINE, S_DPASS_SPLINE, S_SOLO, S_DUO, S_LANE, S_NSF_SOLO, S_NSF_DUO = range(8)
EXPLICIT = {S_DPASS_AFFINE: NAIVE, S_DPASS_SPLINE: NAIVE, S_SOLO: SOLO, S_DUO: DUO, S_LANE: LANE, S_NSF_SOLO: SOLO,
            S_NSF_DUO: DUO}
# case -> the sweep AUTO runs (tests/test_inverse_plan_cpu.py has the whole plans); the lane classes also at 4097 and 8193
# rows, where the subsets per workgroup change
FLOWS = {"o4": S_DUO, "o8_d33": S_DUO, "o8_d60": S_DUO, "t15": S_DUO, "t16": S_LANE, "d65_t16": S_LANE, "t45_d66": S_LANE,
         "t64_d66_bf16": S_LANE,
         "t46_d66": S_DPASS_AFFINE, "tri_no": S_DPASS_AFFINE, "t15_bf16": S_DUO, "t16_bf16": S_LANE, "t16_f16": S_LANE,
         "t16_four": S_DUO, "nsf_d2": S_NSF_DUO, "nsf_d64": S_NSF_DUO, "nsf_d65": S_NSF_SOLO, "nsf_tri_no": S_DPASS_SPLINE,
         "nsf_bins4": S_DPASS_SPLINE, "nsf_bins16": S_DPASS_SPLINE}
FUSED = {"o4": S_DUO, "o8_d33": S_DUO, "t15": S_DUO, "t16_four": S_DUO, "nsf_d2": S_NSF_DUO, "nsf_d64": S_NSF_DUO,
         "t16": S_NONE, "nsf_d65": S_NONE}


def _flow(name):
    import pocomc_amd as pc
    from pocomc_amd.maf_spec import MAFSpec
    lay, fmt, reserved = ic.CASES[name]
    spec = MAFSpec(lay["D"], lay["T"], lay["hidden"], lay["uni"], lay["bins"])
    flow = pc.Flow(lay["D"], spec, seed=1, inverse_precision={0: "f32", 1: "bf16", 2: "f16"}[fmt], inverse_guard=False)
    flow._desc.reserved |= reserved
    assert {k: getattr(flow._desc, k) for k in ic.layout(name)} == ic.layout(name)
    return flow


def _inverse(flow, z, algo):
    """(rc, x bits, ladj bits) of pmc_maf_inverse on a poisoned output"""
    import torch
    from pocomc_amd import _lib
    n, D = z.shape
    x = torch.full((n, D), -7.0, dtype=torch.float32, device="cuda")
    ladj = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    rc = _lib.load().pmc_maf_inverse(C.byref(flow._desc), _lib.ptr(z), _lib.ptr(x), _lib.ptr(ladj), n, algo, _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, _bits(x.cpu().numpy()), _bits(ladj.cpu().numpy())


def _plan(flow, n, algo, fused=0):
    from pocomc_amd import _lib
    p = _lib.pmc_inverse_plan_t()
    return _lib.load().pmc_maf_inverse_plan(C.byref(flow._desc), n, algo, fused, C.byref(p)), p


@pytest.mark.gpu
def test_two_identical_calls_give_the_same_bits():
    import torch
    for name in ("o4", "t16", "nsf_d2"):
        flow = _flow(name)
        z = torch.randn(4097, flow.n_dim, generator=torch.Generator().manual_seed(3)).cuda()
        a, b = _inverse(flow, z, AUTO), _inverse(flow, z, AUTO)
        assert a[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FLOWS))
def test_auto_and_triangular_launch_the_sweep_the_plan_names(name):
    import torch
    flow = _flow(name)
    rows = (17, 4097, 8193) if FLOWS[name] == S_LANE else (17,)
    for n in rows:
        rc, p = _plan(flow, n, AUTO)
        assert rc == 0 and p.sweep == FLOWS[name], (n, p.sweep)
        explicit = LANE16 if p.helper_fmt else EXPLICIT[p.sweep]
        z = torch.randn(n, flow.n_dim, generator=torch.Generator().manual_seed(n)).cuda()
        rc_e, x_e, l_e = _inverse(flow, z, explicit)
        rc_a, x_a, l_a = _inverse(flow, z, AUTO)
        assert rc_e == 0 and rc_a == 0
        assert np.isfinite(x_e.view(np.float32)).all() and not (x_e.view(np.float32) == -7.0).any()     # (every row was written)
        assert np.array_equal(x_a, x_e) and np.array_equal(l_a, l_e), n
        rc_p, pt = _plan(flow, n, TRI)
        rc_t, x_t, l_t = _inverse(flow, z, TRI)
        assert (rc_t != 0) == (rc_p != 0), n
        if rc_p == 0:                                    # (TRIANGULAR names a sweep: the D-pass classes have none)
            assert pt.sweep == p.sweep and np.array_equal(x_t, x_e) and np.array_equal(l_t, l_e), n
        else:
            assert p.sweep in (S_DPASS_AFFINE, S_DPASS_SPLINE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FUSED))
def test_the_step_launches_the_fused_instance_the_plan_names(name, monkeypatch):
    """no_fuse = 0 (the plan's fused instance, scaler epilogue included, or none) against no_fuse = 1 (proposal, sweep and
    scaler as launches of their own) with the same variates: u', the flow's log-determinant, x' and the finite mask, bit for
    bit -- as tests/test_gpu_epilogue_rows.py compares the epilogue with the scaler launch."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    flow = _flow(name)
    D, n = flow.n_dim, 21
    rc, p = _plan(flow, n, AUTO, fused=1)
    assert rc == 0 and p.sweep == FUSED[name] and p.epilogue == (1 if p.sweep != S_NONE else 0)
    prior = pc.Prior([uniform(-5, 10)] * D)
    rng = np.random.default_rng(1000 * D + n)
    scaler = pc.Reparameterize(D, bounds=np.array([[-5.0, 5.0]] * D))
    scaler.fit(rng.uniform(-4, 4, size=(2000, D)))
    x = rng.uniform(-4, 4, size=(n, D))
    u = scaler.forward(x)
    # whether the step fused shows in p_theta32: only the proposal launch of its own writes the float32 theta' there (the
    # fused instances propose into LDS)
    from pocomc_amd.mcmc import StepEngine
    engines, propose = [], StepEngine.propose

    def poisoned_propose(self, *args, **kw):
        self.p_theta32.fill_(-7.0)
        engines.append(self)
        return propose(self, *args, **kw)
    monkeypatch.setattr(StepEngine, "propose", poisoned_propose)
    a = _pre_step(monkeypatch, 0, n, D, flow, scaler, prior, x, u)
    b = _pre_step(monkeypatch, 1, n, D, flow, scaler, prior, x, u)
    wrote = [bool((e.p_theta32.cpu().numpy() != -7.0).any()) for e in engines]
    assert wrote == [p.sweep == S_NONE, True]
    for k in ("u32", "ldjf", "x", "finite", "theta"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["done"][0] == 1 and b["done"][0] == 1 and (a["finite"] != 0).sum() >= n - 1
