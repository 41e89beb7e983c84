"""The reference the bf16 spline trainer is held to (``tests/bf16_spline_train_model.py``), on the CPU: on the nine cases
of the GPU test the float32 evaluation of the model passes the criterion and the yardstick's own shares, every single
structural defect fails it, and with the rounding switched off the model is ``oracle.maf.torch_loss``.

Not claimed: a rounding LEFT OUT in the backward pass (``dphi`` or ``da2`` stored unrounded) lies at 0.02 - 0.14 of
``d_round``, inside the yardstick's own range at the wide shapes; a value left unrounded is harmless and no norm criterion
sees it."""
import numpy as np
import pytest
import torch

import bf16_spline_train_model as tm


def _id(case):
    return "D%d-T%d-H%d-K%d-n%d-%s-s%g" % (case[0], case[1], case[2], case[3], case[4], "w" if case[5] else "u", case[6])


@pytest.mark.parametrize("case", tm.CASES, ids=_id)
def test_float32_model_passes_the_criterion_and_the_yardstick_shares(case):
    r = tm.case_reference(case)
    v = tm.verdict(r["spec"], r["lossT32"], r["gT32"], r)
    d_round = np.linalg.norm(r["gT64"] - r["g64"])
    print(f"{_id(case)}: d_round / |g| {d_round / np.linalg.norm(r['g64']):.1e}, yardstick overall {v['overall']:.1e}, "
          f"worst tensor {v['worst']:.1e} {v['where']}, loss {v['loss_rel']:.1e}")
    assert d_round > 0.0
    assert v["ok"], v
    assert v["overall"] <= tm.YARD_OVERALL and v["worst"] <= tm.YARD_PER_TENSOR, v


@pytest.mark.parametrize("defect", tm.DEFECTS)
@pytest.mark.parametrize("case", tm.CASES, ids=_id)
def test_every_structural_defect_fails_the_criterion(case, defect):
    r = tm.case_reference(case)
    loss, g = tm.loss_and_gradient(r["spec"], r["flat"], r["x"], r["w"], dtype=torch.float32, defect=defect)
    v = tm.verdict(r["spec"], loss, g, r)
    print(f"{_id(case)} {defect}: overall {v['overall']:.2f}, worst tensor {v['worst']:.2f}, loss {v['loss_rel']:.1e}")
    assert not v["ok"], v
    assert v["overall"] > tm.OVERALL or v["worst"] > tm.PER_TENSOR      # (rejected by the gradient, not by the loss alone)


@pytest.mark.parametrize("case", tm.CASES, ids=_id)
def test_model_without_rounding_is_the_oracle_loss(case):
    r = tm.case_reference(case)
    loss, g = tm.loss_and_gradient(r["spec"], r["flat"], r["x"], r["w"], rounding=False)
    assert abs(loss - r["loss64"]) <= 1e-12 * abs(r["loss64"])
    assert np.linalg.norm(g - r["g64"]) <= 1e-12 * np.linalg.norm(r["g64"])
    assert np.all(g[r["spec"].mask_flat() == 0] == 0.0)
