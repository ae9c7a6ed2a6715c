"""CPU checks of the Lovasz-softmax term's yardsticks and host logic.

The float64 restatement of tests/test_gpu_lovasz.py (`restate`) is pinned here to the reference's own float64 numbers
(tests/golden/lovasz_*.npz, tools/gen_lovasz_golden.py) at 1e-10 relative, loss and gradient, so that the GPU tests compare the kernels
with something that is itself checked. Also: the criteria's constructors and refusals, which need no device."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_gpu_lovasz as G  # noqa: E402


@pytest.mark.parametrize("case", list(G.FIXTURES))
def test_restatement_equals_the_reference_in_float64(case):
    seg, target = G.inputs(case)
    gold = np.load(os.path.join(G.GOLDEN, "lovasz_%s.npz" % case))
    assert np.array_equal(gold["target"].astype(np.int64), target.numpy())
    assert abs(float(seg.double().sum()) - float(gold["seg_sum"])) <= 1e-6
    x = seg.double().requires_grad_(True)
    out = G.restate(x, target)
    out["loss"].backward()
    want = float(gold["loss64"])
    assert abs(float(out["loss"].detach()) - want) <= 1e-10 * abs(want), (float(out["loss"].detach()), want)
    g64 = torch.from_numpy(gold["dseg64"])
    if case != "ties":
        assert float((x.grad - g64).abs().max()) <= 1e-10 * float(g64.abs().max())
    else:
        # exact ties exist in float64 too on this case, the reference's torch.sort is not the stable one, and the gradient (unlike the
        # loss) depends on the order among equal e: the GPU test compares this case's gradient in the kernel's own, validated order
        assert float((x.grad - g64).abs().max()) <= 1e-3 * float(g64.abs().max())
    # the fixture's fp32 numbers are the reference's own fp32 run: close to float64, not equal
    assert gold["dseg32"].dtype == np.float32 and gold["dseg64"].dtype == np.float64 and gold["target"].dtype == np.int16
    assert abs(float(gold["loss32"]) - want) <= 1e-4 * max(1.0, abs(want))
    assert 0.0 < float(gold["R_e"]) < 1e-4


def test_the_given_order_reproduces_the_free_order():
    seg, target = G.inputs("multi")
    free = G.restate(seg, target)
    order = torch.stack([G.stable_order(free["e"][c], free["valid"]) for c in range(seg.shape[1])])
    fixed = G.restate(seg, target, order=order.to(torch.int32))
    assert torch.equal(free["loss"], fixed["loss"]) and free["present"] == 5


def test_cases_do_what_they_are_for():
    for name, ((B, K, h, w, H, W), amp, variant) in G.CASES.items():
        seg, target = G.inputs(name)
        assert seg.shape == (B, K, h, w) and target.shape == (B, H, W)
        valid = (target >= 0) & (target < K)
        present = sorted(set(target[valid].tolist()))
        if name == "tiny":
            assert B * H * W < 64 and bool(valid.all())
        if name == "big":
            assert (B * H * W + 2047) // 2048 >= 3 and (B * H * W) % 2048 != 0
        if name == "absent":
            assert 1 not in present and 4 not in present and len(present) == 4
        if name == "ties":
            assert bool((seg / 2.0 == torch.round(seg / 2.0)).all())
        if name == "void":
            assert bool(valid[0].any()) and not bool(valid[1].any())
        if name == "void_all":
            assert not bool(valid.any())
        if variant is None:
            assert 0.05 < 1.0 - float(valid.double().mean()) < 0.15


def _cfg(**kw):
    return G._cfg("mem_contrast_ce_loss", 5, **kw)


def test_criteria_are_constructed_without_a_device():
    from contrastiveseg_amd.lib.loss.loss_helper import FSAuxCELOVASZLoss, FSAuxCELoss, FSCELOVASZLoss, FSCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    for loss_type, on, off in (("mem_contrast_ce_loss", FSCELOVASZLoss, FSCELoss), ("mem_contrast_auxce_loss", FSAuxCELOVASZLoss, FSAuxCELoss)):
        assert type(SEG_LOSS_DICT[loss_type](G._cfg(loss_type, 5)).seg_criterion) is on
        assert type(SEG_LOSS_DICT[loss_type](G._cfg(loss_type, 5, use_lovasz=False)).seg_criterion) is off
    crit = FSCELOVASZLoss(_cfg(ce_weight=[1.0, 2.0, 0.5, 1.0, 1.0], ce_ignore_index=255))
    assert crit.ignore_index == 255 and crit.ce_loss.weight.tolist() == [1.0, 2.0, 0.5, 1.0, 1.0]
    for reduction in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="ce_reduction"):
            FSCELOVASZLoss(_cfg(ce_reduction=reduction))
    with pytest.raises(NotImplementedError, match="list / tuple"):
        crit([torch.zeros(1, 5, 2, 2)], torch.zeros(1, 4, 4, dtype=torch.int64))
    # the bank-free criteria do not read the key, as in the reference
    for loss_type in ("contrast_ce_loss", "contrast_auxce_loss"):
        cfg = G._cfg(loss_type, 5)
        cfg.get("contrast")["with_memory"] = False
        assert type(SEG_LOSS_DICT[loss_type](cfg).seg_criterion) in (FSCELoss, FSAuxCELoss)


def test_both_switches_are_refused_by_name():
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    rmi = dict(num_classes=5, rmi_radius=3, rmi_pool_way=0, rmi_pool_size=3, rmi_pool_stride=3, loss_weight_lambda=0.5, loss_weight=1.0,
               lambda_way=1, use_sigmoid=False)
    for loss_type in ("mem_contrast_ce_loss", "mem_contrast_auxce_loss"):
        with pytest.raises(NotImplementedError, match="use_lovasz"):
            SEG_LOSS_DICT[loss_type](G._cfg(loss_type, 5, use_rmi=True, **rmi))


def test_binding_refuses_host_tensors_and_bad_shapes():
    from contrastiveseg_amd import kernels as K
    seg, target = G.inputs("tiny")
    with pytest.raises(RuntimeError, match="GPU"):
        K.lovasz_softmax(seg, target)
    with pytest.raises(RuntimeError, match="GPU"):
        K.lovasz_errors(seg, target)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        K.lovasz_softmax(seg, torch.zeros(1, dtype=torch.int64).expand(1, 1 << 16, 1 << 15))
    with pytest.raises(RuntimeError, match="257 classes"):
        K.lovasz_softmax(torch.zeros(1, 257, 3, 3), target)
    with pytest.raises(RuntimeError, match="only upsampling"):
        K.lovasz_softmax(torch.zeros(1, 3, 9, 9), target)
