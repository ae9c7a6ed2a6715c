"""CPU checks of the OHEM cross entropy's yardsticks and host logic.

The float64 restatement of tests/test_gpu_ohem.py (`restate`) is pinned here to the reference's own float64 numbers
(tests/golden/ohem_*.npz, tools/gen_ohem_golden.py) at 1e-10 relative -- loss, gradient, threshold and kept set -- so that the GPU tests
compare the kernels with something that is itself checked. Also: the registry keys, the wiring of contrast.use_ohem, the constructors'
refusals and the shipped OHEM config, which need no device."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_gpu_ohem as G  # noqa: E402


@pytest.mark.parametrize("case", list(G.FIXTURES))
def test_restatement_equals_the_reference_in_float64(case):
    seg, target, weight = G.inputs(case)
    _, _, _, thresh, min_kept, _ = G.CASES[case]
    gold = np.load(os.path.join(G.GOLDEN, "ohem_%s.npz" % case))
    assert np.array_equal(gold["target"].astype(np.int64), target.numpy())
    assert abs(float(seg.double().sum()) - float(gold["seg_sum"])) <= 1e-6
    x = seg.double().requires_grad_(True)
    out = G.restate(x, target, weight, thresh, min_kept)
    out["loss"].backward()
    want = float(gold["loss64"])
    assert abs(float(out["loss"].detach()) - want) <= 1e-10 * abs(want), (float(out["loss"].detach()), want)
    g64 = torch.from_numpy(gold["dseg64"])
    assert float((x.grad - g64).abs().max()) <= 1e-10 * float(g64.abs().max())
    # the threshold: the k-th probability to 1e-10; on the threshold branch the restatement compares with fp32(thresh), as the fp32
    # reference does, and the float64 reference with the double -- no probability lies between the two (the generator's gap check)
    tol = 1e-10 if case in G.KTH_BRANCH else 2.0 ** -24
    assert abs(float(out["thr"]) - float(gold["thr64"])) <= tol and abs(float(gold["thr32"]) - float(gold["thr64"])) <= 1e-5
    kept64 = np.unpackbits(gold["kept64"])[:target.numel()].astype(bool).reshape(target.shape)
    assert np.array_equal(out["kept"].numpy(), kept64) and np.array_equal(gold["kept32"], gold["kept64"])
    # the fixture's fp32 numbers are the reference's own fp32 run: close to float64, not equal
    assert gold["dseg32"].dtype == np.float32 and gold["dseg64"].dtype == np.float64 and gold["target"].dtype == np.int16
    assert abs(float(gold["loss32"]) - want) <= 1e-4 * max(1.0, abs(want))
    assert 0.0 < float(gold["R_p"]) < 1e-4


def test_cases_do_what_they_are_for():
    for name, ((B, K, h, w, H, W), amp, boost, thresh, min_kept, variant) in G.CASES.items():
        seg, target, weight = G.inputs(name)
        assert seg.shape == (B, K, h, w) and target.shape == (B, H, W) and weight.tolist() == pytest.approx([1 + 0.1 * c for c in range(K)])
        r = G.restate(seg, target, weight, thresh, min_kept)
        kth_wins = r["n"] > 0 and float(r["thr"]) > thresh
        assert kth_wins == (name in G.KTH_BRANCH + ("ties", "narrow", "confident")), name
        if name == "tiny":
            assert B * H * W < 64 and bool(r["valid"].all())
        if name == "all":
            assert min_kept >= r["n"] and r["k"] == r["n"] - 1 and int(r["kept"].sum()) == r["n"] - 1
        if name == "big":
            assert B * H * W > 4 * 2048
        if name == "ties":
            assert bool((seg / 2.0 == torch.round(seg / 2.0)).all())
        if name == "void":
            assert bool(r["valid"][0].any()) and not bool(r["valid"][1].any())
        if name == "void_all":
            assert r["n"] == 0 and r["k"] == 0
        if name == "confident":
            assert r["n"] > 0 and int(r["kept"].sum()) == 0 and bool(torch.isnan(r["loss"]))
        if variant is None:
            assert 0.05 < 1.0 - float(r["valid"].double().mean()) < 0.15


def test_fp32_threshold_comparison_is_the_pinned_one():
    """`p < thr` happens in fp32 with ohem_thresh rounded to fp32: 0.9 itself is not below it, its fp32 predecessor is."""
    t = torch.tensor(0.9, dtype=torch.float32)
    assert not bool(t < 0.9) and bool(torch.nextafter(t, torch.tensor(0.0)) < 0.9)


def test_registry_and_wiring():
    from contrastiveseg_amd.lib.loss import loss_helper as H
    from contrastiveseg_amd.lib.loss.loss_contrast import SEG_CRITERIA
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    assert SEG_LOSS_DICT["fs_ohemce_loss"] is H.FSOhemCELoss and SEG_LOSS_DICT["fs_auxohemce_loss"] is H.FSAuxOhemCELoss
    assert SEG_CRITERIA[False]["ohem"] is H.FSOhemCELoss and SEG_CRITERIA[True]["ohem"] is H.FSAuxOhemCELoss
    assert issubclass(H.FSOhemCELoss, H.FSCELoss), "bad_label_total finds its status through FSCELoss"
    crit = H.FSOhemCELoss(G._cfg("fs_ohemce_loss", 5, ce_weight=[1.0, 2.0, 0.5, 1.0, 1.0], ce_ignore_index=255, ohem_minkeep=-3))
    assert crit.ignore_index == 255 and crit.weight.tolist() == [1.0, 2.0, 0.5, 1.0, 1.0] and crit.min_kept == 1 and crit.thresh == 0.7
    aux = H.FSAuxOhemCELoss(G._cfg("fs_auxohemce_loss", 5))
    assert type(aux.ohem_ce_loss) is H.FSOhemCELoss and type(aux.ce_loss) is H.FSCELoss
    for loss_type in ("contrast_ce_loss", "contrast_auxce_loss", "mem_contrast_ce_loss", "mem_contrast_auxce_loss"):
        on, off = (H.FSAuxOhemCELoss, H.FSAuxCELoss) if "aux" in loss_type else (H.FSOhemCELoss, H.FSCELoss)
        assert type(SEG_LOSS_DICT[loss_type](G._cfg(loss_type, 5)).seg_criterion) is on
        assert type(SEG_LOSS_DICT[loss_type](G._cfg(loss_type, 5, use_ohem=False)).seg_criterion) is off
        assert type(SEG_LOSS_DICT[loss_type](G._cfg(loss_type, 5, use_ohem=None, ohem_thresh=None)).seg_criterion) is off


def test_refusals_need_no_device():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import FSOhemCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    with pytest.raises(NotImplementedError, match="ce_reduction"):
        FSOhemCELoss(G._cfg("fs_ohemce_loss", 5, ce_reduction="sum"))
    with pytest.raises(KeyError, match="ohem_thresh"):
        FSOhemCELoss(G._cfg("fs_ohemce_loss", 5, ohem_thresh=None))
    with pytest.raises(NotImplementedError, match="use_ohem together with contrast.use_lovasz"):
        SEG_LOSS_DICT["mem_contrast_ce_loss"](G._cfg("mem_contrast_ce_loss", 5, use_lovasz=True))
    seg, target, _ = G.inputs("tiny")
    with pytest.raises(RuntimeError, match="GPU"):
        K.ohem_ce(seg, target)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        K.ohem_ce(seg, torch.zeros(1, dtype=torch.int64).expand(1, 1 << 16, 1 << 15))
    with pytest.raises(RuntimeError, match="only upsampling"):
        K.ohem_ce(torch.zeros(1, 3, 9, 9), target)


def test_the_shipped_ohem_config_builds_its_criterion():
    from contrastiveseg_amd.lib.loss.loss_helper import FSOhemCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import LossManager
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    path = os.path.join(ROOT, "configs", "cityscapes", "H_48_D_4_OHEM.json")
    cfg, base = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "cityscapes", "H_48_D_4.json")))
    assert cfg["contrast"].pop("use_ohem") is True and cfg["loss"]["params"].pop("ohem_thresh") == 0.9
    assert cfg["loss"]["params"].pop("ohem_minkeep") == 100000 and cfg == base, "H_48_D_4.json plus the three keys, nothing else"
    crit = LossManager(Configer(config_dict=json.load(open(path)))).get_seg_loss()
    assert type(crit.seg_criterion) is FSOhemCELoss and crit.seg_criterion.thresh == 0.9 and crit.seg_criterion.min_kept == 100000
    assert crit.seg_criterion.weight.numel() == 19
