"""The four registered contrast criteria are one composite (lib/loss/loss_contrast.py::_ContrastComposite) with other data
(DESIGN.md section 22): which segmentation criterion every accepted term switch gives, the two refusals, and the label check
Trainer._display makes through loss_helper.bad_label_total -- which used to raise for every criterion built with contrast.use_lovasz
(FSCELOVASZLoss has a bad_label_count but no status buffer of its own)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

NCLS, D = 5, 16
RMI = dict(num_classes=NCLS, rmi_radius=3, rmi_pool_way=0, rmi_pool_size=3, rmi_pool_stride=3, loss_weight_lambda=0.5, loss_weight=1.0,
           lambda_way=1, use_sigmoid=False)
MEMORY = dict(with_memory=True, memory_size=8, pixel_update_freq=2)


def _cfg(loss_type, **contrast):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    c = dict(proj_dim=D, temperature=0.1, base_temperature=0.07, max_samples=64, max_views=4, loss_weight=0.1, use_rmi=False)
    if loss_type.startswith("mem"):
        c.update(MEMORY)
    c.update(contrast)
    params = {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}
    if c["use_rmi"]:
        params.update(RMI)
    return Configer(config_dict={"data": {"num_classes": NCLS}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": 4},
                                 "contrast": c, "loss": {"loss_type": loss_type, "params": params}})


def test_term_table_refusals_label_check_and_the_kernel_module_swap():
    from contrastiveseg_amd.lib.loss import loss_contrast, loss_contrast_mem, loss_helper as H
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    # (criterion, switches) -> segmentation criterion; the bank-free pair has no use_lovasz switch and does not look at it
    table = {
        "contrast_ce_loss": [({}, H.FSCELoss), ({"use_rmi": True}, H.FSRMILoss), ({"use_lovasz": True}, H.FSCELoss),
                             ({"use_rmi": True, "use_lovasz": True}, H.FSRMILoss)],
        "contrast_auxce_loss": [({}, H.FSAuxCELoss), ({"use_rmi": True}, H.FSAuxRMILoss), ({"use_lovasz": True}, H.FSAuxCELoss),
                                ({"use_rmi": True, "use_lovasz": True}, H.FSAuxRMILoss)],
        "mem_contrast_ce_loss": [({}, H.FSCELoss), ({"use_lovasz": False}, H.FSCELoss), ({"use_rmi": True}, H.FSRMILoss),
                                 ({"use_lovasz": True}, H.FSCELOVASZLoss)],
        "mem_contrast_auxce_loss": [({}, H.FSAuxCELoss), ({"use_lovasz": False}, H.FSAuxCELoss), ({"use_rmi": True}, H.FSAuxRMILoss),
                                    ({"use_lovasz": True}, H.FSAuxCELOVASZLoss)],
    }
    assert sorted(table) == sorted(n for n in SEG_LOSS_DICT if "contrast" in n)
    for name, rows in table.items():
        mem = name.startswith("mem")
        module = loss_contrast_mem if mem else loss_contrast
        assert SEG_LOSS_DICT[name] is (module.ContrastAuxCELoss if "aux" in name else module.ContrastCELoss)
        for switches, want in rows:
            crit = SEG_LOSS_DICT[name](_cfg(name, **switches))
            assert type(crit.seg_criterion) is want, (name, switches)
            assert type(crit.contrast_criterion) is module.PixelContrastLoss and crit.contrast_criterion.uses_memory_bank is mem
            assert crit.loss_weight == 0.1 and bool(crit.use_rmi) == bool(switches.get("use_rmi")) and crit.configer is not None
            assert hasattr(crit, "use_lovasz") == mem and (not mem or bool(crit.use_lovasz) == bool(switches.get("use_lovasz")))
            assert list(crit.state_dict()) == []
            bad = H.bad_label_total(crit)
            assert torch.is_tensor(bad) and bad.dtype == torch.int32 and bad.dim() == 0 and int(bad) == 0, (name, switches)
        if mem:
            with pytest.raises(NotImplementedError, match="use_lovasz"):
                SEG_LOSS_DICT[name](_cfg(name, use_rmi=True, use_lovasz=True))
    # oracle/cpu_port.install swaps the attribute `K` of the three loss modules (bench.py's CPU leg relies on it) and puts it back
    from contrastiveseg_amd import kernels
    from oracle import cpu_port
    mods = (loss_contrast, loss_contrast_mem, H)
    assert all(m.K is kernels for m in mods)
    restore = cpu_port.install()
    try:
        assert all(m.K is cpu_port for m in mods)
    finally:
        restore()
    assert all(m.K is kernels for m in mods)


def _check_label_total_on_the_validation_path(dev):
    """mem_contrast_[aux]ce_loss with use_lovasz, `preds` without queues (the validation pass: no mining, so a label outside
    [0, num_classes) is not refused there): 1 x 5 x 4 x 4 logits, 8 x 8 labels, three of them num_classes + 2."""
    from contrastiveseg_amd.lib.loss.loss_helper import bad_label_total
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    g = torch.Generator().manual_seed(41)
    seg = torch.randn(1, NCLS, 4, 4, generator=g) * 2.0
    aux = torch.randn(1, NCLS, 4, 4, generator=g) * 2.0
    embed = F.normalize(torch.randn(1, D, 4, 4, generator=g), dim=1)
    target = torch.randint(0, NCLS, (1, 8, 8), generator=g)
    where = ([0, 0, 0], [0, 3, 7], [1, 5, 7])
    for name in ("mem_contrast_ce_loss", "mem_contrast_auxce_loss"):
        for value in (NCLS + 2, -1):
            labels = target.clone()
            labels[where] = value
            crit = SEG_LOSS_DICT[name](_cfg(name, use_lovasz=True)).to(dev)
            preds = {"seg": seg.to(dev), "embed": embed.to(dev)}
            if "aux" in name:
                preds["seg_aux"] = aux.to(dev)
            with torch.no_grad():
                loss = crit(preds, labels.to(dev), with_embed=True)
            bad = bad_label_total(crit, loss.device)
            assert bad.dtype == torch.int32 and bad.dim() == 0 and bad.device == loss.device
            print(name, value, float(loss), int(bad))
            assert np.isfinite(float(loss)), (name, value)
            assert (int(bad) > 0) if value == NCLS + 2 else (int(bad) == 0), (name, value, int(bad))


def test_label_total_of_the_lovasz_memory_criteria_on_the_emulated_device(monkeypatch):
    from tests.emu import inject
    inject.install(monkeypatch)
    _check_label_total_on_the_validation_path(torch.device("cpu"))


@pytest.mark.gpu
def test_label_total_of_the_lovasz_memory_criteria_on_the_mi355x():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _check_label_total_on_the_validation_path(torch.device("cuda:0"))
