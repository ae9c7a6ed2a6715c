"""Host side of contrast.device_sampling (no GPU): the switch and its refusals, the export / import of the CPU generator's mt19937
state (csrc_host/rng_draws.cpp), the messages of the status bits."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module", autouse=True)
def host_lib():
    from contrastiveseg_amd.csrc_host import build
    build.build()


def _cfg(loss_type="contrast_ce_loss", **contrast):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    c = {"proj_dim": 16, "temperature": 0.1, "base_temperature": 0.07, "max_samples": 64, "max_views": 10, "loss_weight": 0.1,
         "use_rmi": False}
    c.update(contrast)
    return Configer(config_dict={"data": {"num_classes": 5}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": 8},
                                 "contrast": c,
                                 "loss": {"loss_type": loss_type, "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


def test_default_is_the_host_path_and_the_environment_overrides(monkeypatch):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    monkeypatch.setattr(K, "DEVICE_SAMPLING", None)
    for name in ("contrast_ce_loss", "contrast_auxce_loss"):
        assert SEG_LOSS_DICT[name](_cfg(name)).contrast_criterion.device_sampling is False
        assert SEG_LOSS_DICT[name](_cfg(name, device_sampling=True)).contrast_criterion.device_sampling is True
    monkeypatch.setattr(K, "DEVICE_SAMPLING", "1")
    assert SEG_LOSS_DICT["contrast_ce_loss"](_cfg()).contrast_criterion.device_sampling is True
    monkeypatch.setattr(K, "DEVICE_SAMPLING", "0")
    assert SEG_LOSS_DICT["contrast_ce_loss"](_cfg(device_sampling=True)).contrast_criterion.device_sampling is False
    crit = SEG_LOSS_DICT["contrast_ce_loss"](_cfg())
    assert not any("rng" in k or "sampling" in k for k in crit.state_dict())      # state_dict keys stay the reference's


@pytest.mark.parametrize("name", ["mem_contrast_ce_loss", "mem_contrast_auxce_loss"])
def test_memory_bank_criteria_refuse_by_name(name, monkeypatch):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    monkeypatch.setattr(K, "DEVICE_SAMPLING", None)
    SEG_LOSS_DICT[name](_cfg(name, with_memory=True, memory_size=8, pixel_update_freq=2))            # off: builds
    with pytest.raises(NotImplementedError, match="device_sampling"):
        SEG_LOSS_DICT[name](_cfg(name, with_memory=True, memory_size=8, pixel_update_freq=2, device_sampling=True))


def test_cross_rank_refuses_by_name(monkeypatch):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss import loss_contrast
    monkeypatch.setattr(K, "DEVICE_SAMPLING", None)
    crit = loss_contrast.PixelContrastLoss(_cfg(device_sampling=True, cross_rank=True))
    monkeypatch.setattr(loss_contrast.D, "exercise_single_rank", lambda: True)               # CSEG_DIST_SINGLE_RANK=1 in a process group
    feats, labels, seg = torch.zeros(1, 16, 4, 4), torch.zeros(1, 8, 8, dtype=torch.long), torch.zeros(1, 5, 4, 4)
    with pytest.raises(NotImplementedError, match="device_sampling"):
        crit(feats, labels, seg=seg)
    monkeypatch.setattr(loss_contrast.D, "exercise_single_rank", lambda: False)
    monkeypatch.setattr(loss_contrast.D, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="device_sampling"):
        crit(feats, labels, seg=seg)


def test_export_of_a_fresh_seed_and_round_trip():
    from contrastiveseg_amd import _host
    torch.manual_seed(304)
    words = _host.mt_export()
    assert words.dtype == np.uint32 and words.shape == (625,)
    assert words[624] == 624 and words[0] == 304          # "regenerate first"; init_genrand(s): state[0] = s
    want = torch.randperm(50)
    after = _host.mt_export()
    assert after[624] == 49                               # 49 draws: the first one regenerated, pos = 49
    _host.mt_import(words)
    assert torch.equal(torch.randperm(50), want)
    # export -> import is the identity, anywhere in the stream (here across a regeneration)
    torch.randperm(700)
    mid = _host.mt_export()
    _host.mt_import(mid)
    assert np.array_equal(_host.mt_export(), mid)
    want = torch.randperm(777)
    _host.mt_import(mid)
    assert torch.equal(torch.randperm(777), want)
    with pytest.raises(RuntimeError, match="pos"):
        _host.mt_import(np.zeros(625, dtype=np.uint32))


def test_without_the_helper_library_device_sampling_raises(monkeypatch):
    from contrastiveseg_amd import _host, kernels as K
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    monkeypatch.setattr(K, "DEVICE_SAMPLING", None)
    monkeypatch.setattr(_host, "_lib", None)
    monkeypatch.setattr(_host, "_tried", True)             # what CSEG_NO_HOST_LIB or a missing libcseg_host.so leaves behind
    with pytest.raises(RuntimeError, match="libcseg_host"):
        _host.mt_export()
    crit = PixelContrastLoss(_cfg(device_sampling=True))
    with pytest.raises(RuntimeError, match="device_sampling"):
        crit._rng_on(torch.device("cpu"))


def test_status_messages():
    from contrastiveseg_amd.lib.loss.anchor_sampling import sampling_status_messages as msgs
    assert msgs(0) == []
    assert len(msgs(1)) == 1 and "num_classes" in msgs(1)[0]
    assert "max_views=10" in msgs(2, max_samples=64, max_views=10)[0]
    assert "max_samples=64" in msgs(4, max_samples=64, max_views=10)[0]
    assert "never touched" in msgs(8)[0]
    assert len(msgs(15, 64, 10)) == 4 and msgs(6, 64, 10) == msgs(2, 64, 10) + msgs(4, 64, 10)
