"""Host side of contrast.device_bank (no GPU): the switch and its environment override, what stays refused, the three refusals of the
device route by name, the state_dict keys."""
import pytest
import torch

MEM = ["mem_contrast_ce_loss", "mem_contrast_auxce_loss"]


@pytest.fixture(scope="module", autouse=True)
def host_lib():
    from contrastiveseg_amd.csrc_host import build
    build.build()


@pytest.fixture(autouse=True)
def no_environment(monkeypatch):
    from contrastiveseg_amd import kernels as K
    monkeypatch.setattr(K, "DEVICE_SAMPLING", None)
    monkeypatch.setattr(K, "DEVICE_BANK", None)


def _cfg(loss_type="mem_contrast_ce_loss", **contrast):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    c = {"proj_dim": 16, "temperature": 0.1, "base_temperature": 0.07, "max_samples": 64, "max_views": 10, "loss_weight": 0.1,
         "use_rmi": False, "with_memory": True, "memory_size": 8, "pixel_update_freq": 2}
    c.update(contrast)
    return Configer(config_dict={"data": {"num_classes": 5}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": 8},
                                 "contrast": c,
                                 "loss": {"loss_type": loss_type, "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


def _build(name, **contrast):
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    return SEG_LOSS_DICT[name](_cfg(name, **contrast))


@pytest.mark.parametrize("name", MEM)
def test_default_is_off_and_the_environment_overrides_in_both_directions(name, monkeypatch):
    from contrastiveseg_amd import kernels as K
    assert _build(name).contrast_criterion.device_bank is False
    assert _build(name, device_bank=False).contrast_criterion.device_bank is False
    assert _build(name, device_bank=True).contrast_criterion.device_bank is True
    monkeypatch.setattr(K, "DEVICE_BANK", "1")
    assert _build(name).contrast_criterion.device_bank is True
    monkeypatch.setattr(K, "DEVICE_BANK", "0")
    assert _build(name, device_bank=True).contrast_criterion.device_bank is False


def test_the_environment_variable_is_read_like_device_sampling():
    import subprocess
    import sys
    code = "from contrastiveseg_amd import kernels as K; print(repr(K.DEVICE_BANK), repr(K.DEVICE_SAMPLING))"
    root = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    env = dict(__import__("os").environ, CSEG_DEVICE_BANK="1")
    env.pop("CSEG_DEVICE_SAMPLING", None)
    out = subprocess.check_output([sys.executable, "-c", code], cwd=root, env=env).decode().split()
    assert out[-2:] == ["'1'", "None"]


@pytest.mark.parametrize("name", ["contrast_ce_loss", "contrast_auxce_loss"])
def test_the_bank_free_criteria_ignore_the_switch(name, monkeypatch):
    from contrastiveseg_amd import kernels as K
    crit = _build(name, device_bank=True).contrast_criterion
    assert crit.device_bank is False and crit.device_sampling is False
    monkeypatch.setattr(K, "DEVICE_BANK", "1")
    crit = _build(name).contrast_criterion
    assert crit.device_bank is False and crit.device_sampling is False


@pytest.mark.parametrize("name", MEM)
def test_device_sampling_alone_still_raises_on_a_memory_bank_criterion(name, monkeypatch):
    from contrastiveseg_amd import kernels as K
    with pytest.raises(NotImplementedError, match="device_sampling"):
        _build(name, device_sampling=True)
    with pytest.raises(NotImplementedError, match="device_sampling"):
        _build(name, device_sampling=True, device_bank=False)
    monkeypatch.setattr(K, "DEVICE_SAMPLING", "1")
    with pytest.raises(NotImplementedError, match="device_sampling"):
        _build(name)
    crit = _build(name, device_bank=True).contrast_criterion              # lifted only when device_bank is wanted
    assert crit.device_bank is True


@pytest.mark.parametrize("name", MEM)
def test_refusals_by_name(name, monkeypatch):
    from contrastiveseg_amd.lib.loss import loss_contrast
    with pytest.raises(ValueError, match="device_bank.*pixel_update_freq"):
        _build(name, device_bank=True, pixel_update_freq=9)                 # > memory_size = 8
    _build(name, device_bank=True, pixel_update_freq=8)
    _build(name, pixel_update_freq=9)                                       # off: builds as before
    with pytest.raises(ValueError, match="device_bank.*max_samples"):
        _build(name, device_bank=True, max_samples=81)                      # > 5 * 2 * 8 bank columns
    _build(name, device_bank=True, max_samples=80)
    _build(name, max_samples=81)
    monkeypatch.setattr(loss_contrast.D, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="device_bank"):
        _build(name, device_bank=True)
    monkeypatch.setattr(loss_contrast.D, "get_world_size", lambda: 1)
    monkeypatch.setattr(loss_contrast.D, "exercise_single_rank", lambda: True)          # CSEG_DIST_SINGLE_RANK=1 in a process group
    with pytest.raises(NotImplementedError, match="device_bank"):
        _build(name, device_bank=True)


def test_multi_rank_is_refused_on_the_first_call_too(monkeypatch):
    """A process group that comes up after the criterion was built: the criterion and the trainer's enqueue both refuse."""
    from contrastiveseg_amd.lib.loss import loss_contrast
    from contrastiveseg_amd.segmentor import trainer_contrastive as T
    crit = _build("mem_contrast_ce_loss", device_bank=True)
    feats, labels, seg = torch.zeros(1, 16, 4, 4), torch.zeros(1, 8, 8, dtype=torch.long), torch.zeros(1, 5, 4, 4)
    queues = torch.zeros(5, 8, 16), torch.zeros(5, 8, 16)
    monkeypatch.setattr(loss_contrast.D, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="device_bank"):
        crit.contrast_criterion(feats, labels, seg=seg, segment_queue=queues[0], pixel_queue=queues[1])
    me = T.Trainer.__new__(T.Trainer)
    me.network_stride, me.memory_size, me.pixel_update_freq, me.pixel_loss = 2, 8, 2, crit
    assert me._device_bank_criterion() is crit.contrast_criterion
    monkeypatch.setattr(T, "get_world_size", lambda: 2)
    ptr = torch.zeros(5, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="device_bank"):
        me._dequeue_and_enqueue(feats, labels, queues[0], ptr, queues[1], ptr.clone())


def test_without_the_helper_library_device_bank_raises(monkeypatch):
    from contrastiveseg_amd import _host
    monkeypatch.setattr(_host, "_lib", None)
    monkeypatch.setattr(_host, "_tried", True)             # what CSEG_NO_HOST_LIB or a missing libcseg_host.so leaves behind
    crit = _build("mem_contrast_ce_loss", device_bank=True).contrast_criterion
    with pytest.raises(RuntimeError, match="libcseg_host"):
        crit._rng_on(torch.device("cpu"))


@pytest.mark.parametrize("name", MEM)
def test_state_dict_keys_are_unchanged(name):
    off, on = _build(name), _build(name, device_bank=True)
    assert list(on.state_dict()) == list(off.state_dict())
    assert not any("rng" in k or "sampling" in k or "bank" in k for k in on.state_dict())
    assert not list(on.contrast_criterion.buffers())


def test_the_new_entry_points_are_declared_and_bound():
    import os
    import re
    from contrastiveseg_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(cseg_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "cseg_hip.h")).read()))
    for name in ("cseg_contrast_fwd_dn_bank", "cseg_contrast_bwd_dn_bank", "cseg_contrast_bwd_parts_cap_bank",
                 "cseg_scatter_anchor_grad_dn_bank", "cseg_queue_enqueue_device", "cseg_queue_enqueue_ws_ints"):
        assert name in declared and name in _hip.SIGNATURES, name
