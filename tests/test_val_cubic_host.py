"""Host side of val.score_resize (segmentor/trainer_contrastive.py, lib/datasets/data_loader.py), no GPU: the key's parsing and its
refusals, the celeba refusal, the label files of the val loader from stacked and packed raw batches, and that 'bilinear' and an absent
key never reach kernels.cubic_argmax. The kernel and the cubic pass itself: tests/test_gpu_val_cubic.py, tests/test_emu_val_cubic.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**val_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    cfg.get("train", "data_transformer")["input_size"] = [64, 48]
    cfg.update(["train", "batch_size"], 2)
    cfg.update(["contrast", "max_views"], 1)
    cfg.params_root.pop("checkpoints", None)
    for k, v in val_keys.items():
        cfg.add(["val", k], v)
    return cfg


def test_the_key_parses_to_bilinear_by_default():
    from contrastiveseg_amd.segmentor.trainer_contrastive import SCORE_RESIZES, val_score_resize
    assert SCORE_RESIZES == ("bilinear", "cubic")
    assert val_score_resize(_cfg()) == "bilinear"
    assert val_score_resize(_cfg(score_resize="bilinear")) == "bilinear"
    assert val_score_resize(_cfg(score_resize="cubic")) == "cubic"


@pytest.mark.parametrize("value", ["bicubic", "Cubic", "", None, 3, True])
def test_any_other_value_is_refused_when_the_trainer_is_built(value):
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer, val_score_resize
    with pytest.raises(ValueError, match=r"val\.score_resize .*'bilinear', 'cubic'"):
        val_score_resize(_cfg(score_resize=value))
    with pytest.raises(ValueError, match=r"val\.score_resize"):
        Trainer(_cfg(score_resize=value), train_loader=[])


def test_celeba_with_cubic_is_refused_by_name():
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer, val_score_resize
    cfg = _cfg(score_resize="cubic")
    cfg.update(["dataset"], "celeba")
    with pytest.raises(NotImplementedError, match="celeba"):
        val_score_resize(cfg)
    with pytest.raises(NotImplementedError, match="celeba"):
        Trainer(cfg, train_loader=[])
    for keys in ({}, {"score_resize": "bilinear"}):            # the default pass keeps taking celeba
        cfg = _cfg(**keys)
        cfg.update(["dataset"], "celeba")
        assert val_score_resize(cfg) == "bilinear"
    cfg = _cfg(score_resize="cubic")
    cfg.update(["dataset"], "lip")
    assert val_score_resize(cfg) == "cubic"


@pytest.mark.parametrize("keys", [{}, {"score_resize": "bilinear"}], ids=["absent", "bilinear"])
def test_the_bilinear_pass_never_touches_cubic_argmax(keys, monkeypatch):
    """Device half of the model = oracle/cpu_port.py; the confusion matrix is the torch composition's, as it always was."""
    from oracle import cpu_port
    cpu_port.install(monkeypatch)
    from contrastiveseg_amd import kernels
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer

    def boom(*a, **k):
        raise AssertionError("the bilinear validation pass called cubic_argmax")
    monkeypatch.setattr(kernels, "cubic_argmax", boom)
    monkeypatch.setattr(cpu_port, "cubic_argmax", boom, raising=False)
    monkeypatch.delenv("CSEG_VAL_FUSED", raising=False)
    cfg = _cfg(**keys)
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    assert tr.score_resize == "bilinear"
    batches = list(SyntheticLoader(cfg, torch.device("cpu"), length=2, mode="blocky", fixed=False))
    tr.validate(batches)
    got = tr.last_val_score.confusion_matrix
    n = got.shape[0]
    want = torch.zeros(n, n, dtype=torch.int64)
    tr.seg_net.eval()
    with torch.no_grad():
        for b in batches:
            seg = tr.seg_net(b["img"], is_eval=True)["seg"]
            pred = F.interpolate(seg, size=b["labelmap"].shape[-2:], mode="bilinear", align_corners=True).argmax(1)
            t = b["labelmap"]
            want += torch.bincount(n * t[t >= 0] + pred[t >= 0], minlength=n * n).reshape(n, n)
    assert torch.equal(got, want) and int(got.sum()) > 0


def _loader_cfg(**val_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    ids = [3, 7, 9, 11, 20]
    val = dict({"batch_size": 2, "data_transformer": {"size_mode": "fix_size", "input_size": [96, 64], "align_method": "only_pad"}},
               **val_keys)
    train = {"batch_size": 2, "data_transformer": {"size_mode": "fix_size", "input_size": [96, 64], "align_method": "only_pad"}}
    return Configer(config_dict={"data": {"label_list": ids, "num_classes": 5}, "train": train, "val": val,
                                 "train_trans": {"trans_seq": []}, "val_trans": {"trans_seq": []}}), ids


def test_only_the_cubic_val_loader_carries_the_label_files():
    from contrastiveseg_amd.lib.datasets.data_loader import GPUAugLoader
    cpu = torch.device("cpu")
    cfg, ids = _loader_cfg(score_resize="cubic")
    assert GPUAugLoader(cfg, [], cpu, "val").with_ori and not GPUAugLoader(cfg, [], cpu, "train").with_ori
    for keys in ({}, {"score_resize": "bilinear"}):
        assert not GPUAugLoader(_loader_cfg(**keys)[0], [], cpu, "val").with_ori


@pytest.mark.parametrize("reduce_zero", [False, True])
def test_label_files_go_through_the_encoding_table_alone(reduce_zero):
    """The reference's ori_target (lib/datasets/loader/default_loader.py:51-58): _encode_label, _reduce_zero_label, 255 -> -1, at the
    file's size; from a stacked batch and from a packed one."""
    from contrastiveseg_amd.lib.datasets.data_loader import GPUAugLoader
    cfg, ids = _loader_cfg(score_resize="cubic")
    if reduce_zero:
        cfg.add(["data", "reduce_zero_label"], True)
    loader = GPUAugLoader(cfg, [], torch.device("cpu"), "val")
    rs = np.random.RandomState(304)
    raws = [rs.choice(np.array(ids + [0, 255], np.uint8), size=s) for s in ((5, 7), (4, 9))]

    def reference(lab):
        enc = np.full(lab.shape, 255.0, np.float32)            # _encode_label
        for i, cid in enumerate(ids):
            enc[lab == cid] = i
        enc = enc.astype(np.uint8)
        if reduce_zero:
            enc = (enc.astype(np.int64) - 1).astype(np.uint8)   # _reduce_zero_label: uint8 wrap, 0 -> 255
        out = enc.astype(np.int64)
        out[out == 255] = -1
        return out

    def scored(lab):
        # with both keys the reference's ignore value leaves the uint8 shift as 254, a label RunningScore masks like -1 (not a
        # class); the transform's table keeps such pixels at ignore. What is scored is the same, and that is what is compared.
        return np.where((lab < 0) | (lab >= len(ids)), -1, lab)

    packed = torch.from_numpy(np.concatenate([r.reshape(-1) for r in raws]))
    got = loader._ori_labels(packed, [(7, 5), (9, 4)])
    assert [tuple(g.shape) for g in got] == [(5, 7), (4, 9)] and all(g.dtype == torch.int64 for g in got)
    for g, r in zip(got, raws):
        assert np.array_equal(g.numpy(), scored(reference(r)))
        assert reduce_zero or np.array_equal(g.numpy(), reference(r))
    same = np.stack([raws[0], raws[0][::-1].copy()])
    got = loader._ori_labels(torch.from_numpy(same), None)
    assert len(got) == 2 and np.array_equal(got[1].numpy(), scored(reference(same[1])))


def test_score_cubic_refuses_mismatched_batches_before_any_kernel():
    from contrastiveseg_amd.segmentor.trainer_contrastive import score_cubic
    seg = torch.zeros(2, 3, 4, 4)
    hist = torch.zeros(3, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="3 targets for the 2 images"):
        score_cubic(seg, torch.zeros(3, 8, 8, dtype=torch.int64), hist)
    with pytest.raises(ValueError, match="1 borders for the 2 images"):
        score_cubic(seg, torch.zeros(2, 8, 8, dtype=torch.int64), hist, borders=[(8, 8)])
    with pytest.raises(ValueError, match=r"targets\[0\] is \(1, 8, 8\)"):
        score_cubic(seg, [torch.zeros(1, 8, 8, dtype=torch.int64)] * 2, hist)
    with pytest.raises(RuntimeError, match="GPU"):             # and no CPU fallback behind it
        score_cubic(seg, torch.zeros(2, 8, 8, dtype=torch.int64), hist)
