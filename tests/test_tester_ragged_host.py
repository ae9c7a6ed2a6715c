"""Host side of the test phase on mixed-size datasets (no GPU): what segmentor/tester.py:check_config accepts and refuses under
`test.data_transformer.size_mode: diverse_size`, configs/coco_stuff/H_48_D_4_TEST.json, and the test loader's list batches -- files ->
TestFolderLoader -> the ragged augmentation kernels (their HIP source on the CPU emulation): every image at its own size padded right
/ down to fit_stride with image 0 / label -1, pad_offset (0, 0), a last short batch kept."""
import os

import numpy as np
import pytest
import torch

from test_gpu_aug_ragged import COCO_TRANS, IDS, make_mixed_folder_dataset
from tests.emu import build_emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json")
COCO_TEST = os.path.join(ROOT, "configs", "coco_stuff", "H_48_D_4_TEST.json")
COCO_DT = {"size_mode": "diverse_size", "fit_stride": 8, "align_method": "only_pad", "pad_mode": "pad_right_down"}


def _cfg(**test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=TINY)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def test_check_config_accepts_the_coco_transformer():
    from contrastiveseg_amd.segmentor.tester import check_config, is_ragged
    scales = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
    cfg = _cfg(mode="ms_test", scale_search=scales, data_transformer=dict(COCO_DT))
    assert check_config(cfg) == ("ms_test", scales, None) and is_ragged(cfg)
    no_stride = {k: v for k, v in COCO_DT.items() if k != "fit_stride"}
    cfg = _cfg(mode="ss_test", data_transformer=no_stride)
    assert check_config(cfg) == ("ss_test", [1.0], None) and is_ragged(cfg)
    assert not is_ragged(_cfg(mode="ss_test"))
    assert not is_ragged(_cfg(mode="ss_test", data_transformer={"size_mode": "fix_size", "input_size": [64, 64], "align_method": "only_pad"}))


@pytest.mark.parametrize("pad_mode", [None, "pad_left_up", "pad_center", "random"])
def test_check_config_refuses_every_pad_mode_but_an_explicit_pad_right_down(pad_mode):
    from contrastiveseg_amd.segmentor.tester import check_config
    dt = {k: v for k, v in COCO_DT.items() if k != "pad_mode"}
    if pad_mode is not None:
        dt["pad_mode"] = pad_mode
    with pytest.raises(NotImplementedError, match="data_transformer") as e:
        check_config(_cfg(mode="ms_test", scale_search=[1.0], data_transformer=dt))
    assert "pad_right_down" in str(e.value) and "top-left" in str(e.value)


@pytest.mark.parametrize("mode", ["sscrop_test", "mscrop_test"])
def test_check_config_refuses_the_sliding_crop_modes_under_diverse_size(mode):
    from contrastiveseg_amd.segmentor.tester import check_config
    with pytest.raises(NotImplementedError, match="data_transformer") as e:
        check_config(_cfg(mode=mode, scale_search=[1.0], crop_size=[64, 64], data_transformer=dict(COCO_DT)))
    assert mode in str(e.value) and "diverse_size" in str(e.value)
    # the same modes under fix_size stay accepted
    assert check_config(_cfg(mode=mode, scale_search=[1.0], crop_size=[64, 64]))[0] == mode


@pytest.mark.parametrize("dt", [dict(COCO_DT, align_method="scale_and_pad"), dict(COCO_DT, align_method="only_scale"),
                                dict(COCO_DT, size_mode="max_size"), dict(COCO_DT, size_mode="multi_size")])
def test_check_config_still_refuses_the_scaling_transformers(dt):
    from contrastiveseg_amd.segmentor.tester import check_config
    with pytest.raises(NotImplementedError, match="data_transformer"):
        check_config(_cfg(mode="ss_test", data_transformer=dt))


def test_the_coco_stuff_test_config_parses():
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tester import check_config, is_ragged
    cfg = Configer(configs=COCO_TEST)
    mode, scales, weights = check_config(cfg)
    assert mode == "ms_test" and scales == [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0] and weights is None
    assert is_ragged(cfg) and cfg.get("test", "batch_size") == 8
    assert cfg.get("test", "data_transformer") == COCO_DT
    assert cfg.get("data", "num_classes") == 171 and len(cfg.get("data", "label_list")) == 172


def _loader_cfg(tmp_path, dt):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    return Configer(config_dict={
        "data": {"num_classes": 19, "input_mode": "BGR", "image_tool": "cv2", "data_dir": str(tmp_path), "label_list": IDS[:5]},
        "train": {"batch_size": 2, "data_transformer": {"size_mode": "fix_size", "input_size": [96, 64], "align_method": "only_pad"}},
        "val": {"batch_size": 2, "data_transformer": {"size_mode": "fix_size", "input_size": [160, 96], "align_method": "only_pad"}},
        "test": {"batch_size": 2, "data_transformer": dt},
        "train_trans": COCO_TRANS, "val_trans": {"trans_seq": ["resize"], "resize": {"min_side_length": 64}},
        "normalize": {"div_value": 255.0, "mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]}})


@pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
@pytest.mark.parametrize("with_labels", [True, False])
def test_test_loader_yields_list_batches_under_diverse_size(tmp_path, monkeypatch, with_labels):
    from PIL import Image
    from tests.emu import inject
    inject.install(monkeypatch)
    from contrastiveseg_amd.lib.datasets.data_loader import DataLoader
    make_mixed_folder_dataset(tmp_path, IDS[:5], np.random.RandomState(0))       # val: 96 x 160, 120 x 90, 81 x 123 (H x W)
    if not with_labels:
        os.remove(str(tmp_path / "val" / "label" / "f01.png"))
    loader = DataLoader(_loader_cfg(tmp_path, dict(COCO_DT, fit_stride=32)), torch.device("cpu")).get_testloader()
    batches = list(loader)
    assert len(loader) == 2 and [len(b["img"]) for b in batches] == [2, 1]        # the last short batch is kept
    assert [b["name"] for b in batches] == [["f00", "f01"], ["f02"]]
    sizes = [(96, 160), (120, 90), (81, 123)]
    padded = [(96, 160), (128, 96), (96, 128)]                                   # no resize in the test loader: the files' own sizes
    flat = [(b, k) for b in batches for k in range(len(b["img"]))]
    for (b, k), (h, w), (Hp, Wp), stem in zip(flat, sizes, padded, ("f00", "f01", "f02")):
        img = b["img"][k]
        assert isinstance(b["img"], list) and img.shape == (1, 3, Hp, Wp) and img.dtype == torch.float32
        assert b["border_size"][k] == (w, h) and b["pad_offset"][k] == (0, 0)
        assert float(img[:, :, h:, :].abs().sum()) == 0.0 and float(img[:, :, :, w:].abs().sum()) == 0.0
        raw = np.asarray(Image.open(str(tmp_path / "val" / "image" / (stem + ".png"))).convert("RGB"))[:, :, ::-1].astype(np.float64)
        want = (raw / 255.0 - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])
        assert np.abs(img[0, :, :h, :w].permute(1, 2, 0).numpy() - want).max() < 1e-5
        if with_labels:
            lab = b["labelmap"][k]
            assert isinstance(b["labelmap"], list) and lab.shape == (1, Hp, Wp) and lab.dtype == torch.int64
            assert bool((lab[:, h:, :] == -1).all()) and bool((lab[:, :, w:] == -1).all())
            raw_lab = np.asarray(Image.open(str(tmp_path / "val" / "label" / (stem + ".png"))))
            lut = np.full(256, -1, np.int64)
            lut[IDS[:5]] = np.arange(5)
            assert np.array_equal(lab[0, :h, :w].numpy(), lut[raw_lab])
        else:
            assert "labelmap" not in b


@pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
def test_test_loader_without_fit_stride_keeps_the_files_sizes(tmp_path, monkeypatch):
    from tests.emu import inject
    inject.install(monkeypatch)
    from contrastiveseg_amd.lib.datasets.data_loader import DataLoader
    make_mixed_folder_dataset(tmp_path, IDS[:5], np.random.RandomState(0))
    dt = {k: v for k, v in COCO_DT.items() if k != "fit_stride"}
    batches = list(DataLoader(_loader_cfg(tmp_path, dt), torch.device("cpu")).get_testloader())
    assert [tuple(x.shape) for b in batches for x in b["img"]] == [(1, 3, 96, 160), (1, 3, 120, 90), (1, 3, 81, 123)]
    assert [s for b in batches for s in b["border_size"]] == [(160, 96), (90, 120), (123, 81)]
