"""Host side of the sliding-crop test modes (no GPU): the tile starts against the reference's _decide_intersection, and what
segmentor/tester.py refuses before any model is built or any forward pass runs."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json")


def _cfg(**test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=TINY)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def _decide_intersection(total_length, crop_length):
    """segmentor/tester.py:525-533 of the reference, literally."""
    stride = crop_length
    times = (total_length - crop_length) // stride + 1
    cropped_starting = []
    for i in range(times):
        cropped_starting.append(stride * i)
    if total_length - cropped_starting[-1] > crop_length:
        cropped_starting.append(total_length - crop_length)
    return cropped_starting


def test_tile_starts_equal_the_reference():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.segmentor.tester import tile_starts
    for total in range(1, 201):
        for crop in range(1, total + 1):
            want = _decide_intersection(total, crop)
            assert tile_starts(total, crop) == want, (total, crop)
            assert K.crop_tiles(total, crop) == len(want)
            # what the kernel relies on: every index is covered by one or two tiles, the second one being the last
            if total <= 48:
                for p in range(total):
                    over = [i for i, s in enumerate(want) if s <= p < s + crop]
                    assert over == sorted({min(p // crop, len(want) - 1)} | ({len(want) - 1} if p >= total - crop else set())), (total, crop, p)
    assert tile_starts(37, 16) == [0, 16, 21] and tile_starts(53, 24) == [0, 24, 29] and tile_starts(17, 16) == [0, 1]
    with pytest.raises(ValueError, match="cannot be tiled"):
        tile_starts(15, 16)


@pytest.mark.parametrize("mode", ["sscrop_test", "mscrop_test"])
def test_a_missing_crop_size_is_refused_before_a_model_is_built(mode, monkeypatch):
    from contrastiveseg_amd.lib.models import model_manager
    from contrastiveseg_amd.segmentor.tester import Tester, check_config, resolve_crop_size

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(model_manager.ModelManager, "__init__", no_model)
    with pytest.raises(NotImplementedError, match=mode + ".*test.crop_size"):
        Tester(_cfg(mode=mode))
    with pytest.raises(NotImplementedError, match="test.crop_size"):
        resolve_crop_size(_cfg(mode=mode), mode)
    with pytest.raises(ValueError, match="crop_size"):
        Tester(_cfg(mode=mode, crop_size=[40]))
    with pytest.raises(ValueError, match="crop_size"):
        Tester(_cfg(mode=mode, crop_size=[40, 0]))
    assert resolve_crop_size(_cfg(mode=mode, crop_size=[40, 56]), mode) == (40, 56)
    assert check_config(_cfg(mode=mode, crop_size=[40, 56]))[0] == mode


def test_a_canvas_smaller_than_the_crop_is_a_value_error():
    from contrastiveseg_amd.segmentor.tester import check_canvas, resolve_crop_size
    assert check_canvas((64, 96), (40, 56), 1.5) == (96, 144)
    assert check_canvas((64, 96), (64, 96), 1) == (64, 96)
    with pytest.raises(ValueError, match=r"scale 1.25: the canvas 80 x 120 .* smaller than the crop 81 x 56"):
        check_canvas((64, 96), (81, 56), 1.25)
    with pytest.raises(ValueError, match=r"scale 1.0: the canvas 64 x 96 .* smaller than the crop 40 x 97"):
        check_canvas((64, 96), (40, 97), 1.0)
    # a crop that fits at 1.5 only: resolving the key says nothing yet, the scale that does not hold it does
    cfg = _cfg(mode="mscrop_test", crop_size=[70, 100], scale_search=[0.5, 1.0, 1.5])
    crop = resolve_crop_size(cfg, "mscrop_test")
    assert crop == (70, 100) and check_canvas((64, 96), crop, 1.5) == (96, 144)
    with pytest.raises(ValueError, match=r"scale 1.0: the canvas 64 x 96"):
        check_canvas((64, 96), crop, 1.0)


def test_check_config_still_returns_three_values():
    from contrastiveseg_amd.segmentor.tester import check_config, resolve_crop_size
    assert check_config(_cfg(mode="ms_test", scale_search=[0.5, 1.0], scale_weights=[1, 2])) == ("ms_test", [0.5, 1.0], [1, 2])
    assert check_config(_cfg(mode="ss_test", scale_search=[0.5, 1.0])) == ("ss_test", [1.0], None)
    assert check_config(_cfg()) == ("ss_test", [1.0], None)
    assert resolve_crop_size(_cfg(mode="ms_test"), "ms_test") is None
    # the crop modes: scale_search as in ms_test, sscrop_test at scale 1, test.scale_weights never read (reference :511-522)
    assert check_config(_cfg(mode="sscrop_test", crop_size=[40, 56], scale_search=[0.5, 1.0])) == ("sscrop_test", [1.0], None)
    assert check_config(_cfg(mode="mscrop_test", crop_size=[40, 56], scale_search=[0.5, 1.0, 2.0], scale_weights=[1, 2])) == \
        ("mscrop_test", [0.5, 1.0, 2.0], None)
    with pytest.raises(ValueError, match="scale_search"):
        check_config(_cfg(mode="mscrop_test", crop_size=[40, 56], scale_search=[1.0] * 9))
    for mode in ("ms_test_depth", "crf_ss_test"):
        with pytest.raises(NotImplementedError, match=mode):
            check_config(_cfg(mode=mode))
