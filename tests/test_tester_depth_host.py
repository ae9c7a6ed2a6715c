"""Host side of the depth-aware multi-scale test mode, ms_test_depth (no GPU): the binning table and the weight table of
segmentor/tester.py::depth_fusion_tables against the reference's float64 statements (segmentor/tester.py:459-470 of the reference)
restated with numpy over all 65 536 disparity values, the fixed facts about them, what check_config accepts and refuses, and the
disparity PNGs (16-bit round trip, refusal of other files, placement at the pad offset, refusal of another size)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json")
S7 = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]


def _cfg(**test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=TINY)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def _reference_bins(S):
    """fuse_with_depth of the reference (:459-465) on a 'stereo map' that holds every uint16 value once."""
    MAX_DEPTH = 63
    stereo_map = np.arange(65536, dtype=np.uint16)
    with np.errstate(divide="ignore"):
        depth_map = stereo_map / 256.0
        depth_map = 0.5 / depth_map
        depth_map = 500 * depth_map
    depth_map = np.clip(depth_map, 0, MAX_DEPTH)
    return depth_map // (MAX_DEPTH // S)


def _reference_weight(bins, scale, scales):
    """:467-473: the weight map of one scale as the fp32 tensor that multiplies the probabilities."""
    scale_index = 0
    for idx, s in enumerate(scales):          # _locate_scale_index, :477-482
        if scale == s:
            scale_index = idx
            break
    weight_map = np.abs(bins - scale_index)
    weight_map = np.power(0.8, weight_map)
    return weight_map.astype(np.float32)


@pytest.mark.parametrize("S", range(1, 9))
def test_tables_equal_the_reference_statements_over_all_disparities(S):
    from contrastiveseg_amd.segmentor.tester import depth_fusion_tables
    scales = [0.5 + 0.25 * i for i in range(S)]
    lut, table = depth_fusion_tables(scales)
    bins = _reference_bins(S)
    assert lut.dtype == np.uint8 and lut.shape == (65536,)
    assert np.isfinite(bins).all() and np.array_equal(lut.astype(np.float64), bins)
    assert (np.diff(bins) <= 0).all()                                      # non-increasing in the disparity
    nbins = [2, 3, 4, 5, 6, 7, 8, 10][S - 1]
    assert bins.min() == 0 and bins.max() == 63 // (63 // S) == nbins - 1
    assert table.dtype == np.float32 and table.shape == (S, nbins)
    for i, scale in enumerate(scales):                                     # the whole weight map of every scale, bit for bit
        assert np.array_equal(table[i][lut], _reference_weight(bins, scale, scales)), (S, i)


def test_fixed_facts():
    from contrastiveseg_amd.segmentor.tester import depth_fusion_tables
    lut7, table7 = depth_fusion_tables(S7)
    s = np.arange(65536)
    t7 = [7111, 3555, 2370, 1777, 1422, 1185, 1015]
    assert np.array_equal(lut7, sum((s <= t).astype(np.uint8) for t in t7))
    assert lut7[0] == 7 and lut7[65535] == 0 and lut7[7111] == 1 and lut7[7112] == 0
    lut8, table8 = depth_fusion_tables(S7 + [2.25])
    t8 = [9142, 4571, 3047, 2285, 1828, 1523, 1306, 1142, 1015]
    assert np.array_equal(lut8, sum((s <= t).astype(np.uint8) for t in t8))
    assert lut8[0] == 9 and table8.shape == (8, 10)
    want = np.array([np.float32(0.8 ** k) for k in range(10)], dtype=np.float32)
    assert np.array_equal(table8[0], want)
    assert want[0] == 1 and want[1] == np.float32(0.8) and want[2] == np.float32(0.64)
    assert "%.8f" % want[9] == "0.13421772"
    for i in range(8):
        assert np.array_equal(table8[i], want[np.abs(np.arange(10) - i)])
    assert np.array_equal(table7, want[np.abs(np.arange(8)[None, :] - np.arange(7)[:, None])])


def test_repeated_scales_take_the_first_index():
    from contrastiveseg_amd.segmentor.tester import depth_fusion_tables
    lut, table = depth_fusion_tables([1.0, 0.5, 1.0])
    assert table.shape == (3, 4)
    assert np.array_equal(table[2], table[0]) and not np.array_equal(table[1], table[0])
    assert np.array_equal(table[1], np.array([0.8, 1.0, 0.8, 0.8 ** 2], dtype=np.float32))
    with pytest.raises(ValueError, match="9 scales"):
        depth_fusion_tables([1.0] * 9)
    with pytest.raises(ValueError, match="0 scales"):
        depth_fusion_tables([])


def test_check_config_accepts_the_mode_with_a_depth_dir():
    from contrastiveseg_amd.segmentor.tester import check_config, resolve_depth_dir
    cfg = _cfg(mode="ms_test_depth", scale_search=S7, depth_dir="/data/stereo/val")
    assert check_config(cfg) == ("ms_test_depth", S7, None)
    assert resolve_depth_dir(cfg, "ms_test_depth") == "/data/stereo/val" and resolve_depth_dir(cfg, "ms_test") is None
    # scale_weights is not read, whatever its length
    assert check_config(_cfg(mode="ms_test_depth", scale_search=[0.5, 1.0], scale_weights=[1, 2, 3], depth_dir="d")) == \
        ("ms_test_depth", [0.5, 1.0], None)
    assert check_config(_cfg(mode="ms_test_depth", depth_dir="d")) == ("ms_test_depth", [1.0], None)
    fix = {"size_mode": "fix_size", "input_size": [96, 64], "align_method": "only_pad"}
    assert check_config(_cfg(mode="ms_test_depth", scale_search=[1.0], depth_dir="d", data_transformer=fix))[0] == "ms_test_depth"


def test_check_config_refusals():
    from contrastiveseg_amd.segmentor.tester import check_config
    with pytest.raises(NotImplementedError, match=r"ms_test_depth.*needs test\.depth_dir.*not set"):
        check_config(_cfg(mode="ms_test_depth", scale_search=S7))
    with pytest.raises(NotImplementedError, match=r"ms_test_depth.*needs test\.depth_dir.*not set"):
        check_config(_cfg(mode="ms_test_depth", scale_search=S7, depth_dir=None))
    with pytest.raises(ValueError, match="depth_dir"):
        check_config(_cfg(mode="ms_test_depth", depth_dir=7))
    with pytest.raises(NotImplementedError, match="crf_ss_test"):
        check_config(_cfg(mode="crf_ss_test", depth_dir="d"))
    with pytest.raises(ValueError, match="scale_search has 9 scales"):
        check_config(_cfg(mode="ms_test_depth", depth_dir="d", scale_search=[1.0] * 9))
    ragged = {"size_mode": "diverse_size", "align_method": "only_pad", "pad_mode": "pad_right_down"}
    with pytest.raises(NotImplementedError, match=r"ms_test_depth.*diverse_size"):
        check_config(_cfg(mode="ms_test_depth", depth_dir="d", data_transformer=ragged))
    with pytest.raises(NotImplementedError, match=r"flip_swap_pair.*ms_test_depth"):
        check_config(_cfg(mode="ms_test_depth", depth_dir="d", flip_swap_pair=[[1, 2]]))
    # the key alone changes nothing for the other modes
    assert check_config(_cfg(mode="ms_test", scale_search=[0.5, 1.0], depth_dir="d")) == ("ms_test", [0.5, 1.0], None)


def test_the_shipped_config_names_the_mode_and_leaves_the_directory_open():
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tester import check_config
    path = os.path.join(ROOT, "configs", "cityscapes", "H_48_D_4_TEST_DEPTH.json")
    cfg = Configer(configs=path)
    assert cfg.get("test", "mode") == "ms_test_depth" and cfg.get("test", "scale_search") == S7
    assert cfg.get("test", "depth_dir") is None
    with pytest.raises(NotImplementedError, match="depth_dir"):
        check_config(cfg)
    cfg.update(["test", "depth_dir"], "/data/cityscapes/stereo/val")
    assert check_config(cfg) == ("ms_test_depth", S7, None)


def _bare_tester(depth_dir):
    """A Tester without a model: enough for the host-side loading of the disparity maps."""
    from contrastiveseg_amd.segmentor.tester import Tester
    t = Tester.__new__(Tester)
    t.depth_dir = str(depth_dir)
    return t


def test_disparity_pngs(tmp_path):
    from PIL import Image
    from contrastiveseg_amd.segmentor.tester import load_disparity
    rs = np.random.RandomState(304)
    disp = rs.randint(0, 65536, size=(5, 7)).astype(np.uint16)
    disp[0, :3] = [0, 65535, 256]
    Image.fromarray(disp).save(str(tmp_path / "a.png"))
    back = load_disparity(str(tmp_path / "a.png"))
    assert back.dtype == np.uint16 and np.array_equal(back, disp)
    Image.fromarray(rs.randint(0, 256, size=(5, 7)).astype(np.uint8)).save(str(tmp_path / "grey8.png"))
    Image.fromarray(rs.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)).save(str(tmp_path / "rgb.png"))
    for name in ("grey8", "rgb"):
        with pytest.raises(ValueError, match=r"%s\.png.*single-channel 16-bit" % name):
            load_disparity(str(tmp_path / (name + ".png")))
    # placement: at (left, up) inside a zero buffer of the padded size
    other = rs.randint(1, 65536, size=(4, 6)).astype(np.uint16)
    Image.fromarray(other).save(str(tmp_path / "b.png"))
    t = _bare_tester(tmp_path)
    buf = t._disparity(["a", "b"], (8, 10), [(5, 7), (4, 6)], [(3, 2), (0, 0)])
    assert buf.dtype == np.uint16 and buf.shape == (2, 8, 10)
    want = np.zeros((2, 8, 10), np.uint16)
    want[0, 2:7, 3:10] = disp
    want[1, :4, :6] = other
    assert np.array_equal(buf, want)
    assert np.array_equal(t._disparity(["a"], (5, 7), None, None)[0], disp)
    with pytest.raises(ValueError, match=r"a\.png.*5 x 7.*4 x 7.*cv2\.resize"):
        t._disparity(["a"], (8, 10), [(4, 7)], [(0, 0)])
    with pytest.raises(ValueError, match=r"grey8\.png"):
        t._disparity(["grey8"], (5, 7), None, None)
    with pytest.raises(FileNotFoundError):
        t._disparity(["missing"], (5, 7), None, None)
