"""Host side of the SegFix refinement (no GPU): the numpy restatement of the rule (tests/segfix_cases.py) against the REFERENCE's goldens
(tests/golden/segfix/, tools/make_segfix_golden.py) and against torch's CPU grid_sample, the float64 yardstick and the near-tie
pixels, the offset files (lib/datasets/segfix_offsets.py), and what segmentor/tester.py::check_config refuses before a model is
built."""
import fractions
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import segfix_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json")
NAMES = SC.golden_names()


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_the_case_table_and_the_fixtures_belong_together():
    assert NAMES == ["a", "b", "c", "d", "e", "f", "g", "h_s0.5", "h_s1", "h_s2"]
    assert sorted(os.listdir(SC.GOLDEN)) == sorted(n + ".npz" for n in NAMES)
    for case in SC.GOLDEN_CASES:
        for name, x, off, scale in SC.make_case(case):
            g = SC.golden(name)
            assert np.array_equal(g["x"], x) and np.array_equal(g["offsets"], off) and g["scale"] == scale
            assert g["x"].shape == SC.GOLDEN_CASES[case][0] and g["x"].max() <= 18
            assert os.path.getsize(os.path.join(SC.GOLDEN, name + ".npz")) < 64 * 1024
    g = SC.golden("g")                                     # clamping on all four sides
    assert (g["offsets"][0, :, 0] == -50).all() and (g["offsets"][-1, :, 0] == 50).all()
    assert (g["offsets"][1:-1, 0, 1] == -50).all() and (g["offsets"][1:-1, -1, 1] == 50).all()
    assert set(np.unique(SC.golden("c")["offsets"])) == {-1.0, 0.0, 1.0} and float((SC.golden("c")["offsets"] == 0).mean()) > 0.5
    assert not np.array_equal(SC.golden("h_s1")["offsets"], np.round(SC.golden("h_s1")["offsets"]))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_references_labels_exactly(name):
    g = SC.golden(name)
    got = SC.restate(g["x"], g["offsets"], g["scale"])
    assert got.dtype == np.uint8 and np.array_equal(got, g["out"]), "%d labels differ" % (got != g["out"]).sum()
    assert np.array_equal(SC.id_lut()[got], g["out_ids"])
    assert (g["out"] != g["x"]).any()
    if np.array_equal(g["offsets"], np.round(g["offsets"])):
        assert np.array_equal(SC.restate(g["x"], g["offsets"].astype(np.int8), g["scale"]), got)


def _grid_sample_value(x, offsets, scale):
    """The reference's statements (scripts/cityscapes/segfix.py:64-77) up to the rounding, on this machine's CPU torch -> fp32 [h,w]."""
    h, w = x.shape
    xt = torch.from_numpy(x.astype(np.int64)).unsqueeze(0)
    off = torch.from_numpy(offsets.astype(np.float32).transpose(2, 0, 1) * scale).unsqueeze(0)
    ch, cw = torch.meshgrid([torch.arange(h, dtype=torch.float), torch.arange(w, dtype=torch.float)], indexing="ij")
    norm = torch.FloatTensor([(w - 1) / 2, (h - 1) / 2])
    grid = torch.stack([off[:, 1] + cw, off[:, 0] + ch], dim=-1) / norm - 1
    return F.grid_sample(xt.unsqueeze(1).float(), grid, padding_mode="border", mode="bilinear", align_corners=False).squeeze().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_restated_value_has_the_bits_of_torchs_cpu_grid_sample(name):
    g = SC.golden(name)
    v = SC.restate_value(g["x"], g["offsets"], g["scale"])
    ref = _grid_sample_value(g["x"], g["offsets"], g["scale"])
    # the labels gate in any case
    assert np.array_equal(np.round(ref).astype(np.uint8), g["out"]), "this torch build's grid_sample gives other labels than the goldens"
    assert v.dtype == ref.dtype == np.float32
    assert np.array_equal(v.view(np.uint32), ref.view(np.uint32)), (
        "%d of %d interpolated values differ in their bits from torch %s's CPU grid_sample (largest difference %.3g). The order of "
        "fp32 operations restated in tests/segfix_cases.py was established against torch 2.10; if a later build orders them "
        "differently, the label equality with the reference's goldens (test_restatement_equals_the_references_labels_exactly) is "
        "what gates, not this bit comparison" % ((v.view(np.uint32) != ref.view(np.uint32)).sum(), v.size, torch.__version__,
                                                  float(np.abs(v.astype(np.float64) - ref).max())))


@pytest.mark.parametrize("name", NAMES)
def test_float64_labels_differ_on_near_tie_pixels_only(name):
    g = SC.golden(name)
    v64 = SC.value_f64(g["x"], g["offsets"], g["scale"])
    near = SC.near_tie(v64)
    share = float(near.mean())
    assert share == g["near_tie_share"] and share <= SC.NEAR_TIE_SHARE, "%.2f %% of the pixels are near a rounding tie" % (100 * share)
    differ = np.round(v64).astype(np.uint8) != g["out"]
    assert not (differ & ~near).any(), "%d labels differ from the float64 evaluation away from any tie" % (differ & ~near).sum()
    # the fp32 value itself stays within a few ulp of 18 of the float64 one
    assert float(np.abs(SC.restate_value(g["x"], g["offsets"], g["scale"]).astype(np.float64) - v64).max()) < 1e-4 < SC.NEAR_TIE
    if name in ("a", "b", "c"):
        assert near.any()                                  # these fixtures do contain near-tie pixels


def test_fma32_is_a_correctly_rounded_fused_multiply_add():
    rs = np.random.RandomState(304)
    a = rs.uniform(0, 19, 4000).astype(np.float32)
    b = rs.uniform(0, 1, 4000).astype(np.float32)
    c = rs.uniform(0, 19, 4000).astype(np.float32)
    # adversarial: (1 + 2^-15) * 2^-24 (1 - 2^-15) = 2^-24 (1 - 2^-30), so a * b + c lies 2^-54 below the point half way between two
    # floats; float64 rounds the sum onto that point, and rounding the float64 sum half to even would then go the wrong way for
    # c = 1 + 2^-23 (odd mantissa). Likewise just above the half-way point for c = 1.
    a[0], b[0], c[0] = np.float32(1 + 2.0 ** -15), np.float32(2.0 ** -24 * (1 - 2.0 ** -15)), np.float32(1 + 2.0 ** -23)
    a[1], b[1], c[1] = np.float32(1 + 2.0 ** -15), np.float32(2.0 ** -24 * (1 + 2.0 ** -15)), np.float32(1.0)
    a[2], b[2], c[2] = np.float32(2.0 ** -40), np.float32(2.0 ** -40), np.float32(1.0)
    a[3], b[3], c[3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(-1.0)
    got = SC.fma32(a, b, c)
    assert got[0] == np.float32(1 + 2.0 ** -23) and np.float32(np.float64(a[0]) * np.float64(b[0]) + np.float64(c[0])) != got[0]

    def exact(x, y, z):
        q = fractions.Fraction(float(x)) * fractions.Fraction(float(y)) + fractions.Fraction(float(z))
        lo = np.float32(float(q))                          # double rounding possible: repair against the neighbours
        best = min((np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))),
                   key=lambda f: (abs(fractions.Fraction(float(f)) - q), int(np.float32(f).view(np.uint32)) & 1))
        return np.float32(best)
    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_regions_with_a_side_of_one_are_refused_by_the_restatement_too():
    with pytest.raises(ValueError, match="divides by"):
        SC.restate(np.zeros((1, 5), np.uint8), np.zeros((1, 5, 2), np.float32), 2.0)


# ---- offset files -------------------------------------------------------------------------------------------------------------------------
def test_npy_files_and_the_int8_or_fp32_choice(tmp_path):
    from contrastiveseg_amd.lib.datasets import segfix_offsets as SO
    rs = np.random.RandomState(304)
    unit = rs.randint(-1, 2, size=(6, 9, 2))
    for dtype in (np.int8, np.int16, np.int64, np.uint8):
        np.save(str(tmp_path / "u.npy"), np.abs(unit).astype(dtype) if dtype == np.uint8 else unit.astype(dtype))
        got = SO.load_offsets(str(tmp_path / "u.npy"), (6, 9))
        assert got.dtype == np.int8 and got.flags.c_contiguous and np.array_equal(got, np.abs(unit) if dtype == np.uint8 else unit)
    np.save(str(tmp_path / "big.npy"), unit.astype(np.int32) * 200)         # integers outside int8
    got = SO.load_offsets(str(tmp_path / "big.npy"), (6, 9))
    assert got.dtype == np.float32 and np.array_equal(got, unit * 200)
    for dtype in (np.float32, np.float64, np.float16):                      # a float array stays float, whatever its values
        np.save(str(tmp_path / "f.npy"), unit.astype(dtype))
        got = SO.load_offsets(str(tmp_path / "f.npy"), (6, 9))
        assert got.dtype == np.float32 and np.array_equal(got, unit)
    # .mat comes first, then .npy
    assert SO.find_offset_file(str(tmp_path), "u") == str(tmp_path / "u.npy") and SO.find_offset_file(str(tmp_path), "v") is None
    (tmp_path / "u.mat").write_bytes(b"")
    assert SO.find_offset_file(str(tmp_path), "u") == str(tmp_path / "u.mat")
    # a batch: every image at its region, zero in the padding; int8 only when every array is
    a, b = unit.astype(np.int8), (unit[:4, :5] * 0.5).astype(np.float32)
    both = SO.batch_offsets([a, a], [(1, 2, 9, 6), (0, 0, 9, 6)], (8, 12))
    assert both.dtype == np.int8 and both.shape == (2, 8, 12, 2) and np.array_equal(both[0, 2:8, 1:10], a) and int(np.abs(both).sum()) == 2 * int(np.abs(a).sum())
    mixed = SO.batch_offsets([a, b], [(1, 2, 9, 6), (3, 1, 5, 4)], (8, 12))
    assert mixed.dtype == np.float32 and np.array_equal(mixed[1, 1:5, 3:8], b) and np.array_equal(mixed[0, 2:8, 1:10], a)
    with pytest.raises(ValueError, match=r"the offsets of image 1 of the batch are \(4, 5, 2\), its region 6 x 9"):
        SO.batch_offsets([a, b], [(1, 2, 9, 6), (0, 0, 9, 6)], (8, 12))


def test_mat_round_trip(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from contrastiveseg_amd.lib.datasets import segfix_offsets as SO
    unit = np.random.RandomState(304).randint(-1, 2, size=(6, 9, 2))
    sio.savemat(str(tmp_path / "i.mat"), {"mat": unit.astype(np.int8)})
    sio.savemat(str(tmp_path / "d.mat"), {"mat": unit.astype(np.float64) * 0.5})
    sio.savemat(str(tmp_path / "other.mat"), {"offsets": unit})
    got = SO.load_offsets(str(tmp_path / "i.mat"), (6, 9))
    assert got.dtype == np.int8 and np.array_equal(got, unit)
    got = SO.load_offsets(str(tmp_path / "d.mat"), (6, 9))
    assert got.dtype == np.float32 and np.array_equal(got, unit * 0.5)
    with pytest.raises(ValueError, match=r"other\.mat: no variable 'mat' .* the file holds \['offsets'\]"):
        SO.load_offsets(str(tmp_path / "other.mat"), (6, 9))


def test_offset_files_refused_by_name(tmp_path, monkeypatch):
    from contrastiveseg_amd.lib.datasets import segfix_offsets as SO
    unit = np.zeros((6, 9, 2), np.float32)
    np.save(str(tmp_path / "t.npy"), unit.transpose(2, 0, 1))
    with pytest.raises(ValueError, match=r"t\.npy: the offsets are an array of shape \(2, 6, 9\), the image is 6 x 9: expected \[6, 9, 2\]"):
        SO.load_offsets(str(tmp_path / "t.npy"), (6, 9))
    np.save(str(tmp_path / "s.npy"), unit)
    with pytest.raises(ValueError, match=r"shape \(6, 9, 2\), the image is 6 x 10"):
        SO.load_offsets(str(tmp_path / "s.npy"), (6, 10))
    for bad, kind in ((unit > 0, "bool"), (unit.astype(np.complex64), "complex64"), (unit.astype("U4"), "<U4")):
        np.save(str(tmp_path / "k.npy"), bad)
        with pytest.raises(ValueError, match=r"k\.npy: the offsets are of type %s, expected an integer or floating-point array" % kind):
            SO.load_offsets(str(tmp_path / "k.npy"), (6, 9))
    for value in (np.nan, np.inf, -np.inf):
        bad = unit.copy()
        bad[2, 3, 1] = bad[0, 0, 0] = value
        np.save(str(tmp_path / "n.npy"), bad)
        with pytest.raises(ValueError, match=r"n\.npy: the offsets hold 2 non-finite values"):
            SO.load_offsets(str(tmp_path / "n.npy"), (6, 9))
    # scipy is looked for only when a .mat file is read, and its absence is named
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "scipy.io", None)
    assert SO.load_offsets(str(tmp_path / "s.npy"), (6, 9)).dtype == np.float32
    (tmp_path / "m.mat").write_bytes(b"")
    with pytest.raises(ImportError, match=r"m\.mat is a MATLAB file and scipy is not installed"):
        SO.load_offsets(str(tmp_path / "m.mat"), (6, 9))


# ---- check_config -------------------------------------------------------------------------------------------------------------------------
def _cfg(label_list=SC.LABEL_LIST, **test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=TINY)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    if label_list is not None:
        cfg.update(["data", "num_classes"], len(label_list))
        cfg.add(["data", "label_list"], list(label_list))
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def _images(tmp_path, stems=("a_000", "b_001")):
    from PIL import Image
    img = tmp_path / "val" / "image"
    img.mkdir(parents=True)
    for stem in stems:
        Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(str(img / (stem + ".png")))
    return str(img)


def test_check_config_resolves_the_keys_and_refuses_by_name(tmp_path):
    from contrastiveseg_amd.segmentor.tester import check_config, resolve_segfix
    off = tmp_path / "offsets"
    off.mkdir()
    images = _images(tmp_path)
    for stem in ("a_000", "b_001"):
        np.save(str(off / (stem + ".npy")), np.zeros((4, 6, 2), np.int8))
    assert resolve_segfix(_cfg(mode="ss_test")) == (None, None)
    assert resolve_segfix(_cfg(segfix_offset_dir=str(off), test_dir=images)) == (str(off), 2.0)         # the default scale
    assert resolve_segfix(_cfg(segfix_offset_dir=str(off), segfix_scale=1, test_dir=images)) == (str(off), 1.0)
    assert check_config(_cfg(mode="ms_test", scale_search=[0.5, 1.0], segfix_offset_dir=str(off), test_dir=images)) == ("ms_test", [0.5, 1.0], None)
    # a stem without a file, named
    os.remove(str(off / "b_001.npy"))
    with pytest.raises(FileNotFoundError, match=r"test\.segfix_offset_dir %s has neither b_001\.mat nor b_001\.npy" % str(off)):
        check_config(_cfg(segfix_offset_dir=str(off), test_dir=images))
    (off / "b_001.mat").write_bytes(b"")                  # either extension will do for the listing
    check_config(_cfg(segfix_offset_dir=str(off), test_dir=images))
    # a missing directory, named
    with pytest.raises(FileNotFoundError, match=r"test\.segfix_offset_dir %s does not exist" % str(tmp_path / "nowhere")):
        check_config(_cfg(segfix_offset_dir=str(tmp_path / "nowhere"), test_dir=images))
    with pytest.raises(ValueError, match=r"test\.segfix_offset_dir 7: expected a directory name"):
        check_config(_cfg(segfix_offset_dir=7))
    for scale in ("2", float("nan"), True):
        with pytest.raises(ValueError, match=r"test\.segfix_scale .*: expected a finite number"):
            check_config(_cfg(segfix_offset_dir=str(off), segfix_scale=scale))
    # size_mode diverse_size: list batches
    dt = {"size_mode": "diverse_size", "align_method": "only_pad", "pad_mode": "pad_right_down", "fit_stride": 8}
    with pytest.raises(NotImplementedError, match=r"test\.segfix_offset_dir under test\.data_transformer size_mode diverse_size"):
        check_config(_cfg(segfix_offset_dir=str(off), data_transformer=dt))
    # the reference script hard-codes the 19 Cityscapes classes
    for label_list in (None, SC.LABEL_LIST[:-1], SC.LABEL_LIST[::-1], list(range(19))):
        with pytest.raises(NotImplementedError, match=r"test\.segfix_offset_dir with data\.label_list .* hard-codes the label list \[7, 8, 11"):
            check_config(_cfg(label_list=label_list, segfix_offset_dir=str(off), test_dir=images))


def test_without_the_key_check_config_is_unchanged(tmp_path):
    from contrastiveseg_amd.segmentor.tester import check_config
    images = _images(tmp_path)
    # configurations the refinement would refuse pass as before, with the same result
    dt = {"size_mode": "diverse_size", "align_method": "only_pad", "pad_mode": "pad_right_down", "fit_stride": 8}
    assert check_config(_cfg(label_list=None, mode="ms_test", scale_search=[0.5, 1.0], scale_weights=[1, 2], test_dir=images,
                             data_transformer=dt)) == ("ms_test", [0.5, 1.0], [1, 2])
    assert check_config(_cfg(label_list=None, mode="ss_test", test_dir=images)) == ("ss_test", [1.0], None)
    assert check_config(_cfg(label_list=None, segfix_offset_dir=None, segfix_scale="unused")) == ("ss_test", [1.0], None)


def test_the_shipped_config_sets_both_keys_with_the_evaluator(tmp_path):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tester import check_config, resolve_evaluator, resolve_segfix
    cfg = Configer(configs=os.path.join(ROOT, "configs", "cityscapes", "H_48_D_4_TEST_SEGFIX.json"))
    assert cfg.get("test", "evaluator") == "cityscapes" and cfg.get("test", "segfix_scale") == 2.0
    assert cfg.get("data", "label_list") == SC.LABEL_LIST
    with pytest.raises(FileNotFoundError, match="offset_hrnext does not exist"):          # the directory is the user's to provide
        check_config(cfg)
    cfg.update(["test", "segfix_offset_dir"], str(tmp_path))
    assert check_config(cfg)[0] == "ms_test" and resolve_segfix(cfg) == (str(tmp_path), 2.0) and resolve_evaluator(cfg)[0] == "cityscapes"


def test_write_json_takes_a_sub_directory(tmp_path):
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    assert CS.RESULT_FILE == os.path.join("evaluationResults", "resultPixelLevelSemanticLabeling.json") == os.path.join(CS.RESULT_DIR, CS.RESULT_NAME)
    score = CS.CityscapesScore(SC.id_lut(), "cpu")
    score.reduced = (np.eye(34, dtype=np.int64), np.zeros((10, 2), np.int64), np.zeros((10, 2), np.float64))
    first = score.write_json(str(tmp_path))
    second = score.write_json(str(tmp_path), "evaluationResults_w_segfix")
    assert first == str(tmp_path / CS.RESULT_FILE) and second == str(tmp_path / "evaluationResults_w_segfix" / CS.RESULT_NAME)
    assert open(first).read() == open(second).read() and "confMatrix" in json.loads(open(first).read().replace("NaN", "null"))
