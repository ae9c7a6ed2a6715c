"""SegFix refinement on the device: kernels.segfix_shift (csrc/segfix.hip: cseg_segfix_shift) and the `test.segfix_offset_dir` leg of
the Tester.

Yardsticks. (1) tests/golden/segfix/*.npz: blocky 19-class maps with offsets and what the REFERENCE's scripts/cityscapes/segfix.py
made of them on CPU torch (tools/make_segfix_golden.py); the kernel's labels must be equal, for fp32 and for int8 offsets.
(2) tests/segfix_cases.py::restate, the numpy fp32 restatement of the rule, which tests/test_segfix_host.py pins to the same goldens
and, bit for bit, to torch's grid_sample: it carries the comparison to padded batches, odd alignments and large images. Everything is
compared with ==; there is no tolerance anywhere. The kernel-level tests are replayed on the CPU emulation by
tests/test_emu_segfix.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import segfix_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = SC.id_lut()


def _dev():
    return torch.device("cuda:0")


def _shift(dev, pred, offsets, records, scale, lut=LUT):
    """numpy in, numpy out: (refined, refined_ids or None, changed)."""
    from contrastiveseg_amd import kernels as K
    refined, ids, changed = K.segfix_shift(torch.from_numpy(np.array(pred)).to(dev), torch.from_numpy(np.array(offsets)).to(dev), records, scale,
                                           None if lut is None else torch.from_numpy(np.array(lut)).to(dev))        # (copies: the fixtures are read-only)
    assert refined.dtype == torch.uint8 and tuple(refined.shape) == pred.shape and changed.dtype == torch.int32
    return refined.cpu().numpy(), None if ids is None else ids.cpu().numpy(), changed.cpu().numpy()


def _as_int8(offsets):
    assert np.array_equal(offsets, np.round(offsets)) and np.abs(offsets).max() <= 127
    return offsets.astype(np.int8)


# ---- 1. the reference's goldens -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.golden_names())
def test_goldens_are_exact_for_both_offset_types(name):
    dev = _dev()
    g = SC.golden(name)
    h, w = g["x"].shape
    integral = bool(np.array_equal(g["offsets"], np.round(g["offsets"])))
    assert integral == (not name.startswith("h"))         # only case h has non-integer offsets
    got = {}
    for kind in ["f32", "i8"] if integral else ["f32"]:
        off = g["offsets"] if kind == "f32" else _as_int8(g["offsets"])
        refined, ids, changed = _shift(dev, g["x"][None], off[None], [(0, 0, w, h)], g["scale"])
        assert np.array_equal(refined[0], g["out"]), "%s %s: %d labels differ from the reference's" % (name, kind, (refined[0] != g["out"]).sum())
        assert np.array_equal(ids[0], g["out_ids"]) and np.array_equal(ids, LUT[refined])
        assert changed.tolist() == [int((g["out"] != g["x"]).sum())] and changed[0] > 0
        got[kind] = refined
    if integral:
        assert np.array_equal(got["f32"], got["i8"])


# ---- 2. a padded batch: the rule runs on each image's region ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _padded():
    """Two images on a 40 x 56 canvas, regions (0, 0, 53, 37) = golden c and (3, 2, 31, 19) = golden b; the padding holds class 200,
    which occurs nowhere inside, and offsets that point far away."""
    c, b = SC.golden("c"), SC.golden("b")
    records = [(0, 0, 53, 37), (3, 2, 31, 19)]
    pred = np.full((2, 40, 56), 200, np.uint8)
    off = np.full((2, 40, 56, 2), 7, np.float32)
    want = pred.copy()
    for k, (g, (x0, y0, bw, bh)) in enumerate(zip((c, b), records)):
        pred[k, y0:y0 + bh, x0:x0 + bw], off[k, y0:y0 + bh, x0:x0 + bw] = g["x"], g["offsets"]
        want[k, y0:y0 + bh, x0:x0 + bw] = g["out"]
    for a in (pred, off, want):
        a.setflags(write=False)
    return pred, off, records, want, [int((g["out"] != g["x"]).sum()) for g in (c, b)]


@pytest.mark.parametrize("kind", ["f32", "i8"])
def test_padded_batch_refines_each_region_as_its_own_image(kind):
    dev = _dev()
    pred, off, records, want, n_changed = _padded()
    refined, ids, changed = _shift(dev, pred, off if kind == "f32" else _as_int8(off), records, 2.0)
    inside = want != 200
    assert int(inside.sum()) == 53 * 37 + 31 * 19
    assert np.array_equal(refined[inside], want[inside]), "the regions differ from the goldens of the cropped images"
    assert (refined[~inside] == 200).all(), "the padding was written"
    assert not (refined[inside] == 200).any() and refined[inside].max() <= 18, "the padding leaked into a region"
    assert np.array_equal(ids, LUT[refined]) and changed.tolist() == n_changed


# ---- 3. the restatement where no golden reaches ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seeded(B, H, W, records, real):
    """-> pred, offsets (fp32; integers in {-1, 0, 1} unless real), the restatement's refined maps; computed once, shared, never
    modified. The padding holds class 200 and large offsets."""
    rs = np.random.RandomState(304 + H + W + len(records))
    pred = np.full((B, H, W), 200, np.uint8)
    off = np.full((B, H, W, 2), 9, np.float32)
    for k, (x0, y0, bw, bh) in enumerate(records):
        pred[k, y0:y0 + bh, x0:x0 + bw] = SC.blocky_map(rs, bh, bw)
        o = rs.uniform(-2.5, 2.5, size=(bh, bw, 2)) if real else rs.randint(-1, 2, size=(bh, bw, 2))
        o = o.astype(np.float32)
        o[rs.random_sample((bh, bw)) < 0.5] = 0
        off[k, y0:y0 + bh, x0:x0 + bw] = o
    want = SC.restate_batch(pred, off, records, 2.0)
    for a in (pred, off, want):
        a.setflags(write=False)
    return pred, off, want


# canvas (H, W), region (x0, y0, bw, bh): widths that are no multiple of 4 take the element-by-element path, x0 = 1, 2, 3 put the region's
# edges inside a group of four pixels on the packed path
ODD = [((19, 31), (0, 0, 31, 19)), ((21, 36), (1, 1, 31, 19)), ((21, 36), (2, 0, 31, 19)), ((19, 34), (3, 0, 31, 19)),
       ((20, 35), (1, 1, 31, 19)), ((19, 33), (2, 0, 31, 19)), ((23, 40), (3, 2, 30, 21)), ((8, 8), (1, 1, 2, 2))]


@pytest.mark.parametrize("kind", ["f32", "i8"])
@pytest.mark.parametrize("canvas, region", ODD, ids=["%dx%d-x%d-w%d" % (c[0], c[1], r[0], r[2]) for c, r in ODD])
def test_odd_alignments_equal_the_restatement(canvas, region, kind):
    dev = _dev()
    pred, off, want = _seeded(1, canvas[0], canvas[1], (region,), False)
    refined, ids, changed = _shift(dev, pred, off if kind == "f32" else _as_int8(off), [region], 2.0)
    assert np.array_equal(refined, want), "%d pixels differ" % (refined != want).sum()
    assert np.array_equal(ids, LUT[refined]) and changed.tolist() == [int((want != pred).sum())]


LARGE = [(1, 256, 512, False), (1, 1024, 2048, False), (2, 256, 512, True)]


@pytest.mark.parametrize("B, H, W, real", LARGE, ids=["%dx%dx%d%s" % (b, h, w, "-real" if r else "") for b, h, w, r in LARGE])
def test_large_images_equal_the_restatement(B, H, W, real):
    dev = _dev()
    records = tuple((0, 0, W, H) for _ in range(B))
    pred, off, want = _seeded(B, H, W, records, real)
    refined, ids, changed = _shift(dev, pred, off, list(records), 2.0)
    assert np.array_equal(refined, want), "%d pixels differ" % (refined != want).sum()
    assert changed.tolist() == [int((want[k] != pred[k]).sum()) for k in range(B)] and changed.min() > 0
    if not real:
        assert np.array_equal(_shift(dev, pred, _as_int8(off), list(records), 2.0)[0], want)


def test_refined_ids_are_optional_and_two_calls_agree():
    dev = _dev()
    pred, off, records, want, n_changed = _padded()
    refined, ids, changed = _shift(dev, pred, off, records, 2.0, lut=None)
    assert ids is None and changed.tolist() == n_changed
    again = _shift(dev, pred, off, records, 2.0)
    assert np.array_equal(refined, again[0]) and np.array_equal(again[1], LUT[refined])
    # scale 0 moves nothing, but the blend is still one: the reference's coordinate mismatch alone changes labels
    g = SC.golden("b")
    zero = _shift(dev, g["x"][None], g["offsets"][None], [(0, 0, 31, 19)], 0.0)[0]
    assert np.array_equal(zero[0], SC.restate(g["x"], g["offsets"], 0.0)) and (zero[0] != g["x"]).any()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    pred, off, records, _, _ = _padded()
    tp, to, tl = (torch.from_numpy(np.array(a)).to(dev) for a in (pred, off, LUT))         # (copies: the fixtures are read-only)
    for bad in ((0, 0, 1, 37), (5, 5, 20, 1)):
        with pytest.raises(RuntimeError, match=r"records\[1\] = \(x0 %d, y0 %d, bw %d, bh %d\): a region needs at least 2 rows and 2 columns" % bad):
            K.segfix_shift(tp, to, [records[0], bad], 2.0, tl)
    with pytest.raises(RuntimeError, match=r"records\[0\] = \(x0 4, y0 0, bw 53, bh 37\) does not lie inside the 40 x 56 image"):
        K.segfix_shift(tp, to, [(4, 0, 53, 37), records[1]], 2.0, tl)
    with pytest.raises(RuntimeError, match=r"offsets is \(2, 40, 55, 2\), expected \(2, 40, 56, 2\)"):
        K.segfix_shift(tp, to[:, :, :55].contiguous(), records, 2.0, tl)
    with pytest.raises(RuntimeError, match=r"offsets is \(2, 2, 40, 56\)"):
        K.segfix_shift(tp, to.permute(0, 3, 1, 2).contiguous(), records, 2.0, tl)
    with pytest.raises(RuntimeError, match=r"pred is \(40, 56\), expected \[B, H, W\]"):
        K.segfix_shift(tp[0], to, records, 2.0, tl)
    with pytest.raises(RuntimeError, match="1 records for 2 images"):
        K.segfix_shift(tp, to, records[:1], 2.0, tl)
    with pytest.raises(RuntimeError, match="offsets must be torch.float32 or torch.int8, got torch.float64"):
        K.segfix_shift(tp, to.double(), records, 2.0, tl)
    with pytest.raises(RuntimeError, match="lut has 19 entries, expected 256"):
        K.segfix_shift(tp, to, records, 2.0, tl[:19].contiguous())
    with pytest.raises(RuntimeError, match="pred must be torch.uint8"):
        K.segfix_shift(tp.to(torch.int32), to, records, 2.0, tl)
    with pytest.raises(RuntimeError, match="scale = .* is not finite"):
        K.segfix_shift(tp, to, records, float("inf"), tl)
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            K.segfix_shift(tp.cpu(), to, records, 2.0, tl)
        with pytest.raises(RuntimeError, match="GPU"):
            K.segfix_shift(tp, to.cpu(), records, 2.0, tl)


# ---- 5. the Tester --------------------------------------------------------------------------------------------------------------------------
class _StubNet(torch.nn.Module):
    """A network whose coarse output does not depend on the weights of anything: logits [B,19,8,16] that favour one class per 1 x 2
    block of a seeded map, so that the upsampled prediction has many class boundaries."""

    def __init__(self, batch):
        super(_StubNet, self).__init__()
        rs = np.random.RandomState(304)
        coarse = np.repeat(rs.randint(0, 19, size=(batch, 8, 8)), 2, axis=2)
        logits = rs.uniform(-1, 1, size=(batch, 19, 8, 16)).astype(np.float32)
        np.put_along_axis(logits, coarse[:, None], 6.0, axis=1)
        self.register_buffer("logits", torch.from_numpy(logits))

    def forward(self, x, is_eval=False):
        assert x.shape[0] == self.logits.shape[0]
        return {"seg": self.logits.to(x.device)}


def _dataset(tmp_path):
    """Two 32 x 64 images with label / instance PNGs and .npy offsets (one int8-sized integer array, one float array)."""
    from PIL import Image
    rs = np.random.RandomState(304)
    val, off_dir = tmp_path / "val", tmp_path / "offsets"
    for sub in ("image", "label", "instance"):
        (val / sub).mkdir(parents=True)
    off_dir.mkdir()
    stems = ("frankfurt_000000_000294", "munster_000001_000019")
    truth, offsets = {}, {}
    for k, stem in enumerate(stems):
        Image.fromarray(rs.randint(0, 256, size=(32, 64, 3)).astype(np.uint8)).save(str(val / "image" / (stem + ".png")))
        lab = LUT[SC.blocky_map(rs, 32, 64)]
        lab[rs.random_sample((32, 64)) < 0.05] = 0          # some unlabelled pixels: ignored by the mIoU
        inst = lab.astype(np.uint16)
        for l, n in [(24, 0), (26, 3), (33, 999)]:
            y0, x0 = rs.randint(0, 24), rs.randint(0, 48)
            lab[y0:y0 + 8, x0:x0 + 16], inst[y0:y0 + 8, x0:x0 + 16] = l, l * 1000 + n
        Image.fromarray(lab).save(str(val / "label" / (stem + ".png")))
        Image.fromarray(inst).save(str(val / "instance" / (stem + ".png")))
        off = rs.randint(-1, 2, size=(32, 64, 2)).astype(np.int64) if k == 0 else rs.uniform(-1.5, 1.5, size=(32, 64, 2)).astype(np.float32)
        np.save(str(off_dir / (stem + ".npy")), off)
        truth[stem], offsets[stem] = lab, off
    return val, off_dir, stems, truth, offsets


def _run_tester(tmp_path, val, out_name, evaluator=True, **segfix):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.lib.utils.tools.logger import Logger as Log
    from contrastiveseg_amd.segmentor.tester import Tester
    cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.update(["data", "num_classes"], 19)
    cfg.add(["data", "label_list"], list(SC.LABEL_LIST))
    keys = dict(mode="ss_test", batch_size=2, test_dir=str(val / "image"), out_dir=str(tmp_path / out_name),
                data_transformer={"size_mode": "fix_size", "input_size": [64, 32], "align_method": "only_pad"}, **segfix)
    if evaluator:
        keys["evaluator"] = "cityscapes"
    for k, v in keys.items():
        cfg.add(["test", k], v)
    log = str(tmp_path / (out_name + ".log"))
    Log.init(logfile_level="info", stdout_level="error", log_file=log, rewrite=True)
    tester = Tester(cfg, seg_net=_StubNet(2).to(_dev()))
    miou = tester.test()
    for handler in list(Log.logger.handlers) if getattr(Log, "logger", None) is not None else []:
        handler.flush()
    return tester, miou, open(log).read()


def test_phase_test_with_segfix_writes_both_directories_and_both_scores(tmp_path):
    from PIL import Image
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    from contrastiveseg_amd.lib.metrics.running_score import RunningScore
    from contrastiveseg_amd.segmentor.tester import SEGFIX_LABEL_DIR, SEGFIX_RESULT_DIR
    val, off_dir, stems, truth, offsets = _dataset(tmp_path)
    plain, miou_plain, log_plain = _run_tester(tmp_path, val, "plain")
    fixed, miou_fixed, log_fixed = _run_tester(tmp_path, val, "fixed", segfix_offset_dir=str(off_dir), segfix_scale=2.0)
    inv = np.full(256, 255, np.uint8)
    inv[SC.LABEL_LIST] = np.arange(19)
    score = RunningScore(num_classes=19, ignore_index=-1)
    n_changed = 0
    for stem in stems:
        # label/ is byte-identical to the run without the key
        a, b = (open(str(tmp_path / d / "label" / (stem + ".png")), "rb").read() for d in ("plain", "fixed"))
        assert a == b
        pred = inv[np.asarray(Image.open(str(tmp_path / "fixed" / "label" / (stem + ".png"))))]
        assert pred.shape == (32, 64) and pred.max() <= 18
        want = SC.restate(pred, offsets[stem], 2.0)
        got = np.asarray(Image.open(str(tmp_path / "fixed" / SEGFIX_LABEL_DIR / (stem + ".png"))))
        assert got.dtype == np.uint8 and np.array_equal(got, LUT[want]), "%s: %d pixels differ" % (stem, (got != LUT[want]).sum())
        changed = int((want != pred).sum())
        assert changed > 0 and "SegFix {}: {} of 2048 pixels changed".format(stem, changed) in log_fixed
        n_changed += changed
        target = inv[truth[stem]].astype(np.int64)
        target[target == 255] = -1
        score.update(torch.from_numpy(want.astype(np.int64)), torch.from_numpy(target))
    assert sorted(os.listdir(str(tmp_path / "fixed" / SEGFIX_LABEL_DIR))) == [s + ".png" for s in stems]
    assert not os.path.exists(str(tmp_path / "plain" / SEGFIX_LABEL_DIR))
    # the mIoU line and the return value are those of the run without the key; the (SegFix) line is the restated maps'
    assert miou_plain == miou_fixed == fixed.last_miou
    line = [l.split("Test mIoU ")[1] for l in log_plain.splitlines() if "Test mIoU " in l]
    assert len(line) == 1 and "Test mIoU " + line[0] in log_fixed
    want_miou = float(score.get_mean_iou())
    assert fixed.last_miou_segfix == want_miou and want_miou != miou_fixed
    assert "Test mIoU (SegFix) {:.6f}".format(want_miou) in log_fixed and "(SegFix)" not in log_plain
    # both score tables, both JSON files; the refinement changed scored pixels, so they differ
    first, second = (json.load(open(str(tmp_path / "fixed" / d / CS.RESULT_NAME))) for d in (CS.RESULT_DIR, SEGFIX_RESULT_DIR))
    assert first == json.load(open(str(tmp_path / "plain" / CS.RESULT_FILE)))
    assert first["confMatrix"] != second["confMatrix"] and np.sum(first["confMatrix"]) == np.sum(second["confMatrix"]) == 2 * 2048
    assert int(np.abs(np.array(first["confMatrix"]) - np.array(second["confMatrix"])).sum()) > 0 and n_changed > 0
    assert not os.path.exists(str(tmp_path / "plain" / SEGFIX_RESULT_DIR))
    assert log_fixed.count("classes          IoU      nIoU") == 2 and log_plain.count("classes          IoU      nIoU") == 1
    assert "Cityscapes scores of the SegFix refinement" in log_fixed


def test_segfix_without_an_evaluator_writes_no_score_files(tmp_path):
    from contrastiveseg_amd.segmentor.tester import SEGFIX_LABEL_DIR, SEGFIX_RESULT_DIR
    val, off_dir, stems, _, _ = _dataset(tmp_path)
    tester, miou, log = _run_tester(tmp_path, val, "fixed", evaluator=False, segfix_offset_dir=str(off_dir))
    assert tester.segfix_scale == 2.0 and tester.last_miou_segfix is not None and "Test mIoU (SegFix)" in log
    assert sorted(os.listdir(str(tmp_path / "fixed" / SEGFIX_LABEL_DIR))) == [s + ".png" for s in stems]
    assert not os.path.exists(str(tmp_path / "fixed" / SEGFIX_RESULT_DIR)) and tester.last_cityscapes_segfix is None
