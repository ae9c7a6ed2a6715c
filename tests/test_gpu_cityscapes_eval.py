"""The pixel-level Cityscapes evaluation of the test phase: kernels.cs_eval_update / kernels.cs_eval_reduce (csrc/cityscapes_eval.hip:
cseg_cs_eval_update, cseg_cs_eval_reduce), lib/metrics/cityscapes_score.py::CityscapesScore and the `test.evaluator: cityscapes` leg of
the Tester.

Yardsticks. (1) tests/golden/cityscapes_eval/: three synthetic 32 x 64 triples and what the REFERENCE's evaluator
(lib/metrics/cityscapes_evaluator.py, Python path) returned for them (tools/make_cityscapes_eval_golden.py): the matrix and the integer
tp / fn must be equal, every weighted sum must have the golden's float64 BITS, the final dictionary must be equal with NaN in the same
places. (2) `_restate` below: evaluatePair's statements (:607-649) in numpy and Python floats -- np.unique order, one mask per
instance -- on seeded cases that the goldens do not reach; everything is compared with ==, there is no tolerance anywhere.
The kernel-level tests are replayed on the CPU emulation by tests/test_emu_cityscapes_eval.py."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cityscapes_eval")
LABEL_LIST = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


def _dev():
    return torch.device("cuda:0")


def _lut(label_list=LABEL_LIST):
    lut = np.zeros(256, np.uint8)
    lut[:len(label_list)] = label_list
    return lut


IDENTITY = np.where(np.arange(256) < 34, np.arange(256), 0).astype(np.uint8)


# ---- the reference's statements ---------------------------------------------------------------------------------------------------------
def _restate(images):
    """images: [(prediction label ids, labelIds, instanceIds)] as 2-D arrays, in evaluation order -> conf [34,34] int64, stats_i [10,2]
    int64 {tp, fn}, stats_f [10,2] float64 {tpWeighted, fnWeighted}; rows as CS.STAT_ROWS."""
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    conf = np.zeros((34, 34), np.int64)
    stats = {name: {"tp": 0.0, "fn": 0.0, "tpWeighted": 0.0, "fnWeighted": 0.0} for name in CS.STAT_ROWS}
    for pred, gt, inst in images:
        np.add.at(conf, (gt.astype(np.int64).ravel(), pred.astype(np.int64).ravel()), 1)
        masks = {cat: np.isin(pred, ids) for cat, ids in CS.INSTANCE_CATEGORIES.items()}
        for inst_id in np.unique(inst[inst > 1000]):
            label = CS.ID2LABEL[int(inst_id / 1000)]
            if label.ignore_in_eval:
                continue
            mask = inst == inst_id
            size = np.count_nonzero(mask)
            weight = CS.AVG_CLASS_SIZE[label.name] / float(size)
            for row, tp in ((label.name, np.count_nonzero(pred[mask] == label.id)),
                            (label.category, np.count_nonzero(np.logical_and(mask, masks[label.category])))):
                stats[row]["tp"] += tp
                stats[row]["fn"] += size - tp
                stats[row]["tpWeighted"] += float(tp) * weight
                stats[row]["fnWeighted"] += float(size - tp) * weight
    stats_i = np.array([[stats[r]["tp"], stats[r]["fn"]] for r in CS.STAT_ROWS]).astype(np.int64)
    stats_f = np.array([[stats[r]["tpWeighted"], stats[r]["fnWeighted"]] for r in CS.STAT_ROWS], dtype=np.float64)
    return conf, stats_i, stats_f


def _same(a, b):
    """== with NaN equal to NaN, through dictionaries (whatever the order of their keys) and lists."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- seeded cases -----------------------------------------------------------------------------------------------------------------------
# name: (B, H, W), records (x0, y0, bw, bh) per image or None for the whole image, a stripe of full rows (y, rows) for one instance
CASES = {
    "odd83": ((3, 37, 83), None, (6, 9)),                  # width no multiple of 64; runs cross row ends and wave boundaries
    "blocks3": ((2, 70, 131), None, (8, 50)),              # 9170 pixels: three blocks per image, one instance in all of them
    "padded": ((2, 40, 96), [(5, 3, 83, 31), (0, 7, 64, 33)], (4, 11)),        # non-zero pad_offset, garbage in the padding
    "row1": ((1, 1, 9), None, None),
}
THINGS = [(24, 0), (33, 999), (26, 3), (25, 17), (27, 1), (28, 2), (29, 4), (30, 5), (31, 6), (32, 7), (25, 999), (26, 998)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> pred (train ids) u8 [B,H,W], labelmap_raw u8, instancemap u16, records, and the restatement's three arrays; computed once, shared,
    never modified."""
    (B, H, W), records, stripe = CASES[name]
    rs = np.random.RandomState(304 + len(name))
    records = records or [(0, 0, W, H)] * B
    inv = np.full(34, 255, np.uint8)
    inv[LABEL_LIST] = np.arange(len(LABEL_LIST))
    pred = rs.randint(0, 256, size=(B, H, W)).astype(np.uint8)     # garbage wherever no region is written
    raw = np.full((B, H, W), 200, np.uint8)
    inst = np.full((B, H, W), 50000, np.uint16)
    images = []
    for b, (x0, y0, bw, bh) in enumerate(records):
        def rect(hmax, wmax):
            h, w = rs.randint(1, min(hmax, bh) + 1), rs.randint(1, min(wmax, bw) + 1)
            y, x = rs.randint(0, bh - h + 1), rs.randint(0, bw - w + 1)
            return slice(y, y + h), slice(x, x + w)
        lab = np.full((bh, bw), 7, np.uint8)
        for _ in range(10):
            lab[rect(12, 30)] = [0, 3, 4, 7, 8, 11, 21, 23, 9, 16][rs.randint(10)]      # void and ignored labels among them
        ids = lab.astype(np.uint16)
        for l, n in THINGS:                                # the same ids in every image of the batch
            at = rect(9, 20)
            lab[at], ids[at] = l, l * 1000 + n
        if stripe is not None and stripe[0] + stripe[1] <= bh:
            lab[stripe[0]:stripe[0] + stripe[1]], ids[stripe[0]:stripe[0] + stripe[1]] = 26, 26500
        at = rect(5, 9)
        lab[at], ids[at] = 26, 26                          # a crowd region: the bare label id
        at = rect(3, 5)
        lab[at], ids[at] = 1, 1000                         # not above 1000: no instance
        if bw >= 8:                                        # nothing overwrites these: instance numbers 0 and 999, one never predicted
            lab[0, 0:2], ids[0, 0:2] = 24, 24000
            lab[0, 2:4], ids[0, 2:4] = 27, 27777
            lab[0, 4:6], ids[0, 4:6] = 29, 29004           # ignored in the evaluation
            lab[0, 6:8], ids[0, 6:8] = 30, 30005
            lab[bh - 1, bw - 2:], ids[bh - 1, bw - 2:] = 33, 33999
        p = np.where(inv[lab] == 255, rs.randint(0, len(LABEL_LIST), size=lab.shape), inv[lab]).astype(np.uint8)
        for _ in range(12):
            p[rect(8, 16)] = rs.randint(0, len(LABEL_LIST))
        p[rect(2, 3)] = 255                                # a train id outside label_list: label id 0
        p[ids == 27777] = inv[26]                          # an instance without a true positive, all of it inside its category
        pred[b, y0:y0 + bh, x0:x0 + bw], raw[b, y0:y0 + bh, x0:x0 + bw], inst[b, y0:y0 + bh, x0:x0 + bw] = p, lab, ids
        images.append((_lut()[p], lab, ids))
    return pred, raw, inst, records, _restate(images)


def _run(dev, pred, raw, inst, records, lut=None, score=None):
    from contrastiveseg_amd.lib.metrics.cityscapes_score import CityscapesScore
    score = score or CityscapesScore(_lut() if lut is None else lut, dev)
    score.update(torch.from_numpy(pred).to(dev), torch.from_numpy(raw).to(dev), torch.from_numpy(inst.view(np.int16)).to(dev), records)
    return score


def _arrays(score):
    return score.conf.cpu().numpy(), score.stats_i.cpu().numpy(), score.stats_f.cpu().numpy()


def _assert_equal(got, want, what):
    (c, si, sf), (wc, wsi, wsf) = got, want
    assert np.array_equal(c, wc), "%s: the matrix differs at %s" % (what, np.argwhere(c != wc)[:4].tolist())
    assert np.array_equal(si, wsi), "%s: tp / fn\n%s\n%s" % (what, si, wsi)
    assert np.array_equal(_bits(sf), _bits(wsf)), "%s: weighted sums\n%r\n%r" % (what, sf, wsf)


# ---- 1. the reference's goldens -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    from PIL import Image
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        g = json.load(f)
    load = lambda stem, what: np.asarray(Image.open(os.path.join(GOLDEN, "%s_%s.png" % (stem, what))))
    triples = [(load(s, "pred").astype(np.uint8), load(s, "gtFine_labelIds").astype(np.uint8), load(s, "gtFine_instanceIds").astype(np.uint16))
               for s in g["stems"]]
    return g, triples


def test_golden_triples_give_the_references_numbers():
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    dev = _dev()
    g, triples = _golden()
    H, W = triples[0][0].shape
    score = _run(dev, np.stack([t[0] for t in triples]), np.stack([t[1] for t in triples]), np.stack([t[2] for t in triples]),
                 [(0, 0, W, H)] * len(triples), lut=IDENTITY)
    conf, si, sf = _arrays(score)
    ref, stats = g["all"]["result"], g["all"]["instStats"]
    assert conf.tolist() == ref["confMatrix"]
    rows = [stats["classes"][n] for n in CS.INSTANCE_CLASSES] + [stats["categories"][c] for c in CS.INSTANCE_CATEGORIES]
    assert si.tolist() == [[r["tp"], r["fn"]] for r in rows]
    want = np.array([[r["tpWeighted"], r["fnWeighted"]] for r in rows], dtype=np.float64)
    assert np.array_equal(_bits(sf), _bits(want)), (sf, want)
    assert float(want.min()) >= 0 and float(want[:, 0].max()) > 0          # the goldens are not empty
    result, acc = score.results()
    assert _same(json.loads(json.dumps(result)), ref)
    assert acc == g["all"]["pixelAccuracy"]
    assert _same(score.inst_stats(), stats)
    # and the restatement of this file agrees with the reference on them
    _assert_equal((conf, si, sf), _restate(triples), "restatement on the goldens")


# ---- 2. the numpy restatement on seeded cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_update_and_reduce_equal_the_restatement(case):
    dev = _dev()
    pred, raw, inst, records, want = _case(case)
    if case == "blocks3":                                  # three blocks walk each image 768 pixels at a time: the stripe is in all
        assert int((inst[0] == 26500).sum()) > 4096
    if case != "row1":
        assert want[1][:, 0].min() >= 0 and want[0][:7].sum() > 0 and want[1][:8].sum() > 0
    _assert_equal(_arrays(_run(dev, pred, raw, inst, records)), want, case)


def test_the_table_keeps_two_images_apart_and_skips_what_the_reference_skips():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    pred, raw, inst, records, _ = _case("odd83")
    conf = torch.zeros(34, 34, dtype=torch.int64, device=dev)
    table = K.cs_eval_update(torch.from_numpy(pred).to(dev), torch.from_numpy(_lut()).to(dev), torch.from_numpy(raw).to(dev),
                             torch.from_numpy(inst.view(np.int16)).to(dev), records, conf).cpu().numpy()
    assert table.shape == (3, 10, 1000, 3) and int(conf.sum()) == pred.size
    p = _lut()[pred]
    for b in range(3):
        ids = np.unique(inst[b][inst[b] > 1000])
        assert {24000, 33999, 26500} <= set(ids.tolist())              # instance numbers 0 and 999 occur, in every image
        want = np.zeros((10, 1000, 3), np.int64)
        for i in ids:
            l, m = int(i) // 1000, inst[b] == i
            cat = [24, 25] if l <= 25 else list(range(26, 34))
            want[l - 24, int(i) % 1000] = [m.sum(), (p[b][m] == l).sum(), np.isin(p[b][m], cat).sum()]
        assert np.array_equal(table[b], want)
        assert want[5].sum() > 0 and want[6].sum() > 0                    # labels 29 / 30 are in the table; the reduction leaves them out
    assert table[0, 3, 777].tolist() == [2, 0, 2]          # 27777: tp = 0, all of it in its category


def test_two_batches_equal_one_call_on_their_concatenation():
    dev = _dev()
    pred, raw, inst, records, want = _case("odd83")
    whole = _run(dev, pred, raw, inst, records)
    parts = _run(dev, pred[:1], raw[:1], inst[:1], records[:1])
    _run(dev, pred[1:], raw[1:], inst[1:], records[1:], score=parts)
    _assert_equal(_arrays(parts), _arrays(whole), "two batches")
    _assert_equal(_arrays(parts), want, "two batches against the restatement")


def test_two_calls_are_bit_identical():
    dev = _dev()
    pred, raw, inst, records, _ = _case("blocks3")
    _assert_equal(_arrays(_run(dev, pred, raw, inst, records)), _arrays(_run(dev, pred, raw, inst, records)), "second call")


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    pred, raw, inst, records, _ = _case("odd83")

    def call(pred=pred, raw=raw, inst=inst, records=records, lut=_lut(), conf=None, to=dev):
        conf = torch.zeros(34, 34, dtype=torch.int64, device=dev) if conf is None else conf
        return K.cs_eval_update(torch.from_numpy(pred).to(to), torch.from_numpy(lut).to(dev), torch.from_numpy(raw).to(dev),
                                torch.from_numpy(inst.view(np.int16)).to(dev), records, conf)

    bad = raw.copy()
    bad[1, 20, 40], bad[2, 0, 0] = 34, 77
    with pytest.raises(RuntimeError, match=r"labelmap_raw holds label id 34 \(image 1 of the batch, row 20, column 40\)"):
        call(raw=bad)
    for value in (7012, 34000, 65535):
        bad = inst.copy()
        bad[0, 36, 82] = value
        with pytest.raises(RuntimeError, match=r"instance id %d \(image 0 of the batch, row 36, column 82\)" % value):
            call(inst=bad)
    bad_lut = _lut()
    bad_lut[3] = 34
    with pytest.raises(RuntimeError, match="to label id 34"):
        call(lut=bad_lut)
    with pytest.raises(RuntimeError, match=r"labelmap_raw is \(3, 37, 82\), pred is \(3, 37, 83\)"):
        call(raw=np.ascontiguousarray(raw[:, :, :82]))
    with pytest.raises(RuntimeError, match=r"instancemap is \(2, 37, 83\)"):
        call(inst=np.ascontiguousarray(inst[:2]))
    with pytest.raises(RuntimeError, match="2 records for 3 images"):
        call(records=records[:2])
    with pytest.raises(RuntimeError, match=r"records\[1\] = \(x0 1, y0 0, bw 83, bh 37\) does not lie inside the 37 x 83 image"):
        call(records=[records[0], (1, 0, 83, 37), records[2]])
    with pytest.raises(RuntimeError, match="instancemap must be torch.uint16"):
        K.cs_eval_update(torch.from_numpy(pred).to(dev), torch.from_numpy(_lut()).to(dev), torch.from_numpy(raw).to(dev),
                         torch.from_numpy(inst.astype(np.int32)).to(dev), records, torch.zeros(34, 34, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match=r"the matrix is \(19, 19\)"):
        call(conf=torch.zeros(19, 19, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match=r"table is \(1, 10, 999, 3\)"):
        K.cs_eval_reduce(torch.zeros(1, 10, 999, 3, dtype=torch.int32, device=dev), torch.zeros(10, 2, dtype=torch.int64, device=dev),
                         torch.zeros(10, 2, dtype=torch.float64, device=dev))
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            call(to=torch.device("cpu"))
        with pytest.raises(RuntimeError, match="GPU"):
            K.cs_eval_reduce(torch.zeros(1, 10, 1000, 3, dtype=torch.int32), torch.zeros(10, 2, dtype=torch.int64, device=dev),
                             torch.zeros(10, 2, dtype=torch.float64, device=dev))


# ---- 4. the Tester --------------------------------------------------------------------------------------------------------------------------
def test_phase_test_writes_the_scores_of_its_own_pngs(tmp_path):
    from PIL import Image
    from contrastiveseg_amd import main_contrastive
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    ids = [7, 11, 24, 26, 33]
    rs = np.random.RandomState(304)
    val = tmp_path / "val"
    for sub in ("image", "label", "instance"):
        (val / sub).mkdir(parents=True)
    stems = ("frankfurt_000000_000294", "munster_000001_000019")
    truth = {}
    for stem in stems:
        Image.fromarray(rs.randint(0, 256, size=(64, 128, 3)).astype(np.uint8)).save(str(val / "image" / (stem + ".png")))
        lab = np.full((64, 128), 7, np.uint8)
        for _ in range(8):
            y0, x0 = rs.randint(0, 64), rs.randint(0, 128)
            lab[y0:y0 + 20, x0:x0 + 40] = [0, 4, 7, 11, 21][rs.randint(5)]
        inst = lab.astype(np.uint16)
        for l, n in [(24, 0), (26, 3), (33, 999), (29, 1), (26, 4), (24, 7)]:
            y0, x0 = rs.randint(0, 50), rs.randint(0, 100)
            lab[y0:y0 + 14, x0:x0 + 28], inst[y0:y0 + 14, x0:x0 + 28] = l, l * 1000 + n
        Image.fromarray(lab).save(str(val / "label" / (stem + ".png")))
        Image.fromarray(inst).save(str(val / "instance" / (stem + ".png")))
        truth[stem] = (lab, inst)
    out_dir, log = tmp_path / "out", str(tmp_path / "test.log")
    miou = main_contrastive.main(
        ["--configs", os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"), "--phase", "test", "--test_dir", str(val / "image"),
         "--out_dir", str(out_dir), "--log_file", log, "--stdout_level", "error", "network.pretrained", "None", "network.resume", "None",
         "data.label_list", str(ids), "test.mode", "ss_test", "test.batch_size", "2", "test.evaluator", "cityscapes",
         "test.data_transformer", "{'size_mode': 'fix_size', 'input_size': [128, 64], 'align_method': 'only_pad'}"])
    assert miou is not None
    images = []
    for stem in stems:
        png = np.asarray(Image.open(str(out_dir / "label" / (stem + ".png"))))
        assert png.shape == (64, 128) and set(np.unique(png)) <= set(ids)
        images.append((png, truth[stem][0], truth[stem][1]))
    conf, si, sf = _restate(images)
    assert si[:8].sum() > 0
    want, acc = CS.finalize(conf, si, sf)
    with open(str(out_dir / CS.RESULT_FILE)) as f:
        got = json.load(f)
    assert got.pop("pixelAccuracy") == acc
    assert _same(got, json.loads(json.dumps(want, sort_keys=True)))
    text = open(log).read()
    assert "classes          IoU      nIoU" in text and "categories       IoU      nIoU" in text and "Test mIoU" in text
    assert "Score Average : {:5.6f}    {:5.6f}".format(want["averageScoreClasses"], want["averageScoreInstClasses"]) in text
