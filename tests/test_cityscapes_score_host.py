"""Host side of the pixel-level Cityscapes evaluation (no GPU): the label table of lib/metrics/cityscapes_score.py and the order of the
result's dictionaries against what the reference's evaluator returned (tests/golden/cityscapes_eval/golden.json, written by
tools/make_cityscapes_eval_golden.py), the finalisation fed the golden's matrix and instStats -- every score with ==, NaN in the same
places --, what check_config and the test loader refuse under `test.evaluator`, the loader's two extra maps, and a two-rank gloo run
that splits the golden's per-image partials between the ranks: the matrix and the integer sums exactly, the weighted sums within
n_instances * 2^-52 relative (the reordering bound of a sum of non-negative terms; bit equality is claimed for one rank only)."""
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cityscapes_eval")
IDS = [7, 11, 24, 26, 33]


def _golden():
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        return json.load(f)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def _stat_arrays(stats):
    """The reference's instStats -> stats_i, stats_f with the rows of CS.STAT_ROWS."""
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    rows = [stats["classes"][n] for n in CS.INSTANCE_CLASSES] + [stats["categories"][c] for c in CS.INSTANCE_CATEGORIES]
    return (np.array([[r["tp"], r["fn"]] for r in rows]).astype(np.int64),
            np.array([[r["tpWeighted"], r["fnWeighted"]] for r in rows], dtype=np.float64))


# ---- 1. table and finalisation against the reference ----------------------------------------------------------------------------------
def test_label_table_and_key_order_equal_the_goldens():
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    g = _golden()["all"]
    ref = g["result"]
    assert [(CS.ID2LABEL[l].name, l) for l in CS.EVAL_LABELS] == [(n, ref["labels"][n]) for n in g["order"]["labels"]]
    assert CS.ID2LABEL[-1].name == "license plate" and CS.ID2LABEL[-1].category == "vehicle" and len(CS.LABELS) == 35
    assert CS.NUM_LABELS == 34 == len(ref["confMatrix"])
    result, _ = CS.finalize(ref["confMatrix"], *_stat_arrays(g["instStats"]))
    for key in ("labels", "priors", "classScores", "classInstScores", "categoryScores", "categoryInstScores"):
        assert list(result[key]) == g["order"][key], key
    assert list(g["instStats"]["classes"]) == CS.INSTANCE_CLASSES
    assert list(g["instStats"]["categories"]) == list(CS.INSTANCE_CATEGORIES)
    for cat, ids in CS.INSTANCE_CATEGORIES.items():
        assert g["instStats"]["categories"][cat]["labelIds"] == ids
    # labels the reference scores: NaN exactly for the ignored ones, instance scores only where instStats has a row
    for lab in CS.LABELS:
        if lab.id >= 0:
            assert math.isnan(ref["classScores"][lab.name]) == lab.ignore_in_eval or ref["priors"][lab.name] == 0
            assert (lab.name in CS.INSTANCE_CLASSES) == (lab.has_instances and not lab.ignore_in_eval)
    assert sorted(CS.AVG_CLASS_SIZE) == sorted(lab.name for lab in CS.LABELS if lab.has_instances)


@pytest.mark.parametrize("which", ["all", 0, 1, 2])
def test_finalize_reproduces_every_score_of_the_reference(which):
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    g = _golden()
    g = g["all"] if which == "all" else g["per_image"][which]
    result, acc = CS.finalize(g["result"]["confMatrix"], *_stat_arrays(g["instStats"]))
    result = json.loads(json.dumps(result))
    assert set(result) == set(g["result"])
    for key in g["result"]:
        assert _same(result[key], g["result"][key]), key
    assert acc == g["pixelAccuracy"]
    n_nan = sum(math.isnan(v) for v in result["classInstScores"].values())
    assert 26 <= n_nan < 34 and not math.isnan(result["averageScoreInstCategories"])
    lines = CS.format_tables(result, acc)
    assert lines[3] == "classes          IoU      nIoU" and "categories       IoU      nIoU" in lines
    assert "Score Average : {:5.6f}    {:5.6f}".format(result["averageScoreClasses"], result["averageScoreInstClasses"]) in lines
    assert sum(line.startswith(("road ", "bicycle ", "human ", "void ")) for line in lines) == 3          # void is all ignored: no line


def test_an_empty_matrix_gives_nan_everywhere():
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    result, acc = CS.finalize(np.zeros((34, 34), np.int64), np.zeros((10, 2), np.int64), np.zeros((10, 2)))
    assert math.isnan(acc) and math.isnan(result["averageScoreClasses"]) and all(math.isnan(v) for v in result["classScores"].values())
    with pytest.raises(ValueError, match="19, 19"):
        CS.finalize(np.zeros((19, 19), np.int64), np.zeros((10, 2), np.int64), np.zeros((10, 2)))


# ---- 2. refusals before a model is built -------------------------------------------------------------------------------------------------
def _cfg(label_list=IDS, **test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=TINY)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    if label_list is not None:
        cfg.add(["data", "label_list"], label_list)
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def _dataset(tmp_path, stems=("a_000000_000001", "b_000000_000002"), size=(24, 40), sub=("image", "label", "instance")):
    from PIL import Image
    rs = np.random.RandomState(304)
    val = tmp_path / "val"
    made = {}
    for s in sub:
        (val / s).mkdir(parents=True, exist_ok=True)
    for stem in stems:
        lab = np.array(IDS + [0, 4], np.uint8)[rs.randint(0, 7, size=size)]
        inst = lab.astype(np.uint16)
        inst[2:9, 3:17], lab[2:9, 3:17] = 26003, 26
        inst[12:20, 20:33], lab[12:20, 20:33] = 24999, 24
        arrays = {"image": rs.randint(0, 256, size=size + (3,)).astype(np.uint8), "label": lab, "instance": inst}
        for s in sub:
            Image.fromarray(arrays[s]).save(str(val / s / (stem + ".png")))
        made[stem] = (lab, inst)
    return val, made


def test_check_config_refusals(tmp_path):
    from contrastiveseg_amd.segmentor.tester import check_config, resolve_evaluator
    assert resolve_evaluator(_cfg()) == (None, None)                       # absent: nothing changes
    assert resolve_evaluator(_cfg(evaluator=None)) == (None, None)
    with pytest.raises(NotImplementedError, match=r"test\.evaluator 'ade20k' is not an evaluator"):
        check_config(_cfg(evaluator="ade20k"))
    ragged = {"size_mode": "diverse_size", "align_method": "only_pad", "pad_mode": "pad_right_down"}
    with pytest.raises(NotImplementedError, match=r"test\.evaluator 'cityscapes'.*diverse_size"):
        check_config(_cfg(evaluator="cityscapes", data_transformer=ragged))
    for bad in ([7, 11, 24, 26, 34], [7, 11, 24, 26, -1], [7, 11, 24, 26, 255]):
        with pytest.raises(ValueError, match=r"data\.label_list holds %d" % bad[-1]):
            check_config(_cfg(label_list=bad, evaluator="cityscapes"))
    with pytest.raises(ValueError, match=r"test\.instance_dir 7"):
        check_config(_cfg(evaluator="cityscapes", instance_dir=7))
    # directories and files, where the image directory is known
    val, _ = _dataset(tmp_path / "full")
    cfg = _cfg(evaluator="cityscapes", test_dir=str(val / "image"))
    assert check_config(cfg)[0] == "ss_test" and resolve_evaluator(cfg) == ("cityscapes", str(val / "instance"))
    other, _ = _dataset(tmp_path / "elsewhere", sub=("instance",))
    assert resolve_evaluator(_cfg(evaluator="cityscapes", test_dir=str(val / "image"), instance_dir=str(other / "instance")))[1] == \
        str(other / "instance")
    val, _ = _dataset(tmp_path / "nolabel", sub=("image", "instance"))
    with pytest.raises(FileNotFoundError, match=r"label directory .*nolabel.*label does not exist"):
        check_config(_cfg(evaluator="cityscapes", test_dir=str(val / "image")))
    val, _ = _dataset(tmp_path / "noinst", sub=("image", "label"))
    with pytest.raises(FileNotFoundError, match=r"test\.instance_dir .*noinst.*instance does not exist"):
        check_config(_cfg(evaluator="cityscapes", test_dir=str(val / "image")))
    val, _ = _dataset(tmp_path / "hole")
    os.remove(str(val / "instance" / "b_000000_000002.png"))
    with pytest.raises(FileNotFoundError, match=r"test\.instance_dir .* has no b_000000_000002\.png"):
        check_config(_cfg(evaluator="cityscapes", test_dir=str(val / "image")))
    os.remove(str(val / "label" / "a_000000_000001.png"))
    with pytest.raises(FileNotFoundError, match=r"label directory .* has no a_000000_000001\.png"):
        check_config(_cfg(evaluator="cityscapes", test_dir=str(val / "image")))


def test_the_shipped_config_switches_the_evaluator_on():
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tester import check_config, dataset_id_lut, resolve_evaluator
    cfg = Configer(configs=os.path.join(ROOT, "configs", "cityscapes", "H_48_D_4_TEST_EVAL.json"))
    assert check_config(cfg)[0] == "ms_test" and resolve_evaluator(cfg) == ("cityscapes", None)
    kept = [lab.id for lab in CS.LABELS if not lab.ignore_in_eval]
    assert cfg.get("data", "label_list") == kept and dataset_id_lut(cfg)[:19].tolist() == kept


# ---- 3. the loader ---------------------------------------------------------------------------------------------------------------------------
def test_loader_yields_the_raw_maps_at_the_pad_offset(tmp_path, monkeypatch):
    from PIL import Image
    from contrastiveseg_amd.lib.datasets.data_loader import DataLoader
    from tests.emu import inject
    inject.install(monkeypatch)                            # the loader's transform is a kernel: here on the emulated device
    val, made = _dataset(tmp_path)
    pad = {"size_mode": "fix_size", "input_size": [48, 32], "align_method": "only_pad", "pad_mode": "pad_center"}
    cpu = torch.device("cpu")
    plain = next(iter(DataLoader(_cfg(test_dir=str(val / "image"), batch_size=2, data_transformer=pad), cpu).get_testloader()))
    assert "labelmap_raw" not in plain and "instancemap" not in plain              # only with the switch
    batch = next(iter(DataLoader(_cfg(test_dir=str(val / "image"), batch_size=2, data_transformer=pad, evaluator="cityscapes"),
                                 cpu).get_testloader()))
    raw, inst = batch["labelmap_raw"], batch["instancemap"]
    assert raw.dtype == torch.uint8 and inst.dtype == torch.int16 and tuple(raw.shape) == tuple(inst.shape) == (2, 32, 48)
    assert torch.equal(plain["img"], batch["img"]) and torch.equal(plain["labelmap"], batch["labelmap"])
    for k, stem in enumerate(batch["name"]):
        (x0, y0), (bw, bh) = batch["pad_offset"][k], batch["border_size"][k]
        assert (x0, y0, bw, bh) == (4, 4, 40, 24)
        want_raw, want_inst = np.zeros((32, 48), np.uint8), np.zeros((32, 48), np.uint16)
        want_raw[y0:y0 + bh, x0:x0 + bw], want_inst[y0:y0 + bh, x0:x0 + bw] = made[stem]
        assert np.array_equal(raw[k].numpy(), want_raw)                          # the file's bytes: no label_list look-up
        assert np.array_equal(inst[k].numpy().view(np.uint16), want_inst)
    # an instance map of another size than its image; a file that is no integer map; a missing file
    Image.fromarray(np.zeros((24, 41), np.uint16)).save(str(val / "instance" / "b_000000_000002.png"))
    with pytest.raises(ValueError, match=r"b_000000_000002\.png: the instance map is 24 x 41, the image 24 x 40"):
        next(iter(DataLoader(_cfg(test_dir=str(val / "image"), batch_size=2, data_transformer=pad, evaluator="cityscapes"),
                             cpu).get_testloader()))
    Image.fromarray(np.zeros((24, 40, 3), np.uint8)).save(str(val / "instance" / "b_000000_000002.png"))
    with pytest.raises(ValueError, match=r"b_000000_000002\.png: an instance map must be a single-channel integer image"):
        next(iter(DataLoader(_cfg(test_dir=str(val / "image"), batch_size=2, data_transformer=pad, evaluator="cityscapes"),
                             cpu).get_testloader()))
    os.remove(str(val / "instance" / "b_000000_000002.png"))
    with pytest.raises(FileNotFoundError, match=r"test\.instance_dir .* has no b_000000_000002\.png"):
        DataLoader(_cfg(test_dir=str(val / "image"), batch_size=2, data_transformer=pad, evaluator="cityscapes"), cpu).get_testloader()


# ---- 4. two ranks over gloo ----------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_score(per_image, mine):
    """A host-side CityscapesScore holding the partials of the images `mine`, accumulated in that order."""
    from contrastiveseg_amd.lib.metrics.cityscapes_score import CityscapesScore
    score = CityscapesScore(np.zeros(256, np.uint8), "cpu")
    for k in mine:
        si, sf = _stat_arrays(per_image[k]["instStats"])
        score.conf += torch.tensor(per_image[k]["result"]["confMatrix"], dtype=torch.int64)
        score.stats_i += torch.from_numpy(si)
        score.stats_f += torch.from_numpy(sf)
    return score


def _worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per_image = _golden()["per_image"]
    score = _rank_score(per_image, range(len(per_image))[rank::world])          # the loader's strided share
    conf, si, sf = score.reduce_scores()
    result, acc = score.results()
    q.put((rank, conf.tolist(), si.tolist(), sf.tolist(), json.dumps(result), acc))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reproduce_the_one_rank_scores():
    import torch.multiprocessing as mp
    g = _golden()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    one = _rank_score(g["per_image"], range(len(g["per_image"])))
    one_conf, one_si, one_sf = one.reduce_scores()
    want_si, want_sf = _stat_arrays(g["all"]["instStats"])
    assert one_conf.tolist() == g["all"]["result"]["confMatrix"] and np.array_equal(one_si, want_si)
    n_inst = int(sum(len(np.unique(np.asarray(ids)[np.asarray(ids) > 1000])) for ids in _instance_maps(g)))
    bound = n_inst * 2.0 ** -52
    assert n_inst > 20
    for rank, conf, si, sf, result, acc in res:
        assert conf == g["all"]["result"]["confMatrix"] and si == want_si.tolist()
        sf = np.array(sf)
        assert np.all(np.abs(sf - want_sf) <= bound * want_sf), (sf, want_sf)
        assert acc == g["all"]["pixelAccuracy"]
        result = json.loads(result)
        for key in ("classScores", "categoryScores", "priors", "labels", "confMatrix"):          # functions of the matrix alone
            assert _same(result[key], g["all"]["result"][key]), key
        for key in ("classInstScores", "categoryInstScores"):
            for name, v in result[key].items():
                w = g["all"]["result"][key][name]
                assert (math.isnan(v) and math.isnan(w)) or abs(v - w) <= 4 * bound * w, (key, name, v, w)


def _instance_maps(g):
    from PIL import Image
    return [np.asarray(Image.open(os.path.join(GOLDEN, s + "_gtFine_instanceIds.png"))) for s in g["stems"]]
