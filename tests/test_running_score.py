"""Validation metric parity: this package's on-device RunningScore against the reference's
numpy RunningScore (lib/metrics/running_score.py:120-215) -- integer confusion counts bit-exact, scores to 1e-12 --
on seeded label maps with ignored pixels, out-of-range predictions and classes that never occur. The reference's numbers
are a committed fixture produced by it (tests/golden/running_score.npz, oracle/make_golden.py)."""
import os

import numpy as np
import pytest
import torch



def _case(seed=5, K=19, shape=(3, 64, 96)):
    rs = np.random.RandomState(seed)
    true = rs.randint(-1, K, size=shape).astype(np.int64)
    true[0, :8] = 255                                # a stray out-of-range label value
    pred = rs.randint(0, K - 2, size=shape).astype(np.int64)       # classes K-2, K-1 never predicted
    true[true == 3] = 4                              # class 3 never occurs in the ground truth
    pred[pred == 3] = 5                              # ... nor in the prediction: nan IoU, skipped by nanmean
    return true, pred, K


def _mine(true, pred, K, dev):
    from contrastiveseg_amd.lib.metrics.running_score import RunningScore
    rs = RunningScore(num_classes=K, ignore_index=-1)
    t, p = torch.from_numpy(true).to(dev), torch.from_numpy(pred).to(dev)
    rs.update(p[:2], t[:2])
    rs.update(p[2:], t[2:])
    return rs


def test_running_score_matches_reference_class(golden_dir):
    """Every score of the reference's RunningScore class on the same label maps (tests/golden/running_score.npz)."""
    g = np.load(os.path.join(golden_dir, "running_score.npz"))
    true, pred, K = _case()
    mine = _mine(true, pred, K, "cpu")
    assert np.array_equal(mine.confusion_matrix.numpy(), g["confusion"])
    assert abs(mine.get_mean_iou() - float(g["mean_iou"])) < 1e-12
    assert abs(mine.get_pixel_acc() - float(g["pixel_acc"])) < 1e-12
    assert np.allclose(mine.get_mean_acc(), g["mean_acc"], equal_nan=True, atol=1e-12)
    assert np.allclose(list(mine.get_cls_iou().values()), g["cls_iou"], equal_nan=True)


def test_running_score_matches_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "running_score.npz"))
    true, pred, K = _case()
    mine = _mine(true, pred, K, "cpu")
    assert np.array_equal(mine.confusion_matrix.numpy(), g["confusion"])
    assert abs(mine.get_mean_iou() - float(g["mean_iou"])) < 1e-12


@pytest.mark.gpu
def test_running_score_on_device_and_trainer_val(golden_dir):
    """Confusion counts on the GPU are bit-exact against the reference fixture, and Trainer.validate() accumulates
    exactly the matrix that the reference arithmetic gives for the model's own predictions."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(golden_dir, "running_score.npz"))
    true, pred, K = _case()
    mine = _mine(true, pred, K, dev)
    assert np.array_equal(mine.confusion_matrix.cpu().numpy(), g["confusion"])
    assert abs(mine.get_mean_iou() - float(g["mean_iou"])) < 1e-12

    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Configer(configs=os.path.join(root, "configs", "cityscapes", "H_48_D_4.json"))
    cfg.update(["network", "backbone"], "hrnet18")
    cfg.update(["data", "num_classes"], 7)
    cfg.get("loss", "params").pop("ce_weight", None)
    cfg.update(["train", "batch_size"], 2)
    cfg.get("train", "data_transformer")["input_size"] = [256, 128]
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    loader = SyntheticLoader(cfg, dev, length=2, mode="blocky", fixed=False)
    batches = list(loader)
    tr.validate(batches)
    got = tr.last_val_score.confusion_matrix.cpu().numpy()
    tr.seg_net.eval()
    want = np.zeros((7, 7), dtype=np.int64)
    with torch.no_grad():
        for b in batches:
            seg = tr.seg_net(b["img"], is_eval=True)["seg"]
            p = torch.nn.functional.interpolate(seg, size=b["labelmap"].shape[-2:], mode="bilinear",
                                                align_corners=True).argmax(1).cpu().numpy()
            t = b["labelmap"].cpu().numpy()
            m = (t >= 0) & (t < 7)
            want += np.bincount(7 * t[m] + p[m], minlength=49).reshape(7, 7)        # reference :143-153
    assert np.array_equal(got, want)
    assert abs(cfg.get("performance") - tr.last_val_score.get_mean_iou()) < 1e-12
