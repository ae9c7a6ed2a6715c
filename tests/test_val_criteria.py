"""The validation pass of the contrast criteria: Trainer.validate() calls `pixel_loss(seg_net(img, is_eval=True), target)`, and the
evaluation forward returns `seg` / `embed` [/ `seg_aux`] only -- no memory queues. Every contrast criterion registered in
SEG_LOSS_DICT must then return its cross-entropy term (the reference's memory criteria return `loss + 0 * 0` there,
lib/loss/loss_contrast_mem.py:221-231); the memory criteria of this package used to call `.detach()` on a Python int instead, which
stopped hrnet_w48_mem / hrnet_w48_ocr_mem / deeplab_v3_mem at the first test_interval.

Checked against F.cross_entropy of the bilinearly upsampled logits in float64 (the aux criteria: the weighted sum of the two), at the
bar of test_upsample_ce_matches_torch_and_oracle (1e-5 relative, floor 1), on the emulated device and on the MI355X; and a
Trainer.validate() of one memory-bank model on the GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, NCLS, D, HW, LABEL_HW = 2, 7, 16, (8, 16), (32, 64)
AUX_W, SEG_W, CONTRAST_W = 0.4, 1.0, 0.1


def _configer(loss):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    contrast = dict(proj_dim=D, temperature=0.1, base_temperature=0.07, max_samples=64, max_views=4, loss_weight=CONTRAST_W,
                    use_rmi=False, use_lovasz=False, warmup_iters=0)
    if loss.startswith("mem"):
        contrast.update(with_memory=True, memory_size=8, pixel_update_freq=2)
    return Configer(config_dict={
        "data": {"num_classes": NCLS},
        "network": {"loss_weights": {"aux_loss": AUX_W, "seg_loss": SEG_W}},
        "contrast": contrast, "loss": {"loss_type": loss, "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


def _inputs():
    g = torch.Generator().manual_seed(23)
    seg = torch.randn(B, NCLS, *HW, generator=g) * 2.0
    aux = torch.randn(B, NCLS, *HW, generator=g) * 2.0
    embed = F.normalize(torch.randn(B, D, *HW, generator=g), dim=1)
    target = torch.randint(0, NCLS, (B,) + LABEL_HW, generator=g)
    target = target[:, ::8, ::8].repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()      # blocky: anchors of every class
    target[0, :3, :5] = -1
    target[1, 20, 40:47] = -1
    return seg, aux, embed, target


def _ce64(logits, target):
    up = F.interpolate(logits.double(), size=target.shape[-2:], mode="bilinear", align_corners=True)
    return float(F.cross_entropy(up, target, ignore_index=-1))


def _check_criteria(dev):
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    seg, aux, embed, target = _inputs()
    names = [n for n in SEG_LOSS_DICT if "contrast" in n]
    assert sorted(names) == ["contrast_auxce_loss", "contrast_ce_loss", "mem_contrast_auxce_loss", "mem_contrast_ce_loss"]
    for name in names:
        crit = SEG_LOSS_DICT[name](_configer(name)).to(dev).eval()
        want = _ce64(seg, target)
        preds = {"seg": seg.to(dev), "embed": embed.to(dev)}
        if "aux" in name:
            want = SEG_W * want + AUX_W * _ce64(aux, target)
            preds["seg_aux"] = aux.to(dev)
        for with_embed in (False, True):
            with torch.no_grad():
                torch.manual_seed(5)
                got = crit(preds, target.to(dev), with_embed=with_embed)
            ce, contrast = crit.last_terms
            assert got.dim() == 0 and ce.dim() == 0 and contrast.dim() == 0 and contrast.device == got.device, name
            assert bool(torch.isfinite(got)), name
            print(name, with_embed, float(got), want, float(contrast))
            assert abs(float(ce) - want) <= 1e-5 * max(1.0, abs(want)), (name, with_embed, float(ce), want)
            if name.startswith("mem"):
                assert float(contrast) == 0.0, (name, float(contrast))          # no queues in `preds`: the reference's `0`
            expect = want + (CONTRAST_W * float(contrast) if with_embed else 0.0)
            assert abs(float(got) - expect) <= 1e-5 * max(1.0, abs(expect)), (name, with_embed, float(got), expect)


def test_contrast_criteria_without_queues_on_the_emulated_device(monkeypatch):
    from tests.emu import inject
    inject.install(monkeypatch)
    _check_criteria(torch.device("cpu"))


@pytest.mark.gpu
def test_contrast_criteria_without_queues_on_the_mi355x():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _check_criteria(torch.device("cuda:0"))


@pytest.mark.gpu
def test_trainer_validate_of_a_memory_bank_model():
    """Trainer.validate() on hrnet_w48_mem (hrnet18 backbone, the sizes of tests/test_running_score.py): completes, a finite
    validation loss, and exactly the confusion matrix the reference arithmetic gives for the model's own predictions."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    dev = torch.device("cuda:0")
    cfg = Configer(configs=os.path.join(ROOT, "configs", "cityscapes", "H_48_D_4_MEM.json"))
    cfg.update(["network", "backbone"], "hrnet18")
    cfg.update(["network", "model_name"], "hrnet_w48_mem")
    cfg.update(["loss", "loss_type"], "mem_contrast_ce_loss")
    cfg.update(["data", "num_classes"], 7)
    cfg.get("loss", "params").pop("ce_weight", None)
    cfg.update(["train", "batch_size"], 2)
    cfg.get("train", "data_transformer")["input_size"] = [256, 128]
    cfg.update(["contrast", "memory_size"], 64)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    batches = list(SyntheticLoader(cfg, dev, length=2, mode="blocky", fixed=False))
    tr.validate(batches)
    assert np.isfinite(cfg.get("val_loss")) and cfg.get("val_loss") > 0
    got = tr.last_val_score.confusion_matrix.cpu().numpy()
    tr.seg_net.eval()
    want = np.zeros((7, 7), dtype=np.int64)
    with torch.no_grad():
        for b in batches:
            out = tr.seg_net(b["img"], is_eval=True)
            assert "segment_queue" not in out and "pixel_queue" not in out
            p = F.interpolate(out["seg"], size=b["labelmap"].shape[-2:], mode="bilinear", align_corners=True).argmax(1).cpu().numpy()
            t = b["labelmap"].cpu().numpy()
            m = (t >= 0) & (t < 7)
            want += np.bincount(7 * t[m] + p[m], minlength=49).reshape(7, 7)
    assert np.array_equal(got, want)
    assert abs(cfg.get("performance") - tr.last_val_score.get_mean_iou()) < 1e-12
