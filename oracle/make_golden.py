"""
ORACLE -- test infrastructure only. Generates tests/golden/*.npz by running the REFERENCE ITSELF
(/root/reference, CPU, fp32) on the seeded synthetic inputs of cseg_oracle.synth_case. Run in the build
container only:   PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden.py [--only NAME]

What is stored per loss case (inputs are regenerated from the seed, never stored):
  total / ce / contrast loss scalars, n_view, the mined anchors as (image, class, pixel index) triples in the
  reference's order (recovered by feeding index-encoding features through the reference's
  _hard_anchor_sampling, lib/loss/loss_contrast.py:30-89), and for the small cases the autograd gradients
  w.r.t. seg (dense) and embed (rows at the mined pixels).
"""
import argparse
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shim  # noqa: E402
from oracle import cseg_oracle as O  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

CITYSCAPES_W = [0.8373, 0.9180, 0.8660, 1.0345, 1.0166, 0.9969, 0.9754, 1.0489, 0.8786, 1.0023, 0.9539,
                0.9843, 1.1116, 0.9037, 1.0865, 1.0955, 1.0865, 1.1529, 1.0507]

# name -> dict(seed, B, K, H, W, stride, D, blocky, contrast overrides, loss_type, ce_weight, grads, torch_seed)
LOSS_CASES = {
    "small_self": dict(seed=11, B=2, K=5, H=64, W=128, stride=4, D=16, blocky=True, loss="contrast_ce_loss",
                       contrast=dict(max_samples=64, max_views=10, temperature=0.1, loss_weight=0.1),
                       ce_weight=[0.9, 1.1, 1.0, 0.8, 1.2], grads=True, torch_seed=304),
    "mid_self": dict(seed=12, B=4, K=19, H=128, W=256, stride=4, D=64, blocky=True, loss="contrast_ce_loss",
                     contrast=dict(max_samples=1024, max_views=100, temperature=0.1, loss_weight=0.1),
                     ce_weight=CITYSCAPES_W, grads=True, torch_seed=7),
    "uniform_self": dict(seed=13, B=3, K=19, H=128, W=256, stride=4, D=32, blocky=False, loss="contrast_ce_loss",
                         contrast=dict(max_samples=1024, max_views=50, temperature=0.07, loss_weight=1.0),
                         ce_weight=None, grads=True, torch_seed=304),
    "odd_stride8_aux": dict(seed=14, B=2, K=7, H=97, W=161, stride=8, D=24, blocky=True,
                            loss="contrast_auxce_loss", hw=(13, 21),
                            contrast=dict(max_samples=128, max_views=6, temperature=0.1, loss_weight=0.1),
                            ce_weight=None, grads=True, torch_seed=5),
    "warmup_self": dict(seed=15, B=2, K=5, H=64, W=128, stride=4, D=16, blocky=True, loss="contrast_ce_loss",
                        contrast=dict(max_samples=64, max_views=10, temperature=0.1, loss_weight=0.1),
                        ce_weight=None, grads=True, torch_seed=304, with_embed=False),
    "mem_v1": dict(seed=16, B=4, K=19, H=128, W=256, stride=4, D=64, blocky=True, loss="mem_contrast_ce_loss",
                   contrast=dict(max_samples=1024, max_views=1, temperature=0.07, loss_weight=1.0,
                                 with_memory=True, memory_size=12, pixel_update_freq=10),
                   ce_weight=CITYSCAPES_W, grads=True, torch_seed=304),
    "mem_v3": dict(seed=17, B=2, K=6, H=64, W=128, stride=4, D=32, blocky=True, loss="mem_contrast_ce_loss",
                   contrast=dict(max_samples=48, max_views=3, temperature=0.1, loss_weight=0.5,
                                 with_memory=True, memory_size=20, pixel_update_freq=10),
                   ce_weight=None, grads=True, torch_seed=9),
    # BASELINE.json configs[1] loss shapes (HRNet-W48 head outputs, bs8, 512x1024, D=256): scalars + indices only
    "cfg2_full": dict(seed=304, B=8, K=19, H=512, W=1024, stride=4, D=256, blocky=True, n_rect=24,
                      loss="contrast_ce_loss",
                      contrast=dict(max_samples=1024, max_views=100, temperature=0.1, loss_weight=0.1),
                      ce_weight=CITYSCAPES_W, grads="subset", torch_seed=304),
    # BASELINE.json configs[3] / [4] criteria (row g of the coverage table): FSAuxCELoss + the memory-bank contrast term. The
    # reference registers no such criterion (its loss_contrast_mem.ContrastAuxCELoss is broken), so the
    # golden COMPOSES the reference's own pieces (RefMemAuxCE below): DeepLab feature size 65x129 with the 4104-column bank of
    # configs/cityscapes/R_101_D_8_MEM.json, and the OCR / COCO-Stuff shape 130x130 with 171 classes.
    "mem_aux_deeplab": dict(seed=18, B=2, K=19, H=512, W=1024, stride=8, D=64, blocky=True, n_rect=24, hw=(65, 129),
                            loss="mem_contrast_auxce_loss",
                            contrast=dict(max_samples=1024, max_views=1, temperature=0.07, loss_weight=1.0,
                                          with_memory=True, memory_size=108, pixel_update_freq=10),
                            ce_weight=CITYSCAPES_W, grads=True, torch_seed=304),
    "mem_aux_ocr": dict(seed=19, B=2, K=171, H=520, W=520, stride=4, D=64, blocky=True, n_rect=10, hw=(130, 130),
                        loss="mem_contrast_auxce_loss",
                        contrast=dict(max_samples=1024, max_views=4, temperature=0.07, loss_weight=1.0,
                                      with_memory=True, memory_size=8, pixel_update_freq=10),
                        ce_weight=None, grads="subset", torch_seed=11),
    "cfg2_uniform": dict(seed=305, B=8, K=19, H=512, W=1024, stride=4, D=256, blocky=False,
                         loss="contrast_ce_loss",
                         contrast=dict(max_samples=1024, max_views=100, temperature=0.1, loss_weight=0.1),
                         ce_weight=CITYSCAPES_W, grads=False, torch_seed=304),
}


def case_inputs(c):
    target, seg, embed = O.synth_case(c["seed"], c["B"], c["K"], c["H"], c["W"], c["stride"], c["D"],
                                      blocky=c["blocky"], n_rect=c.get("n_rect", 14))
    if "hw" in c:   # feature size not H//stride (DeepLab ceil-mode sizes): regenerate seg/embed at that size
        h, w = c["hw"]
        rs = np.random.RandomState(c["seed"] + 1000)
        lab = O.nearest_downsample_labels(target, h, w)
        onehot = (lab[:, None] == np.arange(c["K"])[None, :, None, None]).astype(np.float32)
        seg = (onehot * 4.0 + rs.standard_normal((c["B"], c["K"], h, w)) * 2.0).astype(np.float32)
        e = rs.standard_normal((c["B"], c["D"], h, w)).astype(np.float32)
        embed = (e / np.sqrt((e.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)
    extra = {}
    rs = np.random.RandomState(c["seed"] + 2000)
    if c["loss"] in ("contrast_auxce_loss", "mem_contrast_auxce_loss"):
        extra["seg_aux"] = (seg * 0.5 + rs.standard_normal(seg.shape) * 1.0).astype(np.float32)
    if c["loss"].startswith("mem_"):
        ms = c["contrast"]["memory_size"]
        for name in ("segment_queue", "pixel_queue"):
            q = rs.standard_normal((c["K"], ms, c["D"])).astype(np.float32)
            extra[name] = (q / np.sqrt((q.astype(np.float64) ** 2).sum(2, keepdims=True))).astype(np.float32)
    return target, seg, embed, extra


def ref_mem_auxce(cfg):
    """FSAuxCELoss + memory-bank PixelContrastLoss, composed from the reference's own classes exactly as its two registered
    criteria compose theirs: the segmentation part of lib/loss/loss_contrast.py:ContrastAuxCELoss.forward (:213-234: both
    heads upsampled to the label size, FSAuxCELoss([aux, seg])) and the contrast part of
    lib/loss/loss_contrast_mem.py:ContrastCELoss.forward (:198-231: queue = cat(segment, pixel), predict = argmax seg)."""
    import torch
    import torch.nn.functional as F
    from lib.loss.loss_helper import FSAuxCELoss
    from lib.loss.loss_contrast_mem import PixelContrastLoss

    class RefMemAuxCE(torch.nn.Module):
        def __init__(self):
            super(RefMemAuxCE, self).__init__()
            self.loss_weight = cfg.get('contrast', 'loss_weight')
            self.seg_criterion = FSAuxCELoss(configer=cfg)
            self.contrast_criterion = PixelContrastLoss(configer=cfg)

        def forward(self, preds, target, with_embed=False):
            h, w = target.size(1), target.size(2)
            seg, seg_aux = preds['seg'], preds['seg_aux']
            pred = F.interpolate(input=seg, size=(h, w), mode='bilinear', align_corners=True)
            pred_aux = F.interpolate(input=seg_aux, size=(h, w), mode='bilinear', align_corners=True)
            loss = self.seg_criterion([pred_aux, pred], target)
            queue = torch.cat((preds['segment_queue'], preds['pixel_queue']), dim=1)
            _, predict = torch.max(seg, 1)
            loss_contrast = self.contrast_criterion(preds['embed'], target, predict, queue)
            if with_embed is True:
                return loss + self.loss_weight * loss_contrast
            return loss + 0 * loss_contrast
    return RefMemAuxCE()


def run_loss_case(name, c):
    import torch
    ref_shim.install()
    from lib.loss.loss_manager import SEG_LOSS_DICT
    cfg = ref_shim.configer(num_classes=c["K"], loss_type=c["loss"] if c["loss"] in SEG_LOSS_DICT else "mem_contrast_ce_loss",
                            contrast=c["contrast"], ce_weight=c["ce_weight"])
    crit = ref_mem_auxce(cfg) if c["loss"] == "mem_contrast_auxce_loss" else SEG_LOSS_DICT[c["loss"]](cfg)
    target, seg, embed, extra = case_inputs(c)
    t_target = torch.from_numpy(target)
    t_seg = torch.from_numpy(seg).requires_grad_(True)
    t_embed = torch.from_numpy(embed).requires_grad_(True)
    preds = {"seg": t_seg, "embed": t_embed}
    leaves = {"seg": t_seg, "embed": t_embed}
    for k, v in extra.items():
        preds[k] = torch.from_numpy(v)
        if k == "seg_aux":
            preds[k].requires_grad_(True)
            leaves[k] = preds[k]
    with_embed = c.get("with_embed", True)

    torch.manual_seed(c["torch_seed"])
    total = crit(preds, t_target, with_embed=with_embed)
    out = {"total": float(total.detach())}
    if c["grads"]:
        total.backward()

    # separate terms, same RNG position
    with torch.no_grad():
        h, w = seg.shape[-2:]
        _, predict = torch.max(t_seg, 1)
        torch.manual_seed(c["torch_seed"])
        if c["loss"].startswith("mem_"):
            queue = torch.cat((preds["segment_queue"], preds["pixel_queue"]), dim=1)
            lc = crit.contrast_criterion(t_embed, t_target, predict, queue)
        else:
            lc = crit.contrast_criterion(t_embed, t_target, predict)
        out["contrast"] = float(lc)
        # mined anchors: feed index-encoding features through the reference sampler
        B, D = embed.shape[:2]
        P = h * w
        enc = torch.zeros(B, P, 2)
        enc[:, :, 0] = torch.arange(B).view(B, 1).float()
        enc[:, :, 1] = torch.arange(P).view(1, P).float()
        labels = torch.nn.functional.interpolate(t_target.unsqueeze(1).float(), (h, w), mode="nearest")
        labels = labels.squeeze(1).long().view(B, -1)
        torch.manual_seed(c["torch_seed"])
        X_, y_ = crit.contrast_criterion._hard_anchor_sampling(enc, labels, predict.view(B, -1))
        out["n_view"] = int(X_.shape[1])
        out["anchor_img"] = X_[:, :, 0].long().numpy()          # [T, n_view]
        out["anchor_pix"] = X_[:, :, 1].long().numpy()          # [T, n_view]
        out["anchor_cls"] = y_.long().numpy()                   # [T]
        out["labels_ds"] = labels.numpy().astype(np.int16)
        out["predict"] = predict.view(B, -1).numpy().astype(np.int16)
    if c["grads"] == "subset":
        # headline shapes: dense gradients would be 20 + 268 MB; keep a strided slice of d_seg of every image and
        # every GRAD_ROW_STEP-th anchor row of d_embed (class-major, view order)
        out["d_seg_s%d" % GRAD_SEG_STEP] = t_seg.grad.numpy()[:, :, ::GRAD_SEG_STEP, ::GRAD_SEG_STEP].copy()
        g = t_embed.grad.numpy().reshape(embed.shape[0], embed.shape[1], -1)
        img = out["anchor_img"].reshape(-1)[::GRAD_ROW_STEP]
        pix = out["anchor_pix"].reshape(-1)[::GRAD_ROW_STEP]
        out["d_embed_rows_s%d" % GRAD_ROW_STEP] = g[img, :, pix]
        out["d_embed_abs_sum"] = float(np.abs(t_embed.grad.numpy().astype(np.float64)).sum())
        out["d_seg_abs_sum"] = float(np.abs(t_seg.grad.numpy().astype(np.float64)).sum())
        if "seg_aux" in leaves:
            out["d_seg_aux_s%d" % GRAD_SEG_STEP] = leaves["seg_aux"].grad.numpy()[:, :, ::GRAD_SEG_STEP, ::GRAD_SEG_STEP].copy()
    elif c["grads"]:
        out["d_seg"] = t_seg.grad.numpy()
        g = t_embed.grad.numpy().reshape(embed.shape[0], embed.shape[1], -1)
        img = out["anchor_img"].reshape(-1)
        pix = out["anchor_pix"].reshape(-1)
        out["d_embed_rows"] = g[img, :, pix]                     # [T*n_view, D] in (class-major, view) order
        mask = np.ones(g.shape, dtype=bool)
        mask[img, :, pix] = False
        out["d_embed_rest_absmax"] = float(np.abs(g[mask]).max()) if mask.any() else 0.0
        if "seg_aux" in leaves:
            out["d_seg_aux"] = leaves["seg_aux"].grad.numpy()
    out["ce"] = out["total"] - (c["contrast"]["loss_weight"] if with_embed else 0.0) * out["contrast"]
    np.savez_compressed(os.path.join(OUT, "loss_%s.npz" % name), **out)
    print("loss_%s: total %.6f contrast %.6f n_view %d T %d" % (name, out["total"], out["contrast"],
                                                                 out["n_view"], len(out["anchor_cls"])))


GRAD_SEG_STEP = 4       # cfg2_full: d_seg[:, :, ::4, ::4]
GRAD_ROW_STEP = 8       # cfg2_full: every 8th anchor row of d_embed

ENQ_CASES = {
    "enq_a": dict(seed=21, B=3, K=7, H=64, W=128, kstride=4, D=16, network_stride=8, memory_size=9,
                  pixel_update_freq=4, torch_seed=304, rounds=3),
    "enq_b": dict(seed=22, B=2, K=19, H=128, W=256, kstride=4, D=32, network_stride=8, memory_size=50,
                  pixel_update_freq=10, torch_seed=11, rounds=2),
}


def enq_inputs(c, r):
    target, _, embed = O.synth_case(c["seed"] + 31 * r, c["B"], c["K"], c["H"], c["W"], c["kstride"], c["D"],
                                    blocky=True)
    return target, embed


def enq_init(c):
    rs = np.random.RandomState(c["seed"] + 500)
    sq = rs.standard_normal((c["K"], c["memory_size"], c["D"])).astype(np.float32)
    pq = rs.standard_normal((c["K"], c["memory_size"], c["D"])).astype(np.float32)
    return sq, pq


def run_enq_case(name, c):
    import torch
    ref_shim.install()
    # segmentor/trainer_contrastive.py imports the whole data/vis stack; _dequeue_and_enqueue only reads three
    # attributes of self, so bind the unmodified function to a bare namespace.
    import importlib
    for m in ("lib.vis.seg_visualizer", "lib.datasets.data_loader", "segmentor.tools.evaluator"):
        if m not in sys.modules:
            stub = types.ModuleType(m)
            stub.SegVisualizer = object
            stub.DataLoader = object
            stub.get_evaluator = lambda *a, **k: None
            sys.modules[m] = stub
    tc = importlib.import_module("segmentor.trainer_contrastive")
    me = types.SimpleNamespace(network_stride=c["network_stride"], memory_size=c["memory_size"],
                               pixel_update_freq=c["pixel_update_freq"])
    sq, pq = enq_init(c)
    sq, pq = torch.from_numpy(sq), torch.from_numpy(pq)
    sp = torch.zeros(c["K"], dtype=torch.long)
    pp = torch.zeros(c["K"], dtype=torch.long)
    torch.manual_seed(c["torch_seed"])
    out = {}
    for r in range(c["rounds"]):
        target, embed = enq_inputs(c, r)
        tc.Trainer._dequeue_and_enqueue(me, torch.from_numpy(embed), torch.from_numpy(target), sq, sp, pq, pp)
        out["segment_queue_%d" % r] = sq.numpy().copy()
        out["pixel_queue_%d" % r] = pq.numpy().copy()
        out["segment_ptr_%d" % r] = sp.numpy().copy()
        out["pixel_ptr_%d" % r] = pp.numpy().copy()
    np.savez_compressed(os.path.join(OUT, "%s.npz" % name), **out)
    print(name, "ptrs", sp.tolist(), pp.tolist())


MODEL_CASES = {
    "hrnet_w48_contrast": dict(backbone="hrnet48", K=19, B=2, H=64, W=128, seed=31, contrast={}),
    "hrnet_w48_ocr_contrast": dict(backbone="hrnet48", K=19, B=2, H=64, W=96, seed=32, contrast={}),
    # eval-mode BN here: the ASPP image-pool BN sees only B=2 values per channel in train mode, which amplifies
    # fp32 rounding differences by up to 1/sqrt(eps) -- an ill-conditioned comparison, not a property of the model
    # (round 3: `prime` -- the running statistics are first set to the batch statistics of this input by one train-mode pass
    # with momentum 1, prime_bn below; with the untrained statistics (mean 0, variance 1) the activations grew through 100 layers
    # to logits of 1.5e5, where an absolute 1e-3 means nothing. Primed, the logits are O(1) and the north_star bar applies.)
    # `head_scale`: the last layer of both classifiers is multiplied by 0.1 after the seeded initialisation (scale_heads below), on
    # both sides of the comparison. At its random initialisation DeepLab's logits reach |11-15| and the reference's own fp32
    # forward sits 1.6e-3 away from the fp64 evaluation of the same network whatever the batch (measured: eval / train mode,
    # B = 6 / 12 / 16) -- 1e-4 of the logit scale, like HRNet, but HRNet's logits are O(1). With O(1) logits the reference is within
    # 2e-4 of fp64 and the north_star bar (absolute 1e-3) is a meaningful assertion for DeepLab too.
    "deeplab_v3_contrast": dict(backbone="deepbase_resnet101_dilated8", K=19, B=6, H=65, W=97, seed=33, contrast={},
                                mode="eval", prime=True, spread=True, head_scale=0.1),
    # train-mode BN with B=6 so that the image-pool BN of the ASPP head sees six values per channel
    "deeplab_v3_contrast_train": dict(model="deeplab_v3_contrast", backbone="deepbase_resnet101_dilated8", K=19, B=6,
                                      H=97, W=129, seed=35, contrast={}, spread=True, head_scale=0.1),
    # THE BENCHED CONFIGURATION (BASELINE.json configs[1]): HRNet-W48 at 3x512x1024, features 128x256. On the GPU this
    # reaches the same MIOpen solvers as bench.py (shipped miopen_db records active). seg stored dense.
    "hrnet_w48_contrast_fullres": dict(model="hrnet_w48_contrast", backbone="hrnet48", K=19, B=2, H=512, W=1024,
                                       seed=34, contrast={}, embed_step=8),
    # the benched BATCH (8 images: with the grid-fill thresholds of kernels.py this reaches the 96- / 192- / 384-channel branch
    # kernels and every other default route of bench.py inside ONE reference-pinned forward); logits stored every 2nd pixel
    "hrnet_w48_contrast_fullres_b8": dict(model="hrnet_w48_contrast", backbone="hrnet48", K=19, B=8, H=512, W=1024,
                                          seed=37, contrast={}, embed_step=16, seg_step=2),
    # memory-bank wrapper: forward(img, labels) -> seg / embed / key / lb_key (nets/hrnet.py:178-188 of the reference)
    "hrnet_w48_mem": dict(backbone="hrnet48", K=19, B=2, H=64, W=128, seed=36, with_labels=True,
                          contrast=dict(with_memory=True, memory_size=16, pixel_update_freq=10)),
}


def model_input(c):
    rs = np.random.RandomState(c["seed"])
    x = rs.standard_normal((c["B"], 3, c["H"], c["W"])).astype(np.float32)
    if c.get("spread"):
        # per-image contrast and brightness like real photographs: without it the image-level pooled features of
        # i.i.d. noise images are nearly identical, and a train-mode BN over B such values (ASPP image pooling) divides
        # rounding noise by a vanishing batch variance -- an ill-conditioned comparison for ANY two implementations
        gain = np.linspace(0.4, 1.6, c["B"]).astype(np.float32).reshape(-1, 1, 1, 1)
        bias = np.linspace(-0.8, 0.8, c["B"]).astype(np.float32).reshape(-1, 1, 1, 1)
        x = x * gain + bias * np.array([1.0, -0.5, 0.25], dtype=np.float32).reshape(1, 3, 1, 1)
    return x


HEAD_LAST_LAYERS = ("decoder.refine.2.", "decoder.layer_dsn.2.")          # DeepLabHead: final 1x1 of the classifier / the DSN head


def scale_heads(net, factor):
    import torch
    with torch.no_grad():
        hit = 0
        for n, p in net.named_parameters():
            if n.startswith(HEAD_LAST_LAYERS):
                p.mul_(factor)
                hit += 1
        assert hit >= 2, "no classifier parameters found to scale"


def set_bn_eval(net):
    import torch.nn as nn
    for m in net.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.eval()


def prime_bn(net, x):
    """running statistics := batch statistics of x (one train-mode forward with momentum 1, no gradient); every module's
    train / eval flag is restored afterwards (net.train() would switch the frozen dropout layers back on)."""
    import torch
    import torch.nn as nn
    bns = [m for m in net.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    saved = [m.momentum for m in bns]
    flags = [(m, m.training) for m in net.modules()]
    for m in bns:
        m.momentum = 1.0
    net.train()
    freeze_dropout(net)
    with torch.no_grad():
        net(x.detach(), with_embed=True)
    for m, mom in zip(bns, saved):
        m.momentum = mom
    for m, t in flags:
        m.training = t


def freeze_dropout(net):
    import torch.nn as nn
    for m in net.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
            m.eval()            # the only stochastic layer; BN stays in train mode (batch statistics)


def model_labels(c):
    rs = np.random.RandomState(c["seed"] + 7)
    return rs.randint(-1, c["K"], size=(c["B"], c["H"], c["W"])).astype(np.int64)


def run_model_case(name, c):
    """Reference model (seed 304 init, train-mode BN, dropout off) forward on a seeded input; stores the logits and a
    strided slice of the embedding. The repo's models are seed-identical (tests/test_models_vs_reference.py), so a
    GPU forward of the repo's model under the same seed must reproduce these within 1e-3."""
    import torch
    ref_shim.install()
    from lib.models.model_manager import ModelManager
    cfg = ref_shim.configer(num_classes=c["K"], model_name=c.get("model", name), backbone=c["backbone"],
                            contrast=c["contrast"])
    torch.manual_seed(304)
    net = ModelManager(cfg).semantic_segmentor().train()
    freeze_dropout(net)
    if c.get("head_scale"):
        scale_heads(net, c["head_scale"])
    if c.get("prime"):
        prime_bn(net, torch.from_numpy(model_input(c)))
    if c.get("mode") == "eval":
        net.eval()
    with torch.no_grad():
        if c.get("with_labels"):
            out = net(torch.from_numpy(model_input(c)), torch.from_numpy(model_labels(c)), with_embed=True)
        else:
            out = net(torch.from_numpy(model_input(c)), with_embed=True)
    es = c.get("embed_step", 4)
    ss = c.get("seg_step", 1)
    res = {"embed_s%d" % es: out["embed"][:, :, ::es, ::es].numpy().copy(), "embed_shape": np.array(out["embed"].shape)}
    if ss == 1:
        res["seg"] = out["seg"].numpy()
    else:
        res["seg_s%d" % ss] = out["seg"][:, :, ::ss, ::ss].numpy().copy()
        res["seg_absmax"] = np.array(float(out["seg"].abs().max()))
    if "seg_aux" in out:
        res["seg_aux"] = out["seg_aux"].numpy()
    if "key" in out:
        assert torch.equal(out["key"], out["embed"]) and torch.equal(out["lb_key"], torch.from_numpy(model_labels(c)))
        res["has_key"] = np.array(1)
    # the reference's OWN fp32 rounding noise on this input: same weights and input in fp64 (input widened exactly)
    net64 = net.double()
    with torch.no_grad():
        x64 = torch.from_numpy(model_input(c)).double()
        out64 = net64(x64, torch.from_numpy(model_labels(c)), with_embed=True) if c.get("with_labels") else \
            net64(x64, with_embed=True)
    res["seg_fp32_noise"] = np.array(float((out64["seg"] - out["seg"].double()).abs().max()))
    res["embed_fp32_noise"] = np.array(float((out64["embed"] - out["embed"].double()).abs().max()))
    np.savez_compressed(os.path.join(OUT, "model_%s.npz" % name), **res)
    print("model_%s: seg %s absmax %.4f embed %s; reference fp32-vs-fp64 noise: seg %.2e embed %.2e" % (
        name, tuple(out["seg"].shape), float(out["seg"].abs().max()), tuple(out["embed"].shape),
        float(res["seg_fp32_noise"]), float(res["embed_fp32_noise"])))


# ---------------------------------------------------------------------------------------------------------------
# One SGD step through the whole network (backward through the backbone): model + criterion + SGD driven exactly as
# segmentor/trainer_contrastive.py:204-261 does (forward, loss, [_dequeue_and_enqueue], zero_grad, backward, step),
# dropout frozen, then a second forward+loss on the same batch. Stored: both losses, the gradient w.r.t. the input image
# and gradients + SGD updates of a few tensors spread over the network (strided subsets), and -- because fp32 backward
# through a 100+ layer BatchNorm network at its random initialisation is badly conditioned -- the SAME gradients from
# the reference evaluated in fp64 (`grad64/*`, the ground truth) with the reference's own fp32-vs-fp64 deviation
# (`gradnoise/*`, max-norm relative): measured 1e-2..7e-2 for backbone tensors and the input gradient, 1e-5 for the
# last head layers (a conv weight gradient in front of a BN sums products whose mean component cancels exactly only in
# exact arithmetic). Two fp32 implementations with different summation orders therefore cannot agree to 1e-3 on those
# tensors; the parity tests bound the distance to the fp64 truth by max(1e-3, 3 x the reference's own deviation).
# ---------------------------------------------------------------------------------------------------------------
STEP_CASES = {
    "step_hrnet48_contrast": dict(model="hrnet_w48_contrast", backbone="hrnet48", loss="contrast_ce_loss", K=7, B=2,
                                  H=128, W=256, seed=41, torch_seed=304,
                                  contrast=dict(max_samples=256, max_views=16, proj_dim=64),
                                  watch=["backbone.conv1.weight", "backbone.layer1.0.downsample.0.weight",
                                         "backbone.stage2.0.branches.1.3.bn2.weight",
                                         "backbone.stage3.1.fuse_layers.2.0.0.0.weight",
                                         "backbone.stage4.2.fuse_layers.0.3.0.weight",
                                         "backbone.stage4.0.branches.3.0.conv1.weight",
                                         "cls_head.0.weight", "cls_head.3.weight", "proj_head.proj.1.0.weight",
                                         "proj_head.proj.2.weight"]),
    "step_hrnet48_ocr": dict(model="hrnet_w48_ocr_contrast", backbone="hrnet48", loss="contrast_auxce_loss", K=7, B=2,
                             H=128, W=192, seed=42, torch_seed=11,
                             contrast=dict(max_samples=256, max_views=16, proj_dim=64),
                             watch=["backbone.conv1.weight", "backbone.stage3.0.fuse_layers.1.0.0.0.weight",
                                    "conv3x3.0.weight", "ocr_distri_head.object_context_block.f_pixel.0.weight",
                                    "ocr_distri_head.object_context_block.f_object.0.weight",
                                    "ocr_distri_head.object_context_block.f_up.0.weight",
                                    "ocr_distri_head.conv_bn_dropout.0.weight", "cls_head.weight", "aux_head.2.weight",
                                    "proj_head.proj.2.weight"]),
    "step_hrnet48_mem": dict(model="hrnet_w48_mem", backbone="hrnet48", loss="mem_contrast_ce_loss", K=7, B=2,
                             H=128, W=256, seed=43, torch_seed=304, network_stride=8,
                             contrast=dict(max_samples=256, max_views=1, proj_dim=256, with_memory=True,
                                           memory_size=12, pixel_update_freq=10, loss_weight=1.0),
                             watch=["encoder_q.backbone.conv1.weight",
                                    "encoder_q.backbone.stage4.2.fuse_layers.0.3.0.weight",
                                    "encoder_q.cls_head.0.weight", "encoder_q.proj_head.proj.0.weight",
                                    "encoder_q.proj_head.proj.2.weight"]),
    "step_resnet50_deeplab": dict(model="deeplab_v3_contrast", backbone="deepbase_resnet50_dilated8",
                                  loss="contrast_auxce_loss", K=7, B=4, H=97, W=129, seed=44, torch_seed=5, spread=True,
                                  contrast=dict(max_samples=128, max_views=8, proj_dim=64),
                                  watch=["backbone.resinit.conv1.weight", "backbone.layer2.0.downsample.0.weight",
                                         "backbone.layer4.2.conv2.weight", "decoder.layer_aspp.b0.0.weight",
                                         "decoder.layer_aspp.b1.0.weight", "decoder.layer_aspp.b4.1.weight", "decoder.layer_aspp.project.0.weight",
                                         "decoder.layer_dsn.0.weight", "decoder.refine.2.weight",
                                         "proj_head.proj.2.weight"]),
    # BASELINE.json configs[3] names ResNet-101 (resnet_models.py:107-178 of the reference): the same step on the real depth
    # (23 dilated blocks in layer3), round 4 -- the R-50 case above stays as the quick one.
    "step_resnet101_deeplab": dict(model="deeplab_v3_contrast", backbone="deepbase_resnet101_dilated8",
                                   loss="contrast_auxce_loss", K=7, B=4, H=97, W=129, seed=47, torch_seed=5, spread=True,
                                   contrast=dict(max_samples=128, max_views=8, proj_dim=64),
                                   watch=["backbone.resinit.conv1.weight", "backbone.layer2.0.downsample.0.weight",
                                          "backbone.layer3.11.conv2.weight", "backbone.layer3.22.conv3.weight",
                                          "backbone.layer4.2.conv2.weight", "decoder.layer_aspp.b1.0.weight",
                                          "decoder.layer_aspp.project.0.weight", "decoder.layer_dsn.0.weight",
                                          "decoder.refine.2.weight", "proj_head.proj.2.weight"]),
    # Frozen-statistics backward (round 3): the same network with BatchNorm in eval mode on statistics primed from this batch
    # (prime_bn) -- the adjoint of the eval-mode BN kernels inside a whole-network step. It was also an experiment (VERDICT r2
    # weak 3): does removing the batch-statistics terms make fp32 backward well conditioned? It does not: the reference's own fp32
    # gradients still sit 1e-2..2e-2 (max-norm) from the fp64 evaluation of the same function in the backbone (2e-5..4e-5 in the
    # last head layers), so the deviation comes from the depth of the ReLU network itself (pre-activations within rounding of
    # zero), not from the statistics. The noise-aware bounds stay; the second loss is not compared (an SGD step of lr 0.01 on
    # frozen statistics leaves the primed operating point: loss 1e5 in the reference too).
    "step_hrnet48_contrast_evalbn": dict(model="hrnet_w48_contrast", backbone="hrnet48", loss="contrast_ce_loss", K=7, B=2,
                                         H=128, W=256, seed=46, torch_seed=304, bn_eval=True, skip_loss1=True,
                                         contrast=dict(max_samples=256, max_views=16, proj_dim=64),
                                         watch=["backbone.conv1.weight", "backbone.layer1.0.conv2.weight",
                                                "backbone.stage2.0.branches.0.1.conv1.weight",
                                                "backbone.stage3.1.fuse_layers.2.0.0.0.weight",
                                                "backbone.stage3.2.branches.2.0.conv2.weight",
                                                "backbone.stage4.2.fuse_layers.0.3.0.weight",
                                                "backbone.stage4.0.branches.3.0.conv1.weight",
                                                "cls_head.0.weight", "cls_head.3.weight", "proj_head.proj.0.weight",
                                                "proj_head.proj.2.weight"]),
    # BASELINE.json configs[3] (row g): DeepLab-V3 + the per-class memory bank. The reference registers a memory model only
    # for HRNet (lib/models/nets/hrnet.py:153-188); the golden runs the reference's OWN HRNet_W48_MEM class with its encoder
    # symbol pointed at the reference's DeepLabV3Contrast (ref_memory_model below), the composed criterion ref_mem_auxce and
    # the reference's _dequeue_and_enqueue.
    "step_resnet50_deeplab_mem": dict(model="deeplab_v3_mem", backbone="deepbase_resnet50_dilated8",
                                      loss="mem_contrast_auxce_loss", K=7, B=4, H=97, W=129, seed=45, torch_seed=5,
                                      spread=True, network_stride=8,
                                      contrast=dict(max_samples=128, max_views=1, proj_dim=64, with_memory=True,
                                                    memory_size=12, pixel_update_freq=10, loss_weight=1.0),
                                      watch=["encoder_q.backbone.resinit.conv1.weight",
                                             "encoder_q.backbone.layer4.2.conv2.weight",
                                             "encoder_q.decoder.layer_aspp.project.0.weight",
                                             "encoder_q.decoder.layer_dsn.0.weight", "encoder_q.decoder.refine.2.weight",
                                             "encoder_q.proj_head.proj.0.weight", "encoder_q.proj_head.proj.2.weight"]),
}
SGD = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)


def ref_memory_model(cfg, encoder_name):
    """The reference's HRNet_W48_MEM (lib/models/nets/hrnet.py:153-188: encoder_q, then the two randn queues, L2-normalised,
    and their pointers, in that order) with `HRNet_W48_CONTRAST` resolved to another reference encoder while the constructor
    runs; forward keeps every head output of the encoder (the reference drops 'seg_aux', which its own memory criterion never
    reads) and adds key / lb_key exactly as :178-188."""
    import lib.models.nets.hrnet as ref_hrnet
    import lib.models.nets.deeplab as ref_deeplab
    encoder = {"deeplab_v3_contrast": ref_deeplab.DeepLabV3Contrast}[encoder_name]

    class RefMem(ref_hrnet.HRNet_W48_MEM):
        def forward(self, im_q, lb_q=None, with_embed=True, is_eval=False):
            if is_eval is True or lb_q is None:
                return self.encoder_q(im_q, with_embed=with_embed)
            ret = self.encoder_q(im_q)
            q = ret['embed']
            ret.update({'key': q.detach(), 'lb_key': lb_q.detach()})
            return ret

    saved = ref_hrnet.HRNet_W48_CONTRAST
    ref_hrnet.HRNet_W48_CONTRAST = encoder
    try:
        return RefMem(cfg, dim=cfg.get('contrast', 'proj_dim'))
    finally:
        ref_hrnet.HRNet_W48_CONTRAST = saved


def ref_model(cfg, name):
    from lib.models.model_manager import ModelManager
    if name == "deeplab_v3_mem":
        return ref_memory_model(cfg, "deeplab_v3_contrast")
    return ModelManager(cfg).semantic_segmentor()


def ref_criterion(cfg, name):
    from lib.loss.loss_manager import SEG_LOSS_DICT
    return ref_mem_auxce(cfg) if name == "mem_contrast_auxce_loss" else SEG_LOSS_DICT[name](cfg)


def watch_subset(a, cap=16384):
    """Every k-th element of the flattened tensor (<= cap values): keeps the golden files small."""
    flat = np.ascontiguousarray(a).reshape(-1)
    return flat[::max(1, flat.size // cap)].copy()


def step_inputs(c):
    rs = np.random.RandomState(c["seed"])
    img = rs.standard_normal((c["B"], 3, c["H"], c["W"])).astype(np.float32)
    if c.get("spread"):
        # per-image contrast / brightness (see model_input): keeps the B-sample BN of the ASPP image pooling conditioned
        gain = np.linspace(0.4, 1.6, c["B"]).astype(np.float32).reshape(-1, 1, 1, 1)
        bias = np.linspace(-0.8, 0.8, c["B"]).astype(np.float32).reshape(-1, 1, 1, 1)
        img = img * gain + bias * np.array([1.0, -0.5, 0.25], dtype=np.float32).reshape(1, 3, 1, 1)
    target, _, _ = O.synth_case(c["seed"] + 1, c["B"], c["K"], c["H"], c["W"], 4, 8, blocky=True, n_rect=10)
    return img, target


def run_step_case(name, c):
    import importlib
    import torch
    ref_shim.install()
    from lib.loss.loss_manager import SEG_LOSS_DICT
    from lib.models.model_manager import ModelManager
    cfg = ref_shim.configer(num_classes=c["K"], model_name=c["model"], backbone=c["backbone"],
                            loss_type=c["loss"] if c["loss"] in SEG_LOSS_DICT else "mem_contrast_ce_loss", contrast=c["contrast"])
    torch.manual_seed(304)
    net = ref_model(cfg, c["model"]).train()
    freeze_dropout(net)
    crit = ref_criterion(cfg, c["loss"])
    opt = torch.optim.SGD(net.parameters(), **SGD)
    img, target = step_inputs(c)
    img, target = torch.from_numpy(img).requires_grad_(True), torch.from_numpy(target)
    if c.get("bn_eval"):
        prime_bn(net, img)
        set_bn_eval(net)
    with_memory = "with_memory" in c["contrast"]
    if with_memory:
        for m in ("lib.vis.seg_visualizer", "lib.datasets.data_loader", "segmentor.tools.evaluator"):
            if m not in sys.modules:
                stub = types.ModuleType(m)
                stub.SegVisualizer = object
                stub.DataLoader = object
                stub.get_evaluator = lambda *a, **k: None
                sys.modules[m] = stub
        tc = importlib.import_module("segmentor.trainer_contrastive")
        me = types.SimpleNamespace(network_stride=c["network_stride"], memory_size=c["contrast"]["memory_size"],
                                   pixel_update_freq=c["contrast"]["pixel_update_freq"])
    named = dict(net.named_parameters())
    res = {}
    # the reference's OWN fp32 rounding noise on these gradients: the same model, input and anchor draws in fp64
    torch.manual_seed(304)
    net64 = ref_model(cfg, c["model"]).train()
    freeze_dropout(net64)
    if c.get("bn_eval"):
        net64.load_state_dict(net.state_dict())          # the SAME (fp32-primed) running statistics: the truth of the same function
        set_bn_eval(net64)
    net64, crit64 = net64.double(), ref_criterion(cfg, c["loss"]).double()
    torch.manual_seed(c["torch_seed"])
    img64 = img.detach().double().requires_grad_(True)
    if with_memory:
        out64 = net64(img64, target, with_embed=True)
        out64["pixel_queue"], out64["segment_queue"] = net64.pixel_queue, net64.segment_queue
    else:
        out64 = net64(img64, with_embed=True)
    loss64 = crit64(out64, target, with_embed=True)
    loss64.backward()
    grads64 = {w: dict(net64.named_parameters())[w].grad.numpy() for w in c["watch"]}
    grads64["input"] = img64.grad.numpy()
    for w in list(c["watch"]) + ["input"]:
        res["grad64/" + w] = watch_subset(grads64[w])          # fp64 ground truth of the same network
    res["loss0_fp64"] = np.array(float(loss64.detach()))
    del net64, crit64, out64
    torch.manual_seed(c["torch_seed"])
    for it in range(2):
        if with_memory:
            out = net(img, target, with_embed=True)
            out["pixel_queue"], out["pixel_queue_ptr"] = net.pixel_queue, net.pixel_queue_ptr
            out["segment_queue"], out["segment_queue_ptr"] = net.segment_queue, net.segment_queue_ptr
        else:
            out = net(img, with_embed=True)
        loss = crit(out, target, with_embed=True)
        res["loss%d" % it] = np.array(float(loss.detach()))
        if it == 1:
            break
        if with_memory:
            tc.Trainer._dequeue_and_enqueue(me, out["key"], out["lb_key"], segment_queue=net.segment_queue,
                                            segment_queue_ptr=net.segment_queue_ptr, pixel_queue=net.pixel_queue,
                                            pixel_queue_ptr=net.pixel_queue_ptr)
            res["segment_queue_after"] = net.segment_queue.numpy().copy()
            res["pixel_queue_after"] = net.pixel_queue.numpy().copy()
        opt.zero_grad()
        loss.backward()
        res["grad/input"] = watch_subset(img.grad.numpy())
        res["gradnoise/input"] = np.array(np.abs(img.grad.numpy() - grads64["input"]).max() / np.abs(grads64["input"]).max())
        res["gradnoise_l2/input"] = np.array(np.linalg.norm((img.grad.numpy() - grads64["input"]).ravel())
                                             / np.linalg.norm(grads64["input"].ravel()))
        for w in c["watch"]:
            res["grad/" + w] = watch_subset(named[w].grad.numpy())
            res["gradnorm/" + w] = np.array(np.sqrt((named[w].grad.numpy().astype(np.float64) ** 2).sum()))
            res["gradnoise/" + w] = np.array(np.abs(named[w].grad.numpy() - grads64[w]).max() / np.abs(grads64[w]).max())
            res["gradnoise_l2/" + w] = np.array(np.linalg.norm((named[w].grad.numpy() - grads64[w]).ravel())
                                                / np.linalg.norm(grads64[w].ravel()))
        before = {w: named[w].detach().numpy().copy() for w in c["watch"]}
        opt.step()
        for w in c["watch"]:
            res["delta/" + w] = watch_subset(named[w].detach().numpy() - before[w])      # the SGD update itself
    np.savez_compressed(os.path.join(OUT, "%s.npz" % name), **res)
    print("%s: loss %.6f (fp64 %.6f) -> %.6f ; |grad conv1|max %.3e; reference fp32-vs-fp64 gradient noise: %s" % (
        name, res["loss0"], res["loss0_fp64"], res["loss1"], np.abs(res["grad/" + c["watch"][0]]).max(),
        " ".join("%.1e" % float(res["gradnoise/" + w]) for w in ["input"] + list(c["watch"]))))


def run_running_score():
    """Confusion matrix + mean IoU of the reference's RunningScore (lib/metrics/running_score.py:120-215) on the seeded
    label maps of tests/test_running_score.py::_case."""
    ref_shim.install()
    from lib.metrics.running_score import RunningScore
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    from test_running_score import _case
    true, pred, K = _case()
    rs = RunningScore(None, num_classes=K, ignore_index=-1)
    rs.update(pred, true)
    np.savez_compressed(os.path.join(OUT, "running_score.npz"), confusion=rs.confusion_matrix.astype(np.int64),
                        mean_iou=np.array(rs.get_mean_iou()), pixel_acc=np.array(rs.get_pixel_acc()),
                        mean_acc=np.array(rs.get_mean_acc(), dtype=np.float64),
                        cls_iou=np.array(list(rs.get_cls_iou().values()), dtype=np.float64))
    print("running_score: mIoU %.6f acc %.6f" % (rs.get_mean_iou(), rs.get_pixel_acc()))


def run_state_dicts():
    """Per model of tests/test_models_vs_reference.py, the reference's state_dict under torch.manual_seed(304) as digests: number
    of entries, SHA-256 of the [key, shape, dtype] list in order, SHA-256 of all values in order (the checkpoint-interchange test
    of tests/test_host_surface.py reads the hrnet_w48_contrast layout digest)."""
    import json
    import torch
    ref_shim.install()
    from lib.models.model_manager import ModelManager as RefManager
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    from test_models_vs_reference import CASES, state_digests
    out = {}
    for model, backbone, contrast in CASES:
        torch.manual_seed(304)
        sd = RefManager(ref_shim.configer(model_name=model, backbone=backbone, contrast=contrast)).semantic_segmentor().state_dict()
        n, layout, values = state_digests(sd)
        out[model] = {"entries": n, "layout_sha256": layout, "values_sha256": values}
        print("state_dict %s: %d entries" % (model, n))
    with open(os.path.join(OUT, "ref_state_digests.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def run_aug_decisions():
    """The random decisions of the reference's own transform classes (lib/datasets/tools/cv2_aug_transforms.py, cv2 stubbed)
    under random.seed(1234) for the sizes of tests/test_gpu_aug_host.py: per sample and transform [name, skipped, arguments,
    output shape, first output value]."""
    import collections
    import collections.abc
    import importlib
    import json
    import random
    ref_shim.install()
    cv2 = sys.modules["cv2"]
    cv2.INTER_CUBIC, cv2.INTER_NEAREST = 2, 0
    cv2.resize = lambda x, size, interpolation=None: np.full((size[1], size[0]) + x.shape[2:], 128, dtype=x.dtype)
    cv2.flip = lambda x, code: x
    if not hasattr(collections, "Iterable"):
        collections.Iterable = collections.abc.Iterable      # the reference predates Python 3.10 (:519)
    aug = importlib.import_module("lib.datasets.tools.cv2_aug_transforms")
    from lib.utils.tools.configer import Configer as RefConfiger
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    from test_gpu_aug_host import AUG_SEED, AUG_SIZES, _configer

    def plain(v):
        if isinstance(v, (tuple, list)):
            return [plain(x) for x in v]
        if isinstance(v, (np.integer, np.bool_)):
            return v.item()
        return v
    log = []
    orig = aug._BaseTransform._process

    def spy(self, img, data_dict, skip, *args, **kw):
        out_img, out = orig(self, img, data_dict, skip, *args, **kw)
        log[-1].append([type(self).__name__, bool(skip), plain(list(args)), list(out_img.shape), int(out_img.reshape(-1)[0])])
        return out_img, out
    aug._BaseTransform._process = spy
    try:
        compose = aug.CV2AugCompose(_configer(RefConfiger), split="train")
        random.seed(AUG_SEED)
        for (w, h) in AUG_SIZES:
            log.append([])
            compose(np.full((h, w, 3), 128, np.uint8), labelmap=np.zeros((h, w), np.float32))
    finally:
        aug._BaseTransform._process = orig
    with open(os.path.join(OUT, "aug_decisions.json"), "w") as f:
        f.write('{"seed": %d, "sizes": %s, "log": [\n' % (AUG_SEED, json.dumps([list(s) for s in AUG_SIZES])))
        f.write(",\n".join(json.dumps(sample) for sample in log))          # one sample per line
        f.write("\n]}\n")
    print("aug_decisions: %d samples" % len(log))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    for name, c in LOSS_CASES.items():
        if a.only is None or a.only == name:
            run_loss_case(name, c)
    for name, c in ENQ_CASES.items():
        if a.only is None or a.only == name:
            run_enq_case(name, c)
    for name, c in MODEL_CASES.items():
        if a.only is None or a.only == name or a.only == "models":
            run_model_case(name, c)
    for name, c in STEP_CASES.items():
        if a.only is None or a.only == name or a.only == "steps":
            run_step_case(name, c)
    if a.only is None or a.only == "running_score":
        run_running_score()
    if a.only is None or a.only == "state_dicts":
        run_state_dicts()
    if a.only is None or a.only == "aug_decisions":
        run_aug_decisions()


if __name__ == "__main__":
    main()
