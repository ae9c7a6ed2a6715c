"""The test phase's kernels (csrc/ms_eval.hip: kernels.ms_fuse_argmax, kernels.confusion_update), segmentor/tester.py and the
CSEG_VAL_FUSED=1 validation pass.

Yardsticks: the reference's composition (segmentor/tester.py:310-327 ss_test, :380-398 ms_test) restated below with torch ops in
float64, and the same composition in fp32 with torch ops on the same device. R = the largest deviation of torch's own fp32
composition from the float64 one on a case; the kernel's largest deviation must be at most 2 R + 2^-20 sum|w_i| max|logit| (the
kernel rounds at other points than torch -- vertical blend first, one fused multiply-add per pixel -- but not more often; R itself
is dominated by the fp32 source coordinate). The prediction equals the float64 argmax wherever the float64 top-two margin exceeds
4 R, is one of the float64 top two elsewhere, and at most 1 % of a case's pixels may be in the second group. The confusion matrix
is compared with np.bincount under RunningScore._fast_hist's mask, exactly. The kernel is never compared with itself, except for
determinism. Replayed on the CPU emulation by tests/test_emu_ms_eval.py (the kernel-level tests; not the Tester / Trainer legs)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _compose(terms, H, W, dtype):
    """segmentor/tester.py:310-327 (ss_test: interpolate the net's output to the input size, bilinear, align_corners=True) and
    :380-398 (ms_test: probs = ss_test(x) + flip(ss_test(flip(x))), full_probs += weight * probs; without scale_weights
    full_probs += probs), on coarse maps that are given. terms: (plain, flipped or None, weight or None)."""
    B, K = terms[0][0].shape[:2]
    full = torch.zeros(B, K, H, W, dtype=dtype, device=terms[0][0].device)
    for a, b, w in terms:
        probs = F.interpolate(a.to(dtype), size=(H, W), mode="bilinear", align_corners=True)
        if b is not None:
            flip_probs = F.interpolate(b.to(dtype), size=(H, W), mode="bilinear", align_corners=True)
            probs = probs + torch.flip(flip_probs, dims=[3])
        if w is None:
            full += probs
        else:
            full += w * probs
    return full


_S4 = [(8, 16), (12, 24), (16, 32), (20, 40), (24, 48), (28, 56), (32, 64)]       # scale_search 0.5 ... 2.0 of 64 x 128 at stride 4
# name: (B, K, H, W), term sizes, paired, weights
CASES = {
    "odd5": ((2, 19, 37, 53), [(5, 7), (10, 14), (19, 27), (37, 53), (48, 70)], True, None),
    "odd5w": ((2, 19, 37, 53), [(5, 7), (10, 14), (19, 27), (37, 53), (48, 70)], True, [0.5, 0.75, 1.0, 1.25, 1.5]),
    "k171": ((1, 171, 33, 41), [(9, 11), (17, 21)], True, None),
    "wide300": ((1, 3, 17, 300), [(5, 75)], False, None),
    "row1": ((1, 2, 1, 9), [(1, 1), (3, 4)], True, None),
    "city7": ((2, 19, 64, 128), _S4, True, None),
}


def _inputs(name, dev):
    (B, K, H, W), sizes, paired, weights = CASES[name]
    g = torch.Generator().manual_seed(304)
    terms = []
    for i, (h, w) in enumerate(sizes):
        a = torch.randn(B, K, h, w, generator=g) * 4
        b = (torch.flip(a, dims=[3]) + 0.5 * torch.randn(B, K, h, w, generator=g)) if paired else None
        terms.append((a.to(dev), None if b is None else b.to(dev), None if weights is None else weights[i]))
    return terms, H, W


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Inputs and the two yardsticks of one case, computed once and shared (never modified)."""
    terms, H, W = _inputs(name, torch.device(dev_str))
    d64 = _compose(terms, H, W, torch.float64)
    d32 = _compose(terms, H, W, torch.float32)
    R = float((d32.double() - d64).abs().max())
    amax = max(float(t.abs().max()) for a, b, _ in terms for t in (a, b) if t is not None)
    wsum = sum(abs(1.0 if w is None else w) for _, _, w in terms)
    return terms, H, W, d64, R, amax, wsum


def _kernel_terms(terms):
    return [(a, b, 1.0 if w is None else w) for a, b, w in terms]


def _check_fused(tag, fused, d64, R, amax, wsum):
    err = float((fused.double() - d64).abs().max())
    bound = 2 * R + 2.0 ** -20 * wsum * amax
    print("%s: R (torch fp32 vs float64) %.3e  kernel vs float64 %.3e  bound %.3e  max|logit| %.2f" % (tag, R, err, bound, amax))
    assert err <= bound, (tag, err, bound, R)


def _check_pred(tag, pred, d64, R):
    top = d64.topk(2, dim=1)
    margin = top.values[:, 0] - top.values[:, 1]
    clear = margin > 4 * R
    pred = pred.long()
    first, second = top.indices[:, 0], top.indices[:, 1]
    share = 1.0 - float(clear.double().mean())
    print("%s: %.4f %% of the pixels within 4 R of a tie" % (tag, 100 * share))
    assert bool((pred[clear] == first[clear]).all()), tag
    assert bool(((pred == first) | (pred == second))[~clear].all()), tag
    assert share <= 0.01, (tag, share)


@pytest.mark.parametrize("case", list(CASES))
def test_fused_map_matches_the_float64_composition(case):
    from contrastiveseg_amd import kernels as K
    terms, H, W, d64, R, amax, wsum = _case(case, str(_dev()))
    pred, fused = K.ms_fuse_argmax(_kernel_terms(terms), H, W, want_fused=True)
    assert fused.shape == d64.shape and fused.dtype == torch.float32
    _check_fused(case, fused, d64, R, amax, wsum)
    only_fused = K.ms_fuse_argmax(_kernel_terms(terms), H, W, want_fused=True, want_pred=False)
    assert only_fused[0] is None and torch.equal(only_fused[1], fused)


@pytest.mark.parametrize("case", list(CASES))
def test_prediction_matches_the_float64_argmax(case):
    from contrastiveseg_amd import kernels as K
    terms, H, W, d64, R, amax, wsum = _case(case, str(_dev()))
    pred = K.ms_fuse_argmax(_kernel_terms(terms), H, W)
    assert pred.shape == (d64.shape[0], H, W) and pred.dtype == torch.uint8
    _check_pred(case, pred, d64, R)


def test_first_index_wins_among_equal_maxima():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W = _inputs("odd5w", dev)
    tied = []
    for a, b, w in terms:
        a, b = a.clone(), b.clone()
        a[:, 2] += 100.0
        b[:, 2] += 100.0
        a[:, 5] = a[:, 2]
        b[:, 5] = b[:, 2]
        tied.append((a, b, w))
    pred, fused = K.ms_fuse_argmax(tied, H, W, want_fused=True)
    assert torch.equal(fused[:, 2], fused[:, 5])
    assert bool((pred == 2).all())
    flat = [(torch.full((1, 7, 3, 5), 1.5, device=dev), torch.full((1, 7, 3, 5), 1.5, device=dev), 0.75),
            (torch.full((1, 7, 6, 4), -2.0, device=dev), None, 1.0)]
    assert bool((K.ms_fuse_argmax(flat, 9, 11) == 0).all())


def _hist(pred, target, K_, ignore):
    p, t = pred.cpu().numpy().astype(np.int64), target.cpu().numpy()
    mask = (t >= 0) & (t < K_) & (p < K_) & (t != ignore)
    return np.bincount(K_ * t[mask] + p[mask], minlength=K_ * K_).reshape(K_, K_), int(mask.sum())


# K = 19: histogram in LDS; 128 / 129: the last size on that path and the first on the global one; 171: global path
@pytest.mark.parametrize("K_,ignore", [(19, -1), (19, 3), (128, -1), (129, -1), (171, -1)])
def test_confusion_update_equals_bincount(K_, ignore):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(304 + K_)
    N = 5 * 4096 - 479                                 # several blocks, not a multiple of the block size
    # neighbouring pixels mostly agree (runs), with -1, 255 and K among the targets and predictions up to 255
    target = torch.randint(-1, K_ + 1, (N // 7 + 1,), generator=g).repeat_interleave(7)[:N].contiguous()
    target[torch.randint(0, N, (N // 50,), generator=g)] = 255
    target[torch.randint(0, N, (N // 50,), generator=g)] = -1
    target[torch.randint(0, N, (N // 50,), generator=g)] = K_
    pred = torch.where(torch.rand(N, generator=g) < 0.7, target.clamp(0, 255), torch.randint(0, 256, (N,), generator=g)).to(torch.uint8)
    pred, target = pred.to(dev), target.to(dev)
    want, n_valid = _hist(pred, target, K_, ignore)
    conf = torch.zeros(K_, K_, dtype=torch.int64, device=dev)
    out = K.confusion_update(pred, target, conf, ignore_index=ignore)
    assert out is conf
    assert np.array_equal(conf.cpu().numpy(), want)
    assert int(conf.sum()) == n_valid and 0 < n_valid < N
    # a second call adds into the same matrix; a short ragged call as well
    K.confusion_update(pred.reshape(-1, 1), target.reshape(-1, 1), conf, ignore_index=ignore)
    want_tail, _ = _hist(pred[:77], target[:77], K_, ignore)
    K.confusion_update(pred[:77], target[:77], conf, ignore_index=ignore)
    assert np.array_equal(conf.cpu().numpy(), 2 * want + want_tail)


def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W = _inputs("city7", dev)
    terms = _kernel_terms(terms)
    p1, f1 = K.ms_fuse_argmax(terms, H, W, want_fused=True)
    p2, f2 = K.ms_fuse_argmax(terms, H, W, want_fused=True)
    assert torch.equal(p1, p2) and torch.equal(f1, f2)
    target = torch.randint(-1, 19, (2, H, W), generator=torch.Generator().manual_seed(1)).to(dev)
    for K_ in (19, 171):
        c1 = K.confusion_update(p1, target, torch.zeros(K_, K_, dtype=torch.int64, device=dev))
        c2 = K.confusion_update(p1, target, torch.zeros(K_, K_, dtype=torch.int64, device=dev))
        assert torch.equal(c1, c2) and int(c1.sum()) == int((target >= 0).sum())


def test_refusals():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    a = torch.randn(1, 4, 3, 5, device=dev)
    with pytest.raises(RuntimeError, match="9 terms"):
        K.ms_fuse_argmax([(a, None, 1.0)] * 9, 6, 10)
    with pytest.raises(RuntimeError, match="257 classes"):
        K.ms_fuse_argmax([(torch.zeros(1, 257, 2, 2, device=dev), None, 1.0)], 4, 4)
    with pytest.raises(RuntimeError, match="both outputs"):
        K.ms_fuse_argmax([(a, None, 1.0)], 6, 10, want_fused=False, want_pred=False)
    with pytest.raises(RuntimeError, match="flipped map"):
        K.ms_fuse_argmax([(a, torch.randn(1, 4, 3, 6, device=dev), 1.0)], 6, 10)
    with pytest.raises(RuntimeError, match="empty"):
        K.ms_fuse_argmax([(a, None, 1.0)], 0, 10)
    conf = torch.zeros(4, 4, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="predictions"):
        K.confusion_update(torch.zeros(5, dtype=torch.uint8, device=dev), torch.zeros(6, dtype=torch.int64, device=dev), conf)
    with pytest.raises(RuntimeError, match="must be"):
        K.confusion_update(torch.zeros(5, dtype=torch.int64, device=dev), torch.zeros(5, dtype=torch.int64, device=dev), conf)
    assert int(conf.sum()) == 0
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            K.ms_fuse_argmax([(a.cpu(), None, 1.0)], 6, 10)
        with pytest.raises(RuntimeError, match="GPU"):
            K.confusion_update(torch.zeros(5, dtype=torch.uint8), torch.zeros(5, dtype=torch.int64, device=dev), conf)


def test_nothing_of_the_size_of_the_fused_map_is_allocated():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W = _inputs("city7", dev)
    terms = _kernel_terms(terms)
    B, K_ = terms[0][0].shape[:2]
    if dev.type != "cuda":
        assert K.ms_fuse_argmax(terms, H, W).numel() == B * H * W
        return
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    pred = K.ms_fuse_argmax(terms, H, W)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("peak growth %d bytes; the fused map would be %d" % (growth, B * K_ * H * W * 4))
    assert pred.numel() == B * H * W and growth < B * K_ * H * W * 4


# ---- Tester orchestration, end to end, CSEG_VAL_FUSED ------------------------------------------------------------------------------------
def _tiny_cfg(**test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def _restate(net, inputs, scales, weights, flip, dtype):
    """Tester.ss_test / ms_test of the reference (:310-327, :380-398) driven with the same model object; the model runs in fp32,
    everything after it in `dtype`."""
    n, c, h, w = inputs.shape

    def ss_test(x, scale):
        scaled = F.interpolate(x, size=(int(h * scale), int(w * scale)), mode="bilinear", align_corners=True)
        out = net(scaled, is_eval=True)["seg"]
        return F.interpolate(out.to(dtype), size=(h, w), mode="bilinear", align_corners=True), float(out.abs().max())

    full, amax = None, 0.0
    for i, scale in enumerate(scales):
        probs, m = ss_test(inputs, scale)
        amax = max(amax, m)
        if flip:
            flip_probs, m = ss_test(torch.flip(inputs, dims=[3]), scale)
            amax = max(amax, m)
            probs = probs + torch.flip(flip_probs, dims=[3])
        if full is None:
            full = torch.zeros_like(probs)
        full += probs if weights is None else weights[i] * probs
    return full, amax


class _Memo(torch.nn.Module):
    """The model with its evaluation outputs remembered per input. Two forward passes of this network on the same input differ in
    the last bits on the GPU (measured on the MI355X with this configuration: up to 9e-6 at |logit| < 5 between any two of five
    calls, in eval mode, with or without a warm-up call), which says nothing about the Tester: where a test compares two routes
    through the Tester bit for bit, or counts pixels that may change class, both routes get the same coarse maps."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x, **kw):
        for x0, out in self.seen:
            if x0.shape == x.shape and torch.equal(x0, x):
                return out
        out = self.net(x, **kw)
        self.seen.append((x.clone(), out))
        return out


@pytest.mark.parametrize("weights", [None, [0.5, 1, 2]])
def test_tester_ms_test_matches_the_restatement(weights):
    from contrastiveseg_amd.segmentor.tester import Tester
    dev = _dev()
    scales = [0.5, 1.0, 1.5]
    keys = dict(mode="ms_test", scale_search=scales)
    if weights is not None:
        keys["scale_weights"] = weights
    torch.manual_seed(304)
    tester = Tester(_tiny_cfg(**keys))
    tester.seg_net = _Memo(tester.seg_net)
    inputs = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(304)).to(dev)
    with torch.no_grad():
        pred, fused = tester.ms_test(inputs, want_fused=True)
        d64, amax = _restate(tester.seg_net, inputs, scales, weights, True, torch.float64)
        d32, _ = _restate(tester.seg_net, inputs, scales, weights, True, torch.float32)
    R = float((d32.double() - d64).abs().max())
    wsum = float(sum(weights)) if weights is not None else float(len(scales))
    tag = "tester ms_test weights=%s" % (weights,)
    _check_fused(tag, fused, d64, R, amax, wsum)
    _check_pred(tag, pred, d64, R)
    assert torch.equal(tester.ms_test(inputs), pred)


def test_tester_ss_test_is_ms_test_with_one_scale_and_no_flip():
    from contrastiveseg_amd.segmentor.tester import Tester
    dev = _dev()
    torch.manual_seed(304)
    one = Tester(_tiny_cfg(mode="ms_test", scale_search=[1.0]))
    one.seg_net = _Memo(one.seg_net)
    inputs = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(304)).to(dev)
    with torch.no_grad():
        p_ms, f_ms = one.ms_test(inputs, want_fused=True, flip=False)
        p_ss, f_ss = one.ss_test(inputs, want_fused=True)
        d64, amax = _restate(one.seg_net, inputs, [1], None, False, torch.float64)
        d32, _ = _restate(one.seg_net, inputs, [1], None, False, torch.float32)
    assert torch.equal(p_ms, p_ss) and torch.equal(f_ms, f_ss)
    R = float((d32.double() - d64).abs().max())
    _check_fused("tester ss_test", f_ss, d64, R, amax, 1.0)
    _check_pred("tester ss_test", p_ss, d64, R)


def test_phase_test_end_to_end(tmp_path):
    from PIL import Image
    from contrastiveseg_amd import main_contrastive
    from contrastiveseg_amd.lib.metrics.running_score import RunningScore
    ids = [3, 7, 9, 11, 20]
    rs = np.random.RandomState(304)
    img_dir, lab_dir, out_dir = tmp_path / "val" / "image", tmp_path / "val" / "label", tmp_path / "out"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir()
    labels = {}
    for stem in ("frankfurt_000000", "munster_000001"):
        Image.fromarray(rs.randint(0, 256, size=(64, 96, 3)).astype(np.uint8)).save(str(img_dir / (stem + ".png")))
        lab = np.full((64, 96), 255, np.uint8)
        for _ in range(10):
            y0, x0 = rs.randint(0, 64), rs.randint(0, 96)
            lab[y0:y0 + 24, x0:x0 + 32] = ids[rs.randint(0, len(ids))]
        Image.fromarray(lab).save(str(lab_dir / (stem + ".png")))
        labels[stem] = lab
    log = str(tmp_path / "test.log")
    miou = main_contrastive.main(
        ["--configs", os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"), "--phase", "test", "--test_dir", str(img_dir),
         "--out_dir", str(out_dir), "--log_file", log, "--stdout_level", "error", "network.pretrained", "None", "network.resume", "None",
         "data.label_list", str(ids), "test.mode", "ms_test", "test.scale_search", "[0.5, 1.0]", "test.batch_size", "2",
         "test.data_transformer", "{'size_mode': 'fix_size', 'input_size': [96, 64], 'align_method': 'only_pad'}"])
    score = RunningScore(num_classes=5, ignore_index=-1)
    lut = np.full(256, -1, np.int64)
    lut[ids] = np.arange(5)
    for stem, lab in labels.items():
        png = np.asarray(Image.open(str(out_dir / "label" / (stem + ".png"))))
        assert png.shape == (64, 96) and png.dtype == np.uint8 and set(np.unique(png)) <= set(ids)
        score.update(torch.from_numpy(lut[png]), torch.from_numpy(lut[lab]))
    assert sorted(os.listdir(str(out_dir / "label"))) == ["frankfurt_000000.png", "munster_000001.png"]
    want = float(score.get_mean_iou())
    assert int(score.confusion_matrix.sum()) == sum(int((lab != 255).sum()) for lab in labels.values())
    assert miou == want, (miou, want)
    assert "Test mIoU {:.6f}".format(want) in open(log).read()


def test_val_fused_switch_gives_the_same_confusion_matrix(monkeypatch, tmp_path):
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    dev = _dev()
    cfg = _tiny_cfg()
    cfg.get("train", "data_transformer")["input_size"] = [96, 64]
    cfg.update(["train", "batch_size"], 2)
    cfg.update(["contrast", "max_views"], 1)
    cfg.update(["checkpoints", "checkpoints_dir"], str(tmp_path))
    cfg.get("checkpoints")["checkpoints_root"] = None
    cfg.add(["project_dir"], str(tmp_path))
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    batches = list(SyntheticLoader(cfg, dev, length=2, mode="blocky", fixed=False))
    tr.seg_net = _Memo(tr.seg_net)
    monkeypatch.delenv("CSEG_VAL_FUSED", raising=False)
    tr.validate(batches)
    default = tr.last_val_score.confusion_matrix.clone()
    monkeypatch.setenv("CSEG_VAL_FUSED", "1")
    tr.validate(batches)
    fused = tr.last_val_score.confusion_matrix.clone()
    # pixels under the near-tie rule, from the model's own coarse maps
    tr.seg_net.eval()
    n_tie = n_pix = 0
    with torch.no_grad():
        for b in batches:
            seg = tr.seg_net(b["img"], is_eval=True)["seg"]
            size = b["labelmap"].shape[-2:]
            d64 = F.interpolate(seg.double(), size=size, mode="bilinear", align_corners=True)
            d32 = F.interpolate(seg, size=size, mode="bilinear", align_corners=True)
            R = float((d32.double() - d64).abs().max())
            top = d64.topk(2, dim=1).values
            n_tie += int(((top[:, 0] - top[:, 1]) <= 4 * R).sum())
            n_pix += top[:, 0].numel()
    tr.seg_net.train()
    moved = int((default - fused).abs().sum()) // 2
    print("pixels counted elsewhere: %d, within 4 R of a tie: %d of %d" % (moved, n_tie, n_pix))
    assert int(default.sum()) == int(fused.sum()) > 0
    assert torch.equal(default.sum(1), fused.sum(1))            # rows are ground truth: the mask is the same
    assert moved <= n_tie and n_tie <= 0.01 * n_pix
