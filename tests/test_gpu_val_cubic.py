"""Validation on the reference's resize: kernels.cubic_argmax (csrc/cubic_eval.hip), score_cubic and the val.score_resize switch of
segmentor/trainer_contrastive.py, the 'ori_labelmap' / 'border_size' keys of the val loader.

The rule the kernel implements is cv2's float INTER_CUBIC as its scalar source states it (resize.cpp: the xofs / alpha table loop,
interpolateCubic, HResizeCubic, VResizeCubic); _restate below spells it with numpy float32 arrays, one rounding per operation, and
the kernel's fused map must equal it bit for bit, on both launch paths. The restatement in turn -- through the kernel, which carries
its bits -- is held against float64: d64 = F.interpolate(x.double(), mode='bicubic', align_corners=False) on the cropped map
(mathematically the same rule: A = -0.75, replicated border, unclamped source coordinate), R = the largest deviation of torch's own
fp32 bicubic from d64 on the same device, and the checks of tests/test_gpu_ms_eval.py with wsum = 2, which bounds the cubic gain
(sum|c|)^2 <= 1.375^2: error <= 2 R + 2^-20 * 2 * max|logit|, the prediction exact where the float64 margin exceeds 4 R, one of the
top two elsewhere, at most 1 % of a case's pixels there. Bit parity with a cv2 binary is not pinned. The kernel-level tests
are replayed on the CPU emulation by tests/test_emu_val_cubic.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ms_eval import _Memo, _check_fused, _check_pred, _tiny_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIP_PERM = list(range(14)) + [15, 14, 17, 16, 19, 18]


def _dev():
    return torch.device("cuda:0")


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------
def _coeffs(t):
    """interpolateCubic, A = -0.75f, every product and sum rounded on its own (t: float32 array)."""
    f = np.float32
    A = f(-0.75)
    x1 = t + f(1)
    c0 = ((A * x1 - f(5) * A) * x1 + f(8) * A) * x1 - f(4) * A
    c1 = ((A + f(2)) * t - (A + f(3))) * t * t + f(1)
    u = f(1) - t
    c2 = ((A + f(2)) * u - (A + f(3))) * u * u + f(1)
    c3 = f(1) - c0 - c1 - c2
    return [c.astype(np.float32) for c in (c0, c1, c2, c3)]


def _axis(n_dst, n_crop):
    """-> tap indices [4][n_dst] (clamped to the crop) and coefficients [4][n_dst] of one axis."""
    scale = 1.0 / (float(n_dst) / float(n_crop))
    x = np.arange(n_dst, dtype=np.float64)
    fx = ((x + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx)
    t = (fx - sx).astype(np.float32)
    sx = sx.astype(np.int64)
    return [np.clip(sx - 1 + j, 0, n_crop - 1) for j in range(4)], _coeffs(t)


def _source(a, flipped=None, perm=None):
    """What the resize reads: a, or the coarse-size average with the mirrored operand (over the map's full width)."""
    if flipped is None:
        return a
    bm = flipped if perm is None else flipped[:, list(perm)]
    return ((a + bm[:, :, :, ::-1]) / np.float32(2)).astype(np.float32)


def _restate(a, H, W, crop=None, flipped=None, perm=None):
    """a, flipped: float32 numpy [B,K,h,w] -> float32 [B,K,H,W], horizontal pass first, then vertical, left to right."""
    s = _source(a, flipped, perm)
    ch, cw = crop if crop is not None else s.shape[2:]
    s = s[:, :, :ch, :cw]
    (x0, x1, x2, x3), (c0, c1, c2, c3) = _axis(W, cw)
    (y0, y1, y2, y3), (d0, d1, d2, d3) = _axis(H, ch)
    hz = ((s[..., x0] * c0 + s[..., x1] * c1) + s[..., x2] * c2) + s[..., x3] * c3
    assert hz.dtype == np.float32
    d0, d1, d2, d3 = (d[:, None] for d in (d0, d1, d2, d3))
    v = ((hz[:, :, y0] * d0 + hz[:, :, y1] * d1) + hz[:, :, y2] * d2) + hz[:, :, y3] * d3
    assert v.dtype == np.float32
    return v


# name: (B, K, h, w), crop or None, (H, W)
CASES = {
    "up4": ((2, 19, 16, 32), None, (64, 128)),
    "odd": ((1, 19, 9, 13), None, (37, 53)),
    "s8": ((1, 19, 17, 33), None, (129, 257)),
    "wide300": ((1, 3, 5, 75), None, (17, 300)),
    "k171": ((1, 171, 9, 11), None, (33, 41)),
    "k256": ((1, 256, 3, 4), None, (10, 14)),
    "row1": ((1, 2, 1, 1), None, (1, 9)),
    "h1": ((1, 3, 1, 5), None, (4, 20)),
    "down": ((1, 5, 20, 24), None, (7, 9)),
    "crop": ((1, 19, 12, 20), (10, 17), (40, 68)),
}


def _tiled_ok(name):
    (B, K, h, w), crop, (H, W) = CASES[name]
    ch, cw = crop if crop is not None else (h, w)
    return H >= 2 * ch and W >= 2 * cw


def _paths(name):
    return (0, 1, 2) if _tiled_ok(name) else (0, 1)


def _input(name):
    shape, crop, size = CASES[name]
    return torch.randn(*shape, generator=torch.Generator().manual_seed(304)) * 4, crop, size


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Input, restatement and the float64 yardstick of one case, computed once and shared (never modified)."""
    x, crop, (H, W) = _input(name)
    want = torch.from_numpy(_restate(x.numpy(), H, W, crop))
    x = x.to(torch.device(dev_str))
    cropped = x if crop is None else x[:, :, :crop[0], :crop[1]]
    d64 = F.interpolate(cropped.double(), size=(H, W), mode="bicubic", align_corners=False)
    d32 = F.interpolate(cropped, size=(H, W), mode="bicubic", align_corners=False)
    R = float((d32.double() - d64).abs().max())
    return x, crop, H, W, want, d64, R, float(x.abs().max())


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_both_sides_of_the_tiled_rule():
    assert [n for n in CASES if not _tiled_ok(n)] == ["row1", "down"]


@pytest.mark.parametrize("case", list(CASES))
def test_fused_map_equals_the_restatement_bit_for_bit_on_every_path(case):
    from contrastiveseg_amd import kernels as K
    x, crop, H, W, want, d64, R, amax = _case(case, str(_dev()))
    preds = []
    for path in _paths(case):
        pred, fused = K.cubic_argmax(x, H, W, crop=crop, want_fused=True, path=path)
        assert fused.shape == want.shape and fused.dtype == torch.float32
        diff = int((fused.cpu() != want).sum())
        print("%s path %d: %d of %d values differ from the restatement" % (case, path, diff, want.numel()))
        assert torch.equal(fused.cpu(), want), (case, path, diff)
        assert pred.shape == (x.shape[0], H, W) and pred.dtype == torch.uint8
        assert np.array_equal(pred.cpu().numpy(), np.argmax(want.numpy(), 1)), (case, path)       # np.argmax: the first maximum
        preds.append(pred)
    assert all(torch.equal(p, preds[0]) for p in preds)


@pytest.mark.parametrize("case", list(CASES))
def test_fused_map_and_prediction_match_float64(case):
    from contrastiveseg_amd import kernels as K
    x, crop, H, W, want, d64, R, amax = _case(case, str(_dev()))
    for path in _paths(case):
        pred, fused = K.cubic_argmax(x, H, W, crop=crop, want_fused=True, path=path)
        tag = "%s path %d" % (case, path)
        _check_fused(tag, fused, d64, R, amax, 2.0)
        _check_pred(tag, pred, d64, R)


def test_cubic_differs_from_bilinear():
    from contrastiveseg_amd import kernels as K
    x, crop, H, W, want, d64, R, amax = _case("up4", str(_dev()))
    cubic = K.cubic_argmax(x, H, W)
    bilinear = K.ms_fuse_argmax([(x, None, 1.0)], H, W)
    share = float((cubic != bilinear).double().mean())
    print("cubic vs bilinear argmax on noise logits at 4x: %.1f %% of the pixels differ" % (100 * share))
    assert share > 0.10


@pytest.mark.parametrize("K_,crop", [(20, None), (19, None), (20, (10, 17)), (19, (12, 9))])
def test_mirrored_operand_equals_averaging_first(K_, crop):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.segmentor.trainer_contrastive import lip_mirror_perm
    dev = _dev()
    g = torch.Generator().manual_seed(304)
    a = (torch.randn(2, K_, 12, 20, generator=g) * 4).to(dev)
    b = (torch.randn(2, K_, 12, 20, generator=g) * 4).to(dev)
    perm = lip_mirror_perm(K_)
    assert (perm == LIP_PERM) if K_ == 20 else (perm is None)
    gathered = b if perm is None else b.index_select(1, torch.tensor(perm, device=dev))
    averaged = (a + torch.flip(gathered, [3])) / 2.
    want = torch.from_numpy(_restate(a.cpu().numpy(), 40, 68, crop, b.cpu().numpy(), perm))
    for path in (0, 1, 2):
        p0, f0 = K.cubic_argmax(averaged, 40, 68, crop=crop, want_fused=True, path=path)
        p1, f1 = K.cubic_argmax(a, 40, 68, crop=crop, flipped=b, perm=perm, want_fused=True, path=path)
        assert torch.equal(f0, f1) and torch.equal(p0, p1), (K_, crop, path)
        assert torch.equal(f1.cpu(), want), (K_, crop, path)
    if perm is not None:                  # the permutation does something: without it the map differs
        assert not torch.equal(K.cubic_argmax(a, 40, 68, crop=crop, flipped=b, want_fused=True)[1], f1)
    if crop is not None:                  # the mirror is over the full width: mirroring the cropped operand is another map
        cw = crop[1]
        narrow = (a[..., :cw] + torch.flip(gathered[..., :cw], [3])) / 2.
        assert not torch.equal(K.cubic_argmax(narrow.contiguous(), 40, 68, crop=(crop[0], cw), want_fused=True)[1], f1)


def test_first_index_wins_among_equal_maxima():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    x, crop, (H, W) = _input("up4")
    x = x.clone()
    x[:, 2] += 100.0
    x[:, 5] = x[:, 2]
    x = x.to(dev)
    for path in (1, 2):
        pred, fused = K.cubic_argmax(x, H, W, want_fused=True, path=path)
        assert torch.equal(fused[:, 2], fused[:, 5])
        assert bool((pred == 2).all())
        assert bool((K.cubic_argmax(torch.full((1, 7, 3, 5), 1.5, device=dev), 9, 11, path=path) == 0).all())


def test_pred_alone_and_fused_alone():
    from contrastiveseg_amd import kernels as K
    x, crop, H, W, want, d64, R, amax = _case("odd", str(_dev()))
    for path in (1, 2):
        pred, fused = K.cubic_argmax(x, H, W, want_fused=True, path=path)
        assert torch.equal(K.cubic_argmax(x, H, W, path=path), pred)
        only = K.cubic_argmax(x, H, W, want_fused=True, want_pred=False, path=path)
        assert only[0] is None and torch.equal(only[1], fused)


def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    x, crop, H, W, want, d64, R, amax = _case("up4", str(_dev()))
    for path in (1, 2):
        p1, f1 = K.cubic_argmax(x, H, W, want_fused=True, path=path)
        p2, f2 = K.cubic_argmax(x, H, W, want_fused=True, path=path)
        assert torch.equal(p1, p2) and torch.equal(f1, f2)


def test_refusals():
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    a = torch.randn(1, 4, 3, 5, device=dev)
    # the library's (item 2), by message
    with pytest.raises(RuntimeError, match="K = 257"):
        K.cubic_argmax(torch.zeros(1, 257, 2, 2, device=dev), 4, 4)
    with pytest.raises(RuntimeError, match="K = 0"):
        K.cubic_argmax(torch.zeros(1, 0, 2, 2, device=dev), 4, 4)
    for crop in ((4, 5), (3, 6), (0, 5), (3, 0)):
        with pytest.raises(RuntimeError, match=r"crop \(ch, cw\) = \(%d, %d\) is outside the 3 x 5 map" % crop):
            K.cubic_argmax(a, 6, 10, crop=crop)
    with pytest.raises(RuntimeError, match="both outputs"):
        K.cubic_argmax(a, 6, 10, want_fused=False, want_pred=False)
    with pytest.raises(RuntimeError, match="path = 2"):
        K.cubic_argmax(a, 5, 10, path=2)                   # 3 -> 5 rows is less than a factor of 2
    with pytest.raises(RuntimeError, match="path = 2"):
        K.cubic_argmax(torch.randn(1, 5, 20, 24, device=dev), 7, 9, path=2)     # the case "down"
    with pytest.raises(RuntimeError, match="path = 3"):
        K.cubic_argmax(a, 6, 10, path=3)
    with pytest.raises(RuntimeError, match="path = -1"):
        K.cubic_argmax(a, 6, 10, path=-1)
    with pytest.raises(RuntimeError, match="empty"):
        K.cubic_argmax(a, 0, 10)
    with pytest.raises(RuntimeError, match=r"perm\[1\] = 0 repeats"):
        K.cubic_argmax(a, 6, 10, flipped=a, perm=[0, 0, 2, 3])
    with pytest.raises(RuntimeError, match=r"perm\[2\] = 4 is not a class"):
        K.cubic_argmax(a, 6, 10, flipped=a, perm=[0, 1, 4, 3])
    # perm without b reaches the library only past the wrapper: through the binding
    pred = torch.zeros(1, 6, 10, dtype=torch.uint8, device=dev)
    table = (ctypes.c_ubyte * 4)(0, 1, 2, 3)
    with pytest.raises(RuntimeError, match="perm was given without b"):
        _hip.call("cseg_cubic_argmax", _hip.dev(a, torch.float32, "a"), None, table, 1, 4, 3, 5, 3, 5, 6, 10, 0,
                  _hip.dev(pred, torch.uint8, "pred"), None, _hip.stream_ptr())
    assert int(pred.sum()) == 0                            # nothing was launched
    # the wrapper's (item 3), each naming the argument
    with pytest.raises(RuntimeError, match="seg is"):
        K.cubic_argmax(a[0], 6, 10)
    with pytest.raises(RuntimeError, match="flipped is"):
        K.cubic_argmax(a, 6, 10, flipped=torch.randn(1, 4, 3, 6, device=dev))
    with pytest.raises(RuntimeError, match="perm was given without flipped"):
        K.cubic_argmax(a, 6, 10, perm=[0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="perm has 3 entries"):
        K.cubic_argmax(a, 6, 10, flipped=a, perm=[0, 1, 2])
    with pytest.raises(RuntimeError, match="crop is"):
        K.cubic_argmax(a, 6, 10, crop=(3,))
    with pytest.raises(RuntimeError, match="must be"):
        K.cubic_argmax(a.double(), 6, 10)
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            K.cubic_argmax(a.cpu(), 6, 10)
    # a non-contiguous view is made contiguous, as in ms_fuse_argmax
    wide = torch.randn(1, 4, 3, 10, device=dev)
    assert torch.equal(K.cubic_argmax(wide[..., ::2], 6, 10), K.cubic_argmax(wide[..., ::2].contiguous(), 6, 10))


# ---- score_cubic ---------------------------------------------------------------------------------------------------------------------------
def _clear_counts(d64, d32, targets, K_):
    """Confusion matrix of the float64 argmax over the pixels whose float64 margin exceeds 4 R, and the targets with every other pixel
    set to the ignore label (the tie handling of tests/test_gpu_lip_swap.py): d64, d32 [1,K,H,W], targets [H,W]."""
    R = float((d32.double() - d64).abs().max())
    top = d64.topk(2, dim=1)
    clear = ((top.values[:, 0] - top.values[:, 1]) > 4 * R)[0]
    assert float(clear.double().mean()) >= 0.99
    kept = torch.where(clear, targets, torch.full_like(targets, -1))
    t, p = kept.cpu().numpy().reshape(-1), top.indices[0, 0].cpu().numpy().reshape(-1)
    return np.bincount(K_ * t[t >= 0] + p[t >= 0], minlength=K_ * K_).reshape(K_, K_), kept


def _bicubic(x, size, dtype):
    return F.interpolate(x.to(dtype), size=size, mode="bicubic", align_corners=False)


@pytest.mark.parametrize("borders,crops", [(None, [(12, 20), (12, 20)]), ([(80, 48), (160, 96)], [(12, 20), (12, 20)]),
                                           ([(17, 10), (20, 7)], [(10, 17), (7, 20)])],
                         ids=["no-borders", "borders-beyond-the-map", "borders-inside-the-map"])
def test_score_cubic_counts_what_float64_predicts(borders, crops):
    """List targets of two sizes, image by image; a border beyond the coarse map crops nothing, one inside it crops."""
    from contrastiveseg_amd.segmentor.trainer_contrastive import score_cubic
    dev = _dev()
    K_ = 7
    g = torch.Generator().manual_seed(304)
    seg = (torch.randn(2, K_, 12, 20, generator=g) * 4).to(dev)
    targets = [torch.randint(-1, K_, size, generator=g).to(dev) for size in ((45, 61), (40, 68))]
    want, kept = np.zeros((K_, K_), np.int64), []
    for i, (ch, cw) in enumerate(crops):
        x = seg[i:i + 1, :, :ch, :cw]
        w_i, k_i = _clear_counts(_bicubic(x, targets[i].shape, torch.float64), _bicubic(x, targets[i].shape, torch.float32),
                                 targets[i], K_)
        want += w_i
        kept.append(k_i)
    hist = torch.zeros(K_, K_, dtype=torch.int64, device=dev)
    assert score_cubic(seg, kept, hist, borders=borders) is hist
    assert int(want.sum()) == sum(int((k >= 0).sum()) for k in kept) > 0
    assert np.array_equal(hist.cpu().numpy(), want)


def test_score_cubic_on_a_tensor_of_targets_and_a_mirrored_pair():
    from contrastiveseg_amd.segmentor.trainer_contrastive import lip_mirror_perm, score_cubic
    dev = _dev()
    K_ = 20
    g = torch.Generator().manual_seed(304)
    seg = (torch.randn(4, K_, 12, 12, generator=g) * 4).to(dev)
    targets = torch.randint(-1, K_, (2, 45, 45), generator=g).to(dev)
    avg = (seg[:2] + torch.flip(seg[2:].index_select(1, torch.tensor(LIP_PERM, device=dev)), [3])) / 2.
    want, kept = np.zeros((K_, K_), np.int64), []
    for i in range(2):
        w_i, k_i = _clear_counts(_bicubic(avg[i:i + 1], (45, 45), torch.float64), _bicubic(avg[i:i + 1], (45, 45), torch.float32),
                                 targets[i], K_)
        want += w_i
        kept.append(k_i)
    hist = torch.zeros(K_, K_, dtype=torch.int64, device=dev)
    score_cubic(seg[:2], torch.stack(kept), hist, flipped=seg[2:], perm=lip_mirror_perm(K_))
    assert np.array_equal(hist.cpu().numpy(), want) and int(want.sum()) > 0
    with pytest.raises(ValueError, match="3 targets"):
        score_cubic(seg[:2], kept + kept[:1], hist)
    with pytest.raises(ValueError, match="1 borders"):
        score_cubic(seg[:2], kept, hist, borders=[(4, 4)])


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, **val_keys):
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    cfg = _tiny_cfg()
    cfg.get("train", "data_transformer")["input_size"] = [96, 64]
    cfg.update(["train", "batch_size"], 2)
    cfg.update(["contrast", "max_views"], 1)
    cfg.update(["checkpoints", "checkpoints_dir"], str(tmp_path))
    cfg.get("checkpoints")["checkpoints_root"] = None
    cfg.add(["project_dir"], str(tmp_path))
    for k, v in val_keys.items():
        cfg.add(["val", k], v)
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    tr.seg_net = _Memo(tr.seg_net)
    return tr, cfg


def _coarse(tr, batch):
    """The coarse maps validate() saw for this batch (the _Memo returns them again, bit for bit)."""
    tr.seg_net.eval()
    with torch.no_grad():
        seg = tr.seg_net(batch["img"], is_eval=True)["seg"]
    tr.seg_net.train()
    return seg


def test_trainer_cubic_scores_through_score_cubic(tmp_path):
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import score_cubic
    dev = _dev()
    tr, cfg = _trainer(tmp_path, score_resize="cubic")
    assert tr.score_resize == "cubic"
    batches = list(SyntheticLoader(cfg, dev, length=2, mode="blocky", fixed=False))
    losses = []
    hook = tr.pixel_loss.register_forward_hook(lambda module, args, out: losses.append(float(out)))
    tr.validate(batches)
    hook.remove()
    got = tr.last_val_score.confusion_matrix.clone()
    n = got.shape[0]
    want = torch.zeros(n, n, dtype=torch.int64, device=dev)
    for b in batches:
        score_cubic(_coarse(tr, b), b["labelmap"], want)
    assert torch.equal(got.to(dev), want) and int(want.sum()) == sum(int((b["labelmap"] >= 0).sum()) for b in batches) > 0
    # the validation loss is computed as before: once per batch, averaged into val_loss (whatever this untrained model's loss is)
    assert len(losses) == 2 and np.isclose(cfg.get("val_loss"), np.mean(losses), rtol=1e-6, equal_nan=True)

    # a batch carrying the label files at another size is scored against them, with the borders the loader recorded
    g = torch.Generator().manual_seed(5)
    ori = [torch.randint(-1, n, size, generator=g).to(dev) for size in ((50, 70), (33, 91))]
    with_ori = dict(batches[0], ori_labelmap=ori, border_size=[(96, 64), (96, 64)])
    tr.validate([with_ori])
    got = tr.last_val_score.confusion_matrix.clone()
    want = torch.zeros(n, n, dtype=torch.int64, device=dev)
    score_cubic(_coarse(tr, batches[0]), ori, want, borders=[(96, 64), (96, 64)])
    assert torch.equal(got.to(dev), want) and int(want.sum()) == sum(int((t >= 0).sum()) for t in ori)


def test_trainer_without_the_key_runs_the_bilinear_pass(tmp_path, monkeypatch):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    dev = _dev()
    tr, cfg = _trainer(tmp_path)
    assert tr.score_resize == "bilinear"

    def boom(*a, **k):
        raise AssertionError("the bilinear pass called kernels.cubic_argmax")
    monkeypatch.setattr(K, "cubic_argmax", boom)
    batches = list(SyntheticLoader(cfg, dev, length=2, mode="blocky", fixed=False))
    tr.validate(batches)
    got = tr.last_val_score.confusion_matrix.cpu()
    n = got.shape[0]
    want = torch.zeros(n, n, dtype=torch.int64)
    for b in batches:
        pred = F.interpolate(_coarse(tr, b), size=b["labelmap"].shape[-2:], mode="bilinear", align_corners=True).argmax(1).cpu()
        t = b["labelmap"].cpu()
        want += torch.bincount(n * t[t >= 0] + pred[t >= 0], minlength=n * n).reshape(n, n)
    assert torch.equal(got, want) and int(want.sum()) > 0


# ---- the loader ----------------------------------------------------------------------------------------------------------------------------
def test_val_loader_yields_the_label_files_at_their_own_size(tmp_path):
    from PIL import Image
    from contrastiveseg_amd.lib.datasets.data_loader import DataLoader
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    dev = _dev()
    ids = [3, 7, 9, 11, 20]
    rs = np.random.RandomState(304)
    sizes = [(40, 56), (64, 48), (40, 56)]
    raw = []
    (tmp_path / "val" / "image").mkdir(parents=True)
    (tmp_path / "val" / "label").mkdir()
    for i, (h, w) in enumerate(sizes):
        lab = rs.choice(np.array(ids + [0, 255], np.uint8), size=(h, w))
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(tmp_path / "val" / "image" / ("im%d.png" % i)))
        Image.fromarray(lab).save(str(tmp_path / "val" / "label" / ("im%d.png" % i)))
        raw.append(lab)
    lut = np.full(256, -1, np.int64)
    lut[ids] = np.arange(len(ids))
    val = {"batch_size": 1, "data_transformer": {"size_mode": "diverse_size", "fit_stride": 8, "align_method": "only_pad",
                                                 "pad_mode": "pad_right_down"}}
    trans = {"trans_seq": ["resize"], "resize": {"min_side_length": 32}}

    def batches(**val_keys):
        cfg = Configer(config_dict={"data": {"data_dir": str(tmp_path), "label_list": ids, "num_classes": 5, "workers": 1},
                                    "val": dict(val, **val_keys), "val_trans": trans})
        return list(DataLoader(cfg, dev).get_valloader())

    plain = batches()
    cubic = batches(score_resize="cubic")
    assert len(plain) == len(cubic) == 3
    for i, (p, c) in enumerate(zip(plain, cubic)):
        assert sorted(p) == ["img", "labelmap"] and sorted(c) == ["border_size", "img", "labelmap", "ori_labelmap"]
        assert torch.equal(p["labelmap"], c["labelmap"]) and torch.equal(p["img"], c["img"])      # labelmap is what it was
        assert len(c["ori_labelmap"]) == 1 and c["ori_labelmap"][0].dtype == torch.int64 and c["ori_labelmap"][0].device.type == dev.type
        assert np.array_equal(c["ori_labelmap"][0].cpu().numpy(), lut[raw[i]])
        (bw, bh), = c["border_size"]
        assert min(bw, bh) == 32 and c["labelmap"].shape[-2:] != raw[i].shape                     # the transform resampled
        assert bw <= c["img"].shape[-1] and bh <= c["img"].shape[-2]
    assert all(sorted(b) == ["img", "labelmap"] for b in batches(score_resize="bilinear"))
