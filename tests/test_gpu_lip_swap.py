"""LIP support on the device: the left / right label swap of random_hflip.swap_pair in both augmentation kernels (csrc/augment.hip,
csrc/augment_ragged.hip: cseg_augment_batch_swap, cseg_augment_ragged_swap), the channel permutation on the mirrored operand of the
scoring kernel (csrc/cseg_ms_fuse.h: cseg_ms_fuse_argmax_perm, cseg_ms_fuse_argmax_ragged_perm) and the scoring helper of the LIP
validation pass (segmentor/trainer_contrastive.py: score_mirrored_pair).

Yardsticks. The permuted scoring call against the call that existed before it on mirrored maps gathered along the class axis, bit for
bit; and against the float64 composition of tests/test_gpu_ms_eval.py with that file's bounds unchanged (fused map within
2 R + 2^-20 sum|w| max|logit|, R = torch's own fp32 deviation from float64; prediction = the float64 argmax where the margin exceeds
4 R, one of the top two elsewhere, at most 1 % of the pixels there). The validation helper against the float64 restatement of the
reference's tensor ops (segmentor/trainer_contrastive.py:335-345) with np.bincount. The augmentation against numpy written out from
the reference (cv2_aug_transforms.py:151-162) and against the forward composition of the oracle's primitives. Replayed on the CPU
emulation by tests/test_emu_lip_swap.py (the kernel-level tests; not the validation helper)."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_aug import DIV, MEAN, STD, _rows, _smooth_images
from test_gpu_aug_ragged import IDS, _lut, finish, literal, make_samples, pack
from test_gpu_ms_eval import _check_fused, _check_pred, _compose, _kernel_terms

pytestmark = pytest.mark.gpu

LIP_PAIRS = [[14, 15], [16, 17], [18, 19]]
LIP_PERM = list(range(14)) + [15, 14, 17, 16, 19, 18]
CYCLE3 = [1, 2, 0]
SIZES5 = [(5, 7), (10, 14), (19, 27), (37, 53), (48, 70)]
WEIGHTS5 = [0.5, 0.75, 1.0, 1.25, 1.5]
SCALES = {1: [1.0], 2: [0.5, 1.0], 3: [0.5, 1.0, 1.5], 5: [0.5, 0.75, 1.0, 1.25, 1.5]}
RAGGED3 = [((40, 56), (37, 53)), ((24, 32), (24, 30)), ((8, 8), (5, 7))]       # (padded, border)


def _dev():
    return torch.device("cuda:0")


# ---- inputs: the recipe of tests/test_gpu_ms_eval.py (seed 304, randn * 4, mirrored map = flip(a) + 0.5 randn) ----------------------
def _dense(n, K_, B, dev, sizes=SIZES5, weights=WEIGHTS5):
    g = torch.Generator().manual_seed(304)
    terms = []
    for i, (h, w) in enumerate(sizes[:n]):
        a = torch.randn(B, K_, h, w, generator=g) * 4
        b = torch.flip(a, dims=[3]) + 0.5 * torch.randn(B, K_, h, w, generator=g)
        terms.append((a.to(dev), b.to(dev), None if weights is None else weights[i]))
    return terms


def _ragged(n, K_, dev, weights=WEIGHTS5):
    g = torch.Generator().manual_seed(304)
    out = []
    for (Hp, Wp), border in RAGGED3:
        terms = []
        for i, s in enumerate(SCALES[n]):
            hc, wc = math.ceil(int(Hp * s) / 4), math.ceil(int(Wp * s) / 4)
            a = torch.randn(1, K_, hc, wc, generator=g) * 4
            b = torch.flip(a, dims=[3]) + 0.5 * torch.randn(1, K_, hc, wc, generator=g)
            terms.append((a.to(dev), b.to(dev), None if weights is None else weights[i]))
        out.append((terms, (Hp, Wp), border))
    return out


def _gathered(terms, p):
    """The operands of the call without a permutation: every mirrored map gathered along the class axis, channel k <- channel p[k]."""
    idx = torch.as_tensor(p, dtype=torch.long, device=terms[0][0].device)
    return [(a, None if b is None else b.index_select(1, idx).contiguous(), w) for a, b, w in terms]


def _gathered_images(images, p):
    return [(_kernel_terms(_gathered(terms, p)), padded, border) for terms, padded, border in images]


def _kernel_images(images):
    return [(_kernel_terms(terms), padded, border) for terms, padded, border in images]


# ---- 1. the permutation equals gathering first, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lip", "identity"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_dense_permutation_equals_gathering_first(n, which):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms = _dense(n, 20, 2, dev)
    p = LIP_PERM if which == "lip" else list(range(20))
    want_pred, want_fused = K.ms_fuse_argmax(_kernel_terms(_gathered(terms, p)), 37, 53, want_fused=True)
    pred, fused = K.ms_fuse_argmax(_kernel_terms(terms), 37, 53, want_fused=True, perm=p)
    assert torch.equal(pred, want_pred) and torch.equal(fused, want_fused)
    pred_t, fused_t = K.ms_fuse_argmax(_kernel_terms(terms), 37, 53, want_fused=True, perm=torch.tensor(p))
    assert torch.equal(pred_t, want_pred) and torch.equal(fused_t, want_fused)
    if which == "identity":                                # perm=None is the call as it was
        plain_pred, plain_fused = K.ms_fuse_argmax(_kernel_terms(terms), 37, 53, want_fused=True, perm=None)
        assert torch.equal(plain_pred, want_pred) and torch.equal(plain_fused, want_fused)
    else:                                                  # the permutation is not a no-op on these inputs
        assert not torch.equal(fused, K.ms_fuse_argmax(_kernel_terms(terms), 37, 53, want_fused=True)[1])


def test_dense_three_cycle_shows_the_direction():
    """Output class k reads class perm[k] of the mirrored map (the reference's outputs_rev[:, 14] = outputs_[.., 15]); an involution
    cannot tell that from its inverse, the 3-cycle can."""
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms = _dense(1, 3, 2, dev, sizes=[(3, 4)], weights=None)
    want_pred, want_fused = K.ms_fuse_argmax(_kernel_terms(_gathered(terms, CYCLE3)), 7, 9, want_fused=True)
    pred, fused = K.ms_fuse_argmax(_kernel_terms(terms), 7, 9, want_fused=True, perm=CYCLE3)
    assert torch.equal(pred, want_pred) and torch.equal(fused, want_fused)
    inverse = K.ms_fuse_argmax(_kernel_terms(_gathered(terms, [2, 0, 1])), 7, 9, want_fused=True)[1]
    assert not torch.equal(fused, inverse)


@pytest.mark.parametrize("which", ["lip", "identity"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_ragged_permutation_equals_gathering_first_and_the_dense_call(n, which):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    images = _ragged(n, 20, dev)
    p = LIP_PERM if which == "lip" else list(range(20))
    want = K.ms_fuse_argmax_ragged(_gathered_images(images, p), want_fused=True)
    out = K.ms_fuse_argmax_ragged(_kernel_images(images), want_fused=True, perm=p)
    assert torch.equal(out.pred, want.pred) and torch.equal(out.fused, want.fused)
    if which == "identity":
        none = K.ms_fuse_argmax_ragged(_kernel_images(images), want_fused=True, perm=None)
        assert torch.equal(none.pred, want.pred) and torch.equal(none.fused, want.fused)
    for k, (terms, (Hp, Wp), (h, w)) in enumerate(images):      # the dense call with the permutation, on every image alone
        pred, fused = K.ms_fuse_argmax(_kernel_terms(terms), Hp, Wp, want_fused=True, perm=p)
        assert torch.equal(out.preds[k], pred[0, :h, :w]), k
        assert torch.equal(out.fuseds[k], fused[0, :, :h, :w]), k


def test_ragged_three_cycle():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    images = _ragged(2, 3, dev, weights=None)
    want = K.ms_fuse_argmax_ragged(_gathered_images(images, CYCLE3), want_fused=True)
    out = K.ms_fuse_argmax_ragged(_kernel_images(images), want_fused=True, perm=CYCLE3)
    assert torch.equal(out.pred, want.pred) and torch.equal(out.fused, want.fused)
    inverse = K.ms_fuse_argmax_ragged(_gathered_images(images, [2, 0, 1]), want_fused=True)
    assert not torch.equal(out.fused, inverse.fused)


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------
def _yardstick(terms, H, W, p):
    """tests/test_gpu_ms_eval.py::_compose with the mirrored map gathered by perm, in float64 and in torch fp32 where the terms live.
    -> (d64, R, max|logit|, sum|w|)"""
    g = _gathered(terms, p)
    d64 = _compose(g, H, W, torch.float64)
    d32 = _compose(g, H, W, torch.float32)
    R = float((d32.double() - d64).abs().max())
    amax = max(float(t.abs().max()) for a, b, _ in terms for t in (a, b))
    wsum = sum(abs(1.0 if w is None else w) for _, _, w in terms)
    return d64, R, amax, wsum


def _near_tie_share(d64, R):
    top = d64.topk(2, dim=1).values
    return float(((top[:, 0] - top[:, 1]) <= 4 * R).double().mean())


F64_DENSE = {"lip5": (5, 20, 2, SIZES5, WEIGHTS5, (37, 53), LIP_PERM), "lip3": (3, 20, 2, SIZES5, None, (37, 53), LIP_PERM),
             "cycle": (1, 3, 2, [(3, 4)], None, (7, 9), CYCLE3)}


@pytest.mark.parametrize("case", list(F64_DENSE))
def test_dense_permuted_call_matches_the_float64_composition(case):
    from contrastiveseg_amd import kernels as K
    n, K_, B, sizes, weights, (H, W), p = F64_DENSE[case]
    # the chosen case leaves room for the prediction check: torch's own fp32 composition, on the CPU, before anything runs on the device
    cpu = _dense(n, K_, B, torch.device("cpu"), sizes, weights)
    d64c, Rc, _, _ = _yardstick(cpu, H, W, p)
    share = _near_tie_share(d64c, Rc)
    print("%s: CPU R %.3e, %.4f %% of the pixels within 4 R of a tie" % (case, Rc, 100 * share))
    assert share <= 0.01
    terms = _dense(n, K_, B, _dev(), sizes, weights)
    d64, R, amax, wsum = _yardstick(terms, H, W, p)
    pred, fused = K.ms_fuse_argmax(_kernel_terms(terms), H, W, want_fused=True, perm=p)
    _check_fused(case, fused, d64, R, amax, wsum)
    _check_pred(case, pred, d64, R)


@pytest.mark.parametrize("n,K_,p", [(3, 20, LIP_PERM), (2, 3, CYCLE3)])
def test_ragged_permuted_call_matches_the_float64_composition(n, K_, p):
    from contrastiveseg_amd import kernels as K
    for terms, (Hp, Wp), (h, w) in _ragged(n, K_, torch.device("cpu")):
        d64c, Rc, _, _ = _yardstick(terms, Hp, Wp, p)
        d64c = d64c[:, :, :h, :w]
        assert _near_tie_share(d64c, Rc) <= 0.01
    images = _ragged(n, K_, _dev())
    out = K.ms_fuse_argmax_ragged(_kernel_images(images), want_fused=True, perm=p)
    for k, (terms, (Hp, Wp), (h, w)) in enumerate(images):
        g = _gathered(terms, p)
        d64 = _compose(g, Hp, Wp, torch.float64)[:, :, :h, :w]
        d32 = _compose(g, Hp, Wp, torch.float32)[:, :, :h, :w]
        R = float((d32.double() - d64).abs().max())
        amax = max(float(t.abs().max()) for a, b, _ in terms for t in (a, b))
        wsum = sum(abs(1.0 if w_ is None else w_) for _, _, w_ in terms)
        _check_fused("ragged K=%d image %d" % (K_, k), out.fuseds[k][None], d64, R, amax, wsum)
        _check_pred("ragged K=%d image %d" % (K_, k), out.preds[k][None], d64, R)


# ---- 3. the scoring helper of the LIP validation pass ------------------------------------------------------------------------------------
def _reference_val(seg, size, dtype):
    """segmentor/trainer_contrastive.py:335-345 of the reference restated in `dtype`, then the bilinear upsampling to the label size
    that this project's validation pass applies before the argmax."""
    outputs_ = seg.to(dtype)
    half = int(outputs_.size(0) / 2)
    outputs = outputs_[0:half].clone()
    outputs_rev = outputs_[half:].clone()
    if outputs_rev.shape[1] == 20:
        for a, b in LIP_PAIRS:
            outputs_rev[:, a] = outputs_[half:, b]
            outputs_rev[:, b] = outputs_[half:, a]
    outputs_rev = torch.flip(outputs_rev, [3])
    outputs = (outputs + outputs_rev) / 2.
    return F.interpolate(outputs, size=size, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("path", ["fused", "torch"])
@pytest.mark.parametrize("K_", [20, 19])
def test_validation_helper_counts_what_the_float64_restatement_predicts(K_, path):
    from contrastiveseg_amd.lib.metrics.running_score import RunningScore
    from contrastiveseg_amd.segmentor.trainer_contrastive import lip_mirror_perm, score_mirrored_pair
    dev = _dev()
    g = torch.Generator().manual_seed(304)
    seg = (torch.randn(4, K_, 12, 12, generator=g) * 4).to(dev)
    targets = torch.randint(-1, K_, (2, 45, 45), generator=g).to(dev)
    d64 = _reference_val(seg, (45, 45), torch.float64)
    d32 = _reference_val(seg, (45, 45), torch.float32)
    R = float((d32.double() - d64).abs().max())
    top = d64.topk(2, dim=1)
    clear = (top.values[:, 0] - top.values[:, 1]) > 4 * R
    share = 1.0 - float(clear.double().mean())
    print("K=%d %s: R %.3e, %.4f %% of the pixels within 4 R of a tie" % (K_, path, R, 100 * share))
    assert share <= 0.01
    assert (lip_mirror_perm(K_) == LIP_PERM) if K_ == 20 else (lip_mirror_perm(K_) is None)
    # pixels within 4 R of a tie are left out on both sides: their target becomes the ignore label
    kept = torch.where(clear, targets, torch.full_like(targets, -1))
    t, p = kept.cpu().numpy().reshape(-1), top.indices[:, 0].cpu().numpy().reshape(-1)
    want = np.bincount(K_ * t[t >= 0] + p[t >= 0], minlength=K_ * K_).reshape(K_, K_)
    if path == "fused":
        hist = torch.zeros(K_, K_, dtype=torch.int64, device=dev)
        score_mirrored_pair(seg, kept, hist=hist)
        got = hist.cpu().numpy()
    else:
        score = RunningScore(num_classes=K_, ignore_index=-1)
        score_mirrored_pair(seg, kept, score=score)
        got = score.confusion_matrix.cpu().numpy()
    assert int(want.sum()) == int((t >= 0).sum()) > 0
    assert np.array_equal(got, want)
    with pytest.raises(ValueError, match="either hist"):
        score_mirrored_pair(seg, kept)
    with pytest.raises(ValueError, match="its mirror"):
        score_mirrored_pair(seg[:3], kept, hist=torch.zeros(K_, K_, dtype=torch.int64, device=dev))


# ---- 4. augmentation from first principles: a flip alone ---------------------------------------------------------------------------------
def _pair_loop(labelmap, pairs):
    """RandomHFlip._process_labelmap of the reference (cv2_aug_transforms.py:151-162) after its cv2.flip, written out."""
    temp = labelmap.copy()
    for a, b in pairs:
        labelmap[temp == a] = b
        labelmap[temp == b] = a
    return labelmap


def _flip_only_cfg(pairs, ratio, label_list=None):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    data = {"num_classes": 20}
    if label_list is not None:
        data["label_list"] = label_list
    return Configer(config_dict={
        "data": data,
        "train": {"data_transformer": {"size_mode": "fix_size", "input_size": [6, 5], "align_method": "only_pad", "pad_mode": "random"}},
        "train_trans": {"trans_seq": ["random_hflip"], "random_hflip": {"ratio": ratio, "swap_pair": pairs}},
        "normalize": {"div_value": DIV, "mean": MEAN, "std": STD}})


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("ratio", [1.0, 0.0])
@pytest.mark.parametrize("pairs,values", [(LIP_PAIRS, [13, 14, 15, 16, 17, 18, 19, 255]), ([[1, 2], [2, 3]], [0, 1, 2, 3, 4, 255])],
                         ids=["lip", "overlapping"])
def test_flip_alone_swaps_the_pairs_as_the_reference_loop_does(pairs, values, ratio, ragged):
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    dev = _dev()
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, size=(2, 5, 6, 3)).astype(np.uint8)
    lab = np.asarray(values, np.uint8)[rs.randint(0, len(values), size=(2, 5, 6))]
    lab.reshape(2, -1)[:, :len(values)] = values            # every value occurs in both images
    ti, tl = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    if ragged:
        ti, tl, sizes = ti.reshape(-1, 3), tl.reshape(-1), [(6, 5), (6, 5)]
    else:
        sizes = None
    random.seed(3)
    out = GPUBatchTransform(_flip_only_cfg(pairs, ratio))(ti, tl, sizes=sizes)
    random.seed(3)
    plain = GPUBatchTransform(_flip_only_cfg([], ratio))(ti, tl, sizes=sizes)
    assert out["aug_params"].shape[1] == (16 if ragged else 12)
    want = lab.copy()
    if ratio == 1.0:                                        # random.random() > 1.0 never holds: the flip is applied
        want = np.stack([_pair_loop(np.ascontiguousarray(np.flip(l, 1)), pairs) for l in lab])
    want = np.where(want == 255, -1, want.astype(np.int64))          # ReLabel(255, -1)
    assert np.array_equal(out["labelmap"].cpu().numpy(), want)
    assert torch.equal(out["img"], plain["img"])
    assert torch.equal(out["aug_params"], plain["aug_params"])
    if ratio == 1.0:
        assert not torch.equal(out["labelmap"], plain["labelmap"])
    else:
        assert torch.equal(out["labelmap"], plain["labelmap"])


# ---- 5. augmentation, composed: the LIP order on a ragged batch, the canonical order on a uniform one ---------------------------------
SWAP_IDS = [[7, 8], [11, 12], [31, 32], [20, 33]]           # raw ids of IDS, ahead of the label_list encoding
LIP_TRANS = {"trans_seq": ["random_hflip", "resize", "random_resize", "random_crop", "random_brightness"],
             "random_brightness": {"ratio": 1.0, "shift_value": 10},
             "resize": {"target_size": [40, 32]},
             "random_hflip": {"ratio": 0.5, "swap_pair": SWAP_IDS},
             "random_resize": {"ratio": 0.5, "method": "random", "scale_range": [0.5, 1.5], "aspect_range": [0.9, 1.1]},
             "random_crop": {"ratio": 1.0, "crop_size": [32, 24], "method": "random", "allow_outside_center": False}}
CANON_TRANS = {"trans_seq": ["random_resize", "random_crop", "random_hflip", "random_brightness"],
               "random_brightness": {"ratio": 0.7, "shift_value": 10},
               "random_hflip": {"ratio": 0.5, "swap_pair": SWAP_IDS},
               "random_resize": {"ratio": 0.9, "method": "random", "scale_range": [0.5, 2.0], "aspect_range": [0.9, 1.1]},
               "random_crop": {"ratio": 1.0, "crop_size": [32, 24], "method": "random", "allow_outside_center": False}}
LIP_SEEDS = (0, 1, 2, 3, 4, 5)


def _composed_cfg(trans, pairs=SWAP_IDS):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    trans = dict(trans, random_hflip=dict(trans["random_hflip"], swap_pair=pairs))
    return Configer(config_dict={
        "data": {"num_classes": 19, "label_list": IDS},
        "train": {"data_transformer": {"size_mode": "fix_size", "input_size": [32, 24], "align_method": "only_pad", "pad_mode": "random"}},
        "train_trans": trans, "normalize": {"div_value": DIV, "mean": MEAN, "std": STD}})


def _swap_values():
    swap = np.arange(256)
    for a, b in SWAP_IDS:
        swap[a], swap[b] = b, a
    return swap


def _literal_with_swap(img, lab, rec):
    """The forward composition of tests/test_gpu_aug_ragged.py::apply_record with the reference's pair loop at every flip."""
    W0, H0, W1, H1, m1, Wr, Hr, m2, x, y, tw, th, flip = [int(v) for v in rec[:13]]
    ops = []
    if W1 > 0:
        ops += [("flip",)] * m1 + [("resize", (W1, H1))]
    ops += [("flip",)] * m2 + [("resize", (Wr, Hr)), ("crop", x, y, tw, th)] + [("flip",)] * flip
    for op in ops:
        img, lab = literal(img, lab, [op])
        if op[0] == "flip":
            lab = _pair_loop(lab, SWAP_IDS)
    return img, lab


def test_lip_order_on_a_ragged_batch():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    dev = _dev()
    samples = make_samples(np.random.RandomState(21), [(32, 40), (29, 37), (45, 50)])      # (H, W); the first is resize's target size
    img, lab, _ = pack(samples)
    sizes = [(s[0].shape[1], s[0].shape[0]) for s in samples]
    ti, tl = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    t, t_plain = GPUBatchTransform(_composed_cfg(LIP_TRANS)), GPUBatchTransform(_composed_cfg(LIP_TRANS, []))
    lut = _lut()
    assert np.array_equal(t.lut.numpy(), lut) and np.array_equal(t.lut_mirrored.numpy(), lut[_swap_values()])
    lut_d, lut_swapped_d = torch.from_numpy(lut).to(dev), torch.from_numpy(np.ascontiguousarray(lut[_swap_values()])).to(dev)
    seen = set()
    for seed in LIP_SEEDS:
        random.seed(seed)
        out = t(ti, tl, sizes=sizes)
        random.seed(seed)
        plain = t_plain(ti, tl, sizes=sizes)
        params, offsets = out["aug_params"], out["aug_offsets"]
        assert torch.equal(params, plain["aug_params"]) and torch.equal(out["img"], plain["img"])
        recs = params.cpu().numpy()
        mid = K.resize_ragged(ti, tl, params, offsets) if (recs[:, 2] > 0).any() else None
        even = K.augment_ragged(ti, tl, lut_d, params, offsets, (24, 32), DIV, MEAN, STD, mid=mid)[1]
        odd = K.augment_ragged(ti, tl, lut_swapped_d, params, offsets, (24, 32), DIV, MEAN, STD, mid=mid)[1]
        got = out["labelmap"]
        for b, (im0, lb0) in enumerate(samples):
            r = recs[b]
            parity = int(r[4]) ^ int(r[7]) ^ int(r[12])
            seen |= {name for name, bit in (("m1", r[4]), ("m2", r[7]), ("flip", r[12]), ("twice", r[2] > 0), ("even", not parity)) if bit}
            seen |= {"two flips"} if int(r[4]) + int(r[7]) + int(r[12]) >= 2 else set()
            assert torch.equal(got[b], (odd if parity else even)[b]), (seed, b)
            im, lb = _literal_with_swap(im0, lb0, r)
            _, want_lab = finish(im, lb, r[13], r[14], r[15], 32, 24, lut)
            assert np.array_equal(got[b].cpu().numpy(), want_lab), (seed, b)
    assert {"m1", "m2", "flip", "twice", "even"} <= seen, seen


def test_canonical_order_on_a_uniform_batch():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    dev = _dev()
    rs = np.random.RandomState(22)
    B, Hs, Ws = 6, 40, 48
    img = _smooth_images(rs, B, Hs, Ws)
    lab = rs.randint(0, 34, size=(B, Hs, Ws)).astype(np.uint8)
    lab[rs.rand(B, Hs, Ws) < 0.05] = 255
    ti, tl = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    t, t_plain = GPUBatchTransform(_composed_cfg(CANON_TRANS)), GPUBatchTransform(_composed_cfg(CANON_TRANS, []))
    assert t.aug.canonical
    lut = _lut()
    lut_d, lut_swapped_d = torch.from_numpy(lut).to(dev), torch.from_numpy(np.ascontiguousarray(lut[_swap_values()])).to(dev)
    random.seed(8)
    out = t(ti, tl)
    random.seed(8)
    plain = t_plain(ti, tl)
    params = out["aug_params"]
    assert params.shape == (B, 12) and torch.equal(params, plain["aug_params"]) and torch.equal(out["img"], plain["img"])
    even = K.augment_batch(ti, tl, lut_d, params, (24, 32), DIV, MEAN, STD)[1]
    odd = K.augment_batch(ti, tl, lut_swapped_d, params, (24, 32), DIV, MEAN, STD)[1]
    rows = params.cpu().numpy()
    assert 0 < int(rows[:, 6].sum()) < B                    # both sides of the coin
    for b in range(B):
        r = rows[b]
        assert torch.equal(out["labelmap"][b], (odd if r[6] else even)[b]), b
        rec = [Ws, Hs, 0, 0, 0, r[0], r[1], 0] + [int(v) for v in r[2:10]]
        im, lb = _literal_with_swap(img[b], lab[b], rec)
        _, want_lab = finish(im, lb, r[7], r[8], r[9], 32, 24, lut)
        assert np.array_equal(out["labelmap"][b].cpu().numpy(), want_lab), b


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def _raw_dense(dev, perm, flipped=True):
    """cseg_ms_fuse_argmax_perm itself, past the wrapper, on a prediction buffer filled with 7: a refusal launches nothing."""
    from contrastiveseg_amd import _hip
    a, b = torch.zeros(1, 4, 3, 5, device=dev), torch.zeros(1, 4, 3, 5, device=dev)
    pred = torch.full((60,), 7, dtype=torch.uint8, device=dev)
    table = (ctypes.c_ubyte * len(perm))(*perm)
    try:
        _hip.call("cseg_ms_fuse_argmax_perm", 1, (ctypes.c_void_p * 1)(a.data_ptr()), (ctypes.c_void_p * 1)(b.data_ptr() if flipped else None),
                  (ctypes.c_int * 1)(3), (ctypes.c_int * 1)(5), (ctypes.c_float * 1)(1.0), table, 1, 4, 6, 10,
                  ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(None), _hip.stream_ptr())
    finally:
        if dev.type == "cuda":
            torch.cuda.synchronize()
    return pred


def test_refusals():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUAugCompose, GPUBatchTransform
    dev = _dev()
    a, b = torch.randn(1, 4, 3, 5, device=dev), torch.randn(1, 4, 3, 5, device=dev)
    one = ([(a, b, 1.0)], (6, 10), (6, 10))
    # the wrapper
    with pytest.raises(RuntimeError, match="perm has 3 entries for 4 classes"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, perm=[0, 1, 2])
    with pytest.raises(RuntimeError, match=r"perm\[2\] = 256 is not a class index"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, perm=[0, 1, 256, 3])
    with pytest.raises(RuntimeError, match="perm has 5 entries for 4 classes"):
        K.ms_fuse_argmax_ragged([one], perm=[0, 1, 2, 3, 4])
    with pytest.raises(RuntimeError, match=r"perm\[0\] = -1 is not a class index"):
        K.ms_fuse_argmax_ragged([one], perm=[-1, 1, 2, 3])
    # the library, through the wrapper
    for call in (lambda p, fl=b: K.ms_fuse_argmax([(a, fl, 1.0)], 6, 10, perm=p),
                 lambda p, fl=b: K.ms_fuse_argmax_ragged([([(a, fl, 1.0)], (6, 10), (6, 10))], perm=p)):
        with pytest.raises(RuntimeError, match=r"perm\[1\] = 4 is not a class"):
            call([0, 4, 2, 3])
        with pytest.raises(RuntimeError, match=r"perm\[3\] = 1 repeats an earlier entry \(not a permutation\)"):
            call([0, 1, 2, 1])
        with pytest.raises(RuntimeError, match="no term has a flipped map"):
            call([0, 1, 3, 2], None)
    # the library alone: accepted as it stands, then refused with the buffer untouched
    assert bool((_raw_dense(dev, [0, 1, 3, 2]) == 0).all())
    for perm, flipped, what in (([0, 9, 2, 3], True, "is not a class"), ([2, 2, 0, 1], True, "not a permutation"),
                                ([0, 1, 3, 2], False, "no term has a flipped map")):
        with pytest.raises(RuntimeError, match=what):
            _raw_dense(dev, perm, flipped)
    # the label swap: the tables of the wrappers, the pairs of the transform
    img, lab = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev), torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev)
    row = torch.tensor([[4, 4, 0, 0, 4, 4, 1, 0, 0, 0, 0, 0]], dtype=torch.int32)
    short = torch.zeros(255, dtype=torch.int16, device=dev)
    with pytest.raises(RuntimeError, match="lut_mirrored has 255 entries"):
        K.augment_batch(img, lab, None, row, (4, 4), DIV, MEAN, STD, lut_mirrored=short)
    rec = torch.tensor([[4, 4, 0, 0, 0, 4, 4, 0, 0, 0, 4, 4, 1, 0, 0, 0]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="lut_mirrored has 255 entries"):
        K.augment_ragged(img.reshape(-1, 3), lab.reshape(-1), None, rec, torch.zeros(1, 2, dtype=torch.int64), (4, 4), DIV, MEAN, STD,
                         lut_mirrored=short)
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            K.augment_batch(img, lab, None, row, (4, 4), DIV, MEAN, STD, lut_mirrored=torch.zeros(256, dtype=torch.int16))
    for pairs, what in (([[14, 255]], "mentions 255"), ([[14, 15, 16]], "two integer label ids"), ([[14, 1.5]], "two integer label ids"),
                        ([[14, 256]], "0..254"), ([[-1, 3]], "0..254")):
        with pytest.raises(ValueError, match=what):
            GPUAugCompose(_flip_only_cfg(pairs, 0.5))
    assert GPUBatchTransform(_flip_only_cfg(None, 0.5)).lut_mirrored is None


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    dev = _dev()
    terms = _kernel_terms(_dense(5, 20, 2, dev))
    p1, f1 = K.ms_fuse_argmax(terms, 37, 53, want_fused=True, perm=LIP_PERM)
    p2, f2 = K.ms_fuse_argmax(terms, 37, 53, want_fused=True, perm=LIP_PERM)
    assert torch.equal(p1, p2) and torch.equal(f1, f2)
    images = _kernel_images(_ragged(3, 20, dev))
    one = K.ms_fuse_argmax_ragged(images, want_fused=True, perm=LIP_PERM)
    two = K.ms_fuse_argmax_ragged(images, want_fused=True, perm=LIP_PERM)
    assert torch.equal(one.pred, two.pred) and torch.equal(one.fused, two.fused)
    samples = make_samples(np.random.RandomState(21), [(32, 40), (29, 37), (45, 50)])
    img, lab, _ = pack(samples)
    sizes = [(s[0].shape[1], s[0].shape[0]) for s in samples]
    ti, tl = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    t = GPUBatchTransform(_composed_cfg(LIP_TRANS))
    outs = []
    for _ in range(2):
        random.seed(2)
        outs.append(t(ti, tl, sizes=sizes))
    assert torch.equal(outs[0]["img"], outs[1]["img"]) and torch.equal(outs[0]["labelmap"], outs[1]["labelmap"])
