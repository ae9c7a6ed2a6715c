"""The Lovasz-softmax segmentation term (csrc/lovasz.hip: kernels.lovasz_errors / lovasz_order / lovasz_grad / lovasz_softmax,
loss_helper.FSCELOVASZLoss / FSAuxCELOVASZLoss) and the memory criteria with contrast.use_lovasz.

Yardsticks, never the code under test:
  (a) tests/golden/lovasz_<case>.npz, made by tools/gen_lovasz_golden.py from the reference's own lovasz_softmax_flat / flatten_probas on
      softmax(F.interpolate(seg)) on the CPU: loss and d loss / d seg in fp32 and in float64, and R_e, the deviation of the reference's
      fp32 probabilities from float64.
  (b) `restate` below: the same term with torch ops in float64 and the project's order (descending e, ascending flat pixel index among
      equal e, invalid pixels last); with `order` it uses the given permutation. tests/test_lovasz_host.py pins (b) to (a) at 1e-10.
R = the deviation of the reference's fp32 result from float64 on the case, for the quantity compared:
  errors     |e - e64| <= 2 R_e + 2^-24 at every valid pixel (cases without a fixture: R_e from torch's softmax of F.interpolate in fp32
             and float64, which is what the generator records); fg, G, the valid count and the bad-label count exact
  order      perm == the indices of torch.sort(e, stable=True, descending=True) on the kernel's own e with invalid pixels at -1, exactly
  grad       g against the float64 lovasz_grad(fg[perm]): 1e-12 relative + 1e-15; loss_c against the float64 dot product: 1e-12 relative
  loss       |loss - loss64| <= 2 R_loss + 2^-20 |loss64|
  d seg      max |dseg - dseg64| <= 2 R_g + 2^-20 max |dseg64|; on `ties` and `sat` against (b) evaluated with the kernel's order (float64
             breaks exact fp32 ties differently, and the gradient, unlike the loss, depends on the order among equal e)
Replayed on the CPU emulation by tests/test_emu_lovasz.py."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _dev():
    return torch.device("cuda:0")


# name: (B, K, h, w, H, W), amplitude, variant. Labels: 8 x 8 blocks, 10 % of the pixels ignored (-1) unless the variant says otherwise.
CASES = {
    "tiny": ((1, 3, 3, 3, 5, 5), 3.0, "no_ignore"),          # P = 25: less than one wave
    "multi": ((2, 5, 9, 11, 33, 41), 3.0, None),             # P = 2706: two sort tiles, ragged last one
    "big": ((2, 4, 24, 20, 95, 77), 3.0, None),              # P = 14 630: eight sort tiles of 2048 keys per class, ragged last one
    "absent": ((2, 6, 8, 8, 29, 31), 3.0, "absent"),         # classes 1 and 4 relabelled away: only_present, mean over 4
    "ident": ((2, 5, 32, 40, 32, 40), 3.0, None),            # identity resize
    "k19": ((1, 19, 16, 32, 64, 128), 3.0, None),            # Cityscapes class count
    "ties": ((2, 4, 12, 10, 45, 37), 4.0, "ties"),           # logits rounded to multiples of 2.0: exact fp32 ties, spanning tiles
    "sat": ((1, 4, 10, 10, 37, 37), 60.0, None),             # e exactly 0 and exactly 1
    "chunk": ((1, 37, 5, 6, 17, 21), 3.0, None),             # K not a multiple of the class chunk
    "void": ((2, 4, 6, 6, 21, 21), 3.0, "void"),             # image 1 all ignored
    "void_all": ((2, 4, 6, 6, 21, 21), 3.0, "void_all"),     # no valid pixel at all
}
FIXTURES = ("tiny", "multi", "big", "absent", "ident", "k19", "ties", "sat")


def inputs(name):
    """Seeded inputs of a case on the CPU: seg f32 [B,K,h,w], target i64 [B,H,W]."""
    (B, K, h, w, H, W), amp, variant = CASES[name]
    g = torch.Generator().manual_seed(304)
    seg = torch.randn(B, K, h, w, generator=g) * amp
    if variant == "ties":
        seg = torch.round(seg / 2.0) * 2.0
    blocks = torch.randint(0, K, (B, (H + 7) // 8, (W + 7) // 8), generator=g)
    target = blocks.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)[:, :H, :W].contiguous()
    if variant != "no_ignore":
        target[torch.rand(B, H, W, generator=g) < 0.10] = -1
    if variant == "absent":
        target[target == 1] = 0
        target[target == 4] = 3
    elif variant == "void":
        target[1] = -1
    elif variant == "void_all":
        target[:] = -1
    return seg, target


def lovasz_grad64(fg_sorted):
    """lovasz_grad of the reference (lib/loss/lovasz_loss.py:241-252) on a float64 0/1 vector."""
    gts = fg_sorted.sum()
    jaccard = 1.0 - (gts - fg_sorted.cumsum(0)) / (gts + (1.0 - fg_sorted).cumsum(0))
    out = jaccard.clone()
    out[1:] = jaccard[1:] - jaccard[:-1]
    return out


def stable_order(e, valid):
    """The project's order of one class: descending e, ascending index among equal e, invalid pixels last."""
    return torch.sort(torch.where(valid, e, torch.full_like(e, -1.0)), stable=True, descending=True).indices


def restate(seg, target, order=None, dtype=torch.float64):
    """The Lovasz-softmax term on F.interpolate(seg) restated with torch ops in `dtype`: mean over the classes present among the valid
    pixels (0 <= label < K) of dot(e sorted, lovasz_grad(fg sorted)); no valid pixel: 0. `order` (int [K,P]) replaces the sort.
    -> dict(loss, e [K,P], fg [K,P], valid [P], loss_c [K], present) -- loss is differentiable with respect to seg."""
    B, K = seg.shape[:2]
    H, W = target.shape[-2:]
    p = F.softmax(F.interpolate(seg.to(dtype), size=(H, W), mode="bilinear", align_corners=True), dim=1)
    p = p.permute(1, 0, 2, 3).reshape(K, -1)
    t = target.reshape(-1)
    valid = (t >= 0) & (t < K)
    fg = ((t[None, :] == torch.arange(K, device=t.device)[:, None]) & valid[None, :])
    e = (fg.to(dtype) - p).abs()
    loss_c = []
    for c in range(K):
        if not bool(fg[c].any()):
            loss_c.append(e[c].sum() * 0.0)
            continue
        perm = stable_order(e[c].detach(), valid) if order is None else order[c].long()
        g = lovasz_grad64(fg[c][perm].double()).to(dtype)
        loss_c.append(((e[c] * valid.to(dtype))[perm] * g).sum())
    loss_c = torch.stack(loss_c)
    present = int(fg.any(dim=1).sum())
    loss = loss_c.sum() / present if present else loss_c.sum()
    return dict(loss=loss, e=e, fg=fg, valid=valid, loss_c=loss_c, present=present)


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Inputs, the golden file (None without one) and the float64 restatement of one case, computed once and shared (never modified)."""
    dev = torch.device(dev_str)
    seg, target = inputs(name)
    gold = None
    if name in FIXTURES:
        gold = dict(np.load(os.path.join(GOLDEN, "lovasz_%s.npz" % name)))
        assert np.array_equal(gold["target"].astype(np.int64), target.numpy()), "the fixture was made from other labels"
        assert abs(float(seg.double().sum()) - float(gold["seg_sum"])) <= 1e-6, "the fixture was made from other logits"
        R_e = float(gold["R_e"])
    else:
        up = F.interpolate(seg, size=target.shape[-2:], mode="bilinear", align_corners=True)
        up64 = F.interpolate(seg.double(), size=target.shape[-2:], mode="bilinear", align_corners=True)
        R_e = float((F.softmax(up, dim=1).double() - F.softmax(up64, dim=1)).abs().max())
    seg, target = seg.to(dev), target.to(dev)
    with torch.no_grad():
        r64 = restate(seg, target)
    return seg, target, gold, r64, R_e


def _R(gold):
    R_loss = abs(float(gold["loss32"]) - float(gold["loss64"]))
    R_g = float(np.abs(gold["dseg32"].astype(np.float64) - gold["dseg64"]).max())
    return R_loss, R_g


# ---- stage 1: errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_errors_match_float64_and_the_counts_are_exact(case):
    from contrastiveseg_amd import kernels as K
    seg, target, gold, r64, R_e = _case(case, str(_dev()))
    K_ = seg.shape[1]
    P = target.numel()
    e, fg, counts = K.lovasz_errors(seg, target)
    assert e.shape == fg.shape == (K_, P) and e.dtype == torch.float32 and fg.dtype == torch.uint8
    valid = r64["valid"]
    assert torch.equal(fg.bool(), r64["fg"])
    assert bool((e[:, ~valid] == -1.0).all()), "invalid pixels carry e = -1"
    err = float((e.double() - r64["e"])[:, valid].abs().max()) if bool(valid.any()) else 0.0
    print("%s: R_e %.3e  e vs float64 %.3e  bound %.3e" % (case, R_e, err, 2 * R_e + 2.0 ** -24))
    assert err <= 2 * R_e + 2.0 ** -24, (case, err, R_e)
    if bool(valid.any()):
        assert float(e[:, valid].min()) >= 0.0 and float(e[:, valid].max()) <= 1.0
    assert counts.dtype == torch.int32 and counts.shape == (K_ + 2,)
    assert torch.equal(counts[:K_].long(), r64["fg"].sum(dim=1))
    assert int(counts[K_]) == int(valid.sum()) and int(counts[K_ + 1]) == 0


def test_bad_labels_are_dropped_and_counted():
    from contrastiveseg_amd import kernels as K
    seg, target, _, r64, _ = _case("multi", str(_dev()))
    K_ = seg.shape[1]
    planted = target.clone()
    where = torch.nonzero(r64["valid"].reshape(target.shape))[[5, 700, 1900]]
    for b, y, x in where.tolist():
        planted[b, y, x] = K_
    status = torch.zeros(4, dtype=torch.int32, device=seg.device)
    e, fg, counts = K.lovasz_errors(seg, planted, status=status)
    assert int(status[1]) == 3 and int(counts[K_ + 1]) == 3 and int(counts[K_]) == int(r64["valid"].sum()) - 3
    flat = (where[:, 0] * target.shape[1] + where[:, 1]) * target.shape[2] + where[:, 2]
    assert bool((e[:, flat] == -1.0).all()) and int(fg[:, flat].sum()) == 0
    # the fused route counts them once per call, in the sticky word, and the term is the one of the labels with those pixels ignored
    loss = K.lovasz_softmax(seg, planted, status=status)
    ignored = planted.clone()
    ignored[planted == K_] = -1
    assert int(status[1]) == 6 and torch.equal(loss, K.lovasz_softmax(seg, ignored))
    # with another ignore index the -1 labels are bad labels too
    _, _, counts = K.lovasz_errors(seg, target, ignore_index=255)
    assert int(counts[K_ + 1]) == int((target == -1).sum())


# ---- stage 2: order --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_order_is_the_stable_descending_sort(case):
    from contrastiveseg_amd import kernels as K
    seg, target, _, r64, _ = _case(case, str(_dev()))
    e, fg, _ = K.lovasz_errors(seg, target)
    perm = K.lovasz_order(e, fg)
    assert perm.dtype == torch.int32 and perm.shape == e.shape
    valid = r64["valid"]
    ties = 0
    for c in range(e.shape[0]):
        want = stable_order(e[c], valid)
        assert torch.equal(perm[c].long(), want), (case, c)
        es = e[c][want][:int(valid.sum())]
        ties += int((es[1:] == es[:-1]).sum())
    print("%s: %d sorted neighbours with equal e" % (case, ties))
    if case == "ties":
        assert ties >= 1000, "the case is there for exact fp32 ties"
    if case == "sat":
        assert bool((e[:, valid] == 0.0).any()) and bool((e[:, valid] == 1.0).any()), "the case is there for e exactly 0 and exactly 1"


def test_order_of_equal_keys_is_the_pixel_order():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    P = 5000                                              # three tiles, ragged last one
    e = torch.full((2, P), 0.25, device=dev)
    e[1, 1234:1300] = -1.0                                # one run of invalid pixels: they go last, in pixel order
    fg = (torch.arange(2 * P, device=dev).reshape(2, P) % 3 == 0).to(torch.uint8)       # fg takes no part in the order
    perm = K.lovasz_order(e, fg)
    idx = torch.arange(P, device=dev)
    assert torch.equal(perm[0].long(), idx)
    assert torch.equal(perm[1].long(), torch.cat([idx[:1234], idx[1300:], idx[1234:1300]]))


# ---- stage 3: grad ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_grad_matches_the_float64_jaccard_differences(case):
    from contrastiveseg_amd import kernels as K
    seg, target, _, r64, _ = _case(case, str(_dev()))
    e, fg, _ = K.lovasz_errors(seg, target)
    perm = K.lovasz_order(e, fg)
    g, loss_c = K.lovasz_grad(fg, perm, e)
    assert g.dtype == torch.float64 and g.shape == e.shape and loss_c.shape == (e.shape[0],)
    valid = r64["valid"]
    worst = 0.0
    for c in range(e.shape[0]):
        if not bool(fg[c].any()):
            assert float(g[c].abs().max()) == 0.0 and float(loss_c[c]) == 0.0, "an absent class has no term"
            continue
        p = perm[c].long()
        want = lovasz_grad64(fg[c][p].double())
        assert bool(((g[c] - want).abs() <= 1e-12 * want.abs() + 1e-15).all()), (case, c, float((g[c] - want).abs().max()))
        dot = float(((e[c].double() * valid.double())[p] * want).sum())
        worst = max(worst, abs(float(loss_c[c]) - dot) / abs(dot) if dot else abs(float(loss_c[c])))
        assert abs(float(loss_c[c]) - dot) <= 1e-12 * abs(dot), (case, c, float(loss_c[c]), dot)
    print("%s: loss_c vs the float64 dot product, worst relative %.3e" % (case, worst))


# ---- the fused route against the reference ---------------------------------------------------------------------------------------------------
def _run(seg, target, **kw):
    from contrastiveseg_amd import kernels as K
    x = seg.clone().requires_grad_(True)
    before = target.clone()
    loss, terms = K.lovasz_softmax(x, target, want_terms=True, **kw)
    loss.backward()
    assert torch.equal(target, before), "the label tensor was modified"
    return loss.detach(), terms, x.grad


def _check_loss(case, loss, terms, gold, r64):
    R_loss, _ = _R(gold)
    want = float(gold["loss64"])
    err = abs(float(loss) - want)
    print("%s: loss %.9g  float64 %.9g  R_loss %.3e  kernel vs float64 %.3e  bound %.3e" % (
        case, float(loss), want, R_loss, err, 2 * R_loss + 2.0 ** -20 * abs(want)))
    assert err <= 2 * R_loss + 2.0 ** -20 * abs(want), (case, err, R_loss)
    assert abs(float(terms[0]) - want) <= 2 * R_loss + 2.0 ** -20 * abs(want) and float(terms[1]) == r64["present"]


@pytest.mark.parametrize("case", ["tiny", "multi", "big", "absent", "ident", "k19"])
def test_loss_and_gradient_match_the_reference(case):
    seg, target, gold, r64, _ = _case(case, str(_dev()))
    _, R_g = _R(gold)
    loss, terms, grad = _run(seg, target)
    _check_loss(case, loss, terms, gold, r64)
    g64 = torch.from_numpy(gold["dseg64"]).to(seg.device)
    gerr = float((grad.double() - g64).abs().max())
    gmax = float(g64.abs().max())
    print("%s: R_g %.3e  d seg vs float64 %.3e  bound %.3e  max|g64| %.3e" % (case, R_g, gerr, 2 * R_g + 2.0 ** -20 * gmax, gmax))
    assert bool(torch.isfinite(grad).all())
    assert gerr <= 2 * R_g + 2.0 ** -20 * gmax, (case, gerr, R_g, gmax)


@pytest.mark.parametrize("case", ["ties", "sat"])
def test_ties_and_saturation_against_float64_in_the_kernels_order(case):
    from contrastiveseg_amd import kernels as K
    seg, target, gold, r64, _ = _case(case, str(_dev()))
    _, R_g = _R(gold)
    loss, terms, grad = _run(seg, target)
    _check_loss(case, loss, terms, gold, r64)
    e, fg, _ = K.lovasz_errors(seg, target)
    perm = K.lovasz_order(e, fg)                           # validated by test_order_is_the_stable_descending_sort
    x64 = seg.double().requires_grad_(True)
    restate(x64, target, order=perm)["loss"].backward()    # torch's abs has gradient 0 at 0: pixels with e == 0 contribute nothing
    gerr = float((grad.double() - x64.grad).abs().max())
    gmax = float(x64.grad.abs().max())
    print("%s: R_g %.3e  d seg vs float64 in the kernel's order %.3e  bound %.3e  max|g64| %.3e" % (
        case, R_g, gerr, 2 * R_g + 2.0 ** -20 * gmax, gmax))
    assert bool(torch.isfinite(grad).all())
    assert gerr <= 2 * R_g + 2.0 ** -20 * gmax, (case, gerr, R_g, gmax)


def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    seg, target, _, _, _ = _case("big", str(_dev()))
    a, b = _run(seg, target), _run(seg, target)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    with torch.no_grad():
        assert torch.equal(K.lovasz_softmax(seg, target), a[0])


def test_class_chunks_give_the_same_bits():
    from contrastiveseg_amd import kernels as K
    seg, target, _, r64, _ = _case("chunk", str(_dev()))
    default = K.LOVASZ_CLASS_CHUNK
    assert default != 8 and seg.shape[1] % 8 != 0 and seg.shape[1] % default != 0
    want = _run(seg, target)
    try:
        K.LOVASZ_CLASS_CHUNK = 8
        got = _run(seg, target)
    finally:
        K.LOVASZ_CLASS_CHUNK = default
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert abs(float(want[0]) - float(r64["loss"])) <= 1e-5 * float(r64["loss"]) and float(want[1][1]) == r64["present"]


def test_void_images():
    """Image 1 all ignored: the term and the gradient of image 0 are, bit for bit, those of image 0 alone (invalid pixels sort after every
    valid one and change no earlier Jaccard value), image 1 gets exactly 0. No valid pixel at all: the term and the gradient are exactly
    0 (the reference returns an empty tensor there)."""
    seg, target, _, r64, _ = _case("void", str(_dev()))
    loss, terms, grad = _run(seg, target)
    alone = _run(seg[:1].contiguous(), target[:1].contiguous())
    assert torch.equal(loss, alone[0]) and torch.equal(grad[:1], alone[2]) and float(grad[1].abs().max()) == 0.0
    assert abs(float(loss) - float(r64["loss"])) <= 1e-5 * float(r64["loss"]) and float(grad[0].abs().max()) > 0
    seg, target, _, _, _ = _case("void_all", str(_dev()))
    loss, terms, grad = _run(seg, target)
    assert float(loss) == 0.0 and float(terms[0]) == 0.0 and float(terms[1]) == 0.0 and float(grad.abs().max()) == 0.0


def test_no_gradient_buffer_without_a_gradient_to_compute():
    """With a gradient the route keeps G_buf [K,P] f32, the one buffer of the size of the upsampled logits; under no_grad it does not
    exist: the peak is the sort workspace of one class chunk."""
    from contrastiveseg_amd import kernels as K
    seg, target, _, _, _ = _case("k19", str(_dev()))
    if seg.device.type != "cuda":
        with torch.no_grad():
            K.lovasz_softmax(seg, target)
        return
    K_, P = seg.shape[1], target.numel()
    x = seg.clone().requires_grad_(True)
    peaks = []
    for grad in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.set_grad_enabled(grad):
            loss = K.lovasz_softmax(x, target)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - before)
        del loss
    print("peak growth without / with a gradient: %d / %d bytes; G_buf is %d" % (peaks[0], peaks[1], K_ * P * 4))
    assert peaks[0] < K_ * P * 4 and peaks[1] >= K_ * P * 4


def test_no_host_synchronisation():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    seg, target, _, _, _ = _case("multi", str(_dev()))
    crit = SEG_LOSS_DICT["mem_contrast_ce_loss"](_cfg("mem_contrast_ce_loss", seg.shape[1])).to(seg.device)

    def both():
        x = seg.clone().requires_grad_(True)
        K.lovasz_softmax(x, target).backward()
        y = seg.clone().requires_grad_(True)
        crit.seg_criterion(y, target).backward()
        return x.grad, y.grad

    both()                                                # first use: the library is loaded, the allocator is warm
    if seg.device.type != "cuda":
        return
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gx, gy = both()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())


# ---- the memory criteria with contrast.use_lovasz --------------------------------------------------------------------------------------------
def _cfg(loss_type, K_, use_lovasz=True, use_rmi=False, **params):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    p = {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}
    p.update(params)
    return Configer(config_dict={
        "data": {"num_classes": K_}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": 4},
        "contrast": dict(proj_dim=16, temperature=0.1, base_temperature=0.07, max_samples=64, max_views=4, loss_weight=0.1,
                         use_rmi=use_rmi, use_lovasz=use_lovasz, warmup_iters=0, with_memory=True, memory_size=8, pixel_update_freq=2),
        "loss": {"loss_type": loss_type, "params": p}})


def _criterion_inputs(dev):
    seg, target = inputs("multi")
    g = torch.Generator().manual_seed(305)
    B, K_, h, w = seg.shape
    aux = torch.randn(B, K_, h, w, generator=g) * 2
    embed = F.normalize(torch.randn(B, 16, h, w, generator=g), dim=1)
    return seg.to(dev), aux.to(dev), embed.to(dev), target.to(dev)


def _ce(x, target, dtype):
    return F.cross_entropy(F.interpolate(x.to(dtype), size=target.shape[-2:], mode="bilinear", align_corners=True), target, ignore_index=-1)


@pytest.mark.parametrize("loss_type,queues", [("mem_contrast_ce_loss", False), ("mem_contrast_ce_loss", True),
                                              ("mem_contrast_auxce_loss", False), ("mem_contrast_auxce_loss", True)])
def test_memory_criteria_with_use_lovasz(loss_type, queues):
    from contrastiveseg_amd.lib.loss.loss_helper import FSAuxCELOVASZLoss, FSCELOVASZLoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    K_ = 5
    seg, aux, embed, target = _criterion_inputs(dev)
    crit = SEG_LOSS_DICT[loss_type](_cfg(loss_type, K_)).to(dev)
    has_aux = "aux" in loss_type
    assert type(crit.seg_criterion) is (FSAuxCELOVASZLoss if has_aux else FSCELOVASZLoss)
    preds = {"seg": seg.clone().requires_grad_(True), "embed": embed.clone().requires_grad_(True)}
    if has_aux:
        preds["seg_aux"] = aux.clone().requires_grad_(True)
    if queues:
        g = torch.Generator().manual_seed(306)
        preds["segment_queue"] = F.normalize(torch.randn(K_, 8, 16, generator=g), dim=2).to(dev)
        preds["pixel_queue"] = F.normalize(torch.randn(K_, 8, 16, generator=g), dim=2).to(dev)
    torch.manual_seed(304)
    total = crit(preds, target, with_embed=True)
    total.backward()
    assert bool(torch.isfinite(total.detach())) and bool(torch.isfinite(preds["seg"].grad).all()) and float(preds["seg"].grad.abs().max()) > 0
    if has_aux:
        assert float(preds["seg_aux"].grad.abs().max()) > 0
    # the segmentation term against float64: CE + Lovasz (+ 0.4 CE of the auxiliary map); R composed of the parts' R
    gold = dict(np.load(os.path.join(GOLDEN, "lovasz_multi.npz")))
    R_loss, _ = _R(gold)
    with torch.no_grad():
        want = _ce(seg, target, torch.float64) + restate(seg, target)["loss"]
        R_loss = R_loss + abs(float(_ce(seg, target, torch.float32)) - float(_ce(seg, target, torch.float64)))
        if has_aux:
            want = 1.0 * want + 0.4 * _ce(aux, target, torch.float64)
            R_loss = R_loss + 0.4 * abs(float(_ce(aux, target, torch.float32)) - float(_ce(aux, target, torch.float64)))
    got = float(crit.last_terms[0])
    print("%s queues=%s: segmentation term %.9g  float64 %.9g  R %.3e" % (loss_type, queues, got, float(want), R_loss))
    assert abs(got - float(want)) <= 2 * R_loss + 2.0 ** -20 * abs(float(want))
    # the validation pass calls the criterion under no_grad
    with torch.no_grad():
        torch.manual_seed(304)
        again = crit({k: v.detach() for k, v in preds.items()}, target, with_embed=True)
    assert float(crit.last_terms[0]) == got and bool(torch.isfinite(again))


def test_without_use_lovasz_the_criteria_are_unchanged():
    """use_lovasz false: the segmentation criterion is the cross-entropy one and the criterion's output is, bit for bit, the fused
    upsample + CE kernel's value plus the contrast term, as before."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import FSAuxCELoss, FSCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg, aux, embed, target = _criterion_inputs(dev)
    for loss_type, cls in (("mem_contrast_ce_loss", FSCELoss), ("mem_contrast_auxce_loss", FSAuxCELoss)):
        crit = SEG_LOSS_DICT[loss_type](_cfg(loss_type, 5, use_lovasz=False)).to(dev)
        assert type(crit.seg_criterion) is cls
        torch.manual_seed(304)
        total = crit({"seg": seg, "embed": embed, "seg_aux": aux}, target, with_embed=True)
        ce = K.upsample_ce(seg, target, None, -1)
        if cls is FSAuxCELoss:
            ce = 1.0 * ce + 0.4 * K.upsample_ce(aux, target, None, -1)
        assert torch.equal(crit.last_terms[0], ce)
        assert torch.equal(total, ce + 0.1 * crit.last_terms[1])


def test_refusals():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import FSCELOVASZLoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg = torch.randn(1, 4, 2, 2, device=dev)
    tgt = torch.zeros(1, 7, 7, dtype=torch.int64, device=dev)
    huge = torch.zeros(1, dtype=torch.int64, device=dev).expand(1, 1 << 16, 1 << 15)       # P = 2^31 without the memory
    for fn in (K.lovasz_softmax, K.lovasz_errors):
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            fn(seg, huge)
        with pytest.raises(RuntimeError, match="257 classes"):
            fn(torch.randn(1, 257, 2, 2, device=dev), tgt)
        with pytest.raises(RuntimeError, match="only upsampling"):
            fn(torch.randn(1, 4, 9, 9, device=dev), tgt)
        with pytest.raises(RuntimeError, match=r"\[B,K,h,w\] / \[B,H,W\]"):
            fn(seg, tgt[0])
    with pytest.raises(RuntimeError, match=r"expected \[K,P\]"):
        K.lovasz_order(torch.zeros(2, 9, device=dev), torch.zeros(2, 8, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match=r"expected \[K,P\]"):
        K.lovasz_grad(torch.zeros(2, 9, dtype=torch.uint8, device=dev), torch.zeros(9, dtype=torch.int32, device=dev),
                      torch.zeros(2, 9, device=dev))
    with pytest.raises(RuntimeError, match="float32"):
        K.lovasz_order(torch.zeros(2, 9, dtype=torch.float64, device=dev), torch.zeros(2, 9, dtype=torch.uint8, device=dev))
    with pytest.raises(NotImplementedError, match="use_lovasz"):
        SEG_LOSS_DICT["mem_contrast_ce_loss"](_cfg("mem_contrast_ce_loss", 4, use_rmi=True, num_classes=4, rmi_radius=3, rmi_pool_way=0,
                                                   rmi_pool_size=3, rmi_pool_stride=3, loss_weight_lambda=0.5, loss_weight=1.0,
                                                   lambda_way=1, use_sigmoid=False))
    for reduction in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="ce_reduction"):
            FSCELOVASZLoss(_cfg("mem_contrast_ce_loss", 4, ce_reduction=reduction))
    crit = FSCELOVASZLoss(_cfg("mem_contrast_ce_loss", 4)).to(dev)
    with pytest.raises(NotImplementedError, match="list / tuple"):
        crit([seg, seg], tgt)
    assert torch.equal(crit({"seg": seg}, tgt), crit(seg, tgt)) and crit.bad_label_count() == 0
    if dev.type == "cuda":
        with pytest.raises(RuntimeError, match="GPU"):
            K.lovasz_softmax(seg.cpu(), tgt.cpu())
        with pytest.raises(RuntimeError, match="GPU"):
            K.lovasz_errors(seg.cpu(), tgt.cpu())
