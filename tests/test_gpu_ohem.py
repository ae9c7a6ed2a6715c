"""Cross entropy with online hard example mining (csrc/ohem.hip: kernels.ohem_prob / ohem_threshold / ohem_reduce / ohem_ce,
loss_helper.FSOhemCELoss / FSAuxOhemCELoss, the registry keys fs_ohemce_loss / fs_auxohemce_loss) and the four contrast criteria with
contrast.use_ohem.

Yardsticks, never the code under test:
  (a) tests/golden/ohem_<case>.npz, made by tools/gen_ohem_golden.py from the reference's own FSOhemCELoss on F.interpolate(seg) on the
      CPU: loss, d loss / d seg, threshold and kept set in fp32 and in float64, and R_p, the deviation of the reference's fp32
      probabilities from float64.
  (b) `restate` below: the same term with torch ops in float64 (tests/test_ohem_host.py pins it to (a) at 1e-10); with `kept` it takes
      the given kept set instead of selecting one.
R = the deviation of the reference's (or, without a fixture, torch's) fp32 result from float64 on the case, for the quantity compared:
  prob       |p - p64| <= 2 R_p + 2^-24 and |nll - nll64| <= 2 R_nll + 2^-20 |nll64| at every valid pixel; the sentinel everywhere else
  threshold  thr bit-equal to max(torch.sort(p_valid)[min(k, n - 1)], fp32(thresh)) on the kernel's own p; k and n exact; with and
             without the shortcut
  reduce     kept == (p < thr).sum() exactly on the kernel's own p and thr; loss against the float64 sum over that set: 1e-6 relative
  parity     kept set equal to the reference's float64 one outside the undecided set {valid: |p64 - thr64| <= 16 R_p} (the kernel is
             allowed 2 R_p plus an ulp, the reference R_p, the rest is margin; the generator asserts that the set is empty on
             threshold-branch cases and exactly the rank-k pixel on k-th-branch cases); |loss - loss64| <= 2 R_loss + 2^-20 |loss64|;
             max |dseg - dseg64| <= 2 R_g + 2^-20 max |dseg64|
Replayed on the CPU emulation by tests/test_emu_ohem.py."""
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


# name: (B, K, h, w, H, W), amplitude, boost, ohem_thresh, ohem_minkeep, variant.
# seg = amp * randn + boost * onehot(label at the coarse grid); labels: 8 x 8 blocks, 10 % of the pixels ignored (-1) unless the variant
# says otherwise; ce_weight = 1 + 0.1 c.
CASES = {
    "tiny": ((1, 3, 3, 3, 5, 5), 3.0, 0.0, 0.7, 5, "no_ignore"),           # 25 pixels: less than one wave
    "thr": ((2, 5, 9, 11, 33, 41), 3.0, 0.0, 0.9, 10, None),               # threshold branch, nearly everything kept
    "multi": ((2, 5, 9, 11, 33, 41), 2.0, 4.0, 0.7, 1000, None),           # threshold branch (the shortcut)
    "multik": ((2, 5, 9, 11, 33, 41), 2.0, 4.0, 0.7, 1500, None),          # k-th branch
    "all": ((2, 5, 9, 11, 33, 41), 2.0, 4.0, 0.7, 10 ** 6, None),          # min_kept >= n: k = n - 1, all but the largest p kept
    "big": ((2, 4, 24, 20, 95, 77), 2.0, 6.0, 0.7, 6003, None),            # k-th branch, several blocks per pass
    "ident": ((2, 5, 32, 40, 32, 40), 2.0, 4.0, 0.7, 800, None),           # identity resize
    "k19": ((1, 19, 16, 32, 64, 128), 2.0, 6.0, 0.7, 3000, None),          # Cityscapes class count, threshold branch
    "k19k": ((1, 19, 16, 32, 64, 128), 2.0, 6.0, 0.7, 6007, None),         # the same, k-th branch
    "chunk": ((1, 37, 5, 6, 17, 21), 2.0, 5.0, 0.7, 100, None),            # 37 classes
    "sat": ((1, 4, 10, 10, 37, 37), 60.0, 0.0, 0.7, 300, None),            # p exactly 0 and exactly 1: ties in the lowest bin, nll finite
    "ties": ((2, 4, 32, 40, 32, 40), 4.0, 0.0, 0.7, 1900, "ties"),         # logits rounded to multiples of 2: the k-th lands in a tie group
    "narrow": ((2, 2, 32, 40, 32, 40), 0.0, 0.0, 0.3, 700, "narrow"),      # all keys share every digit but the last: the lowest level decides
    "void": ((2, 4, 6, 6, 21, 21), 3.0, 0.0, 0.7, 50, "void"),             # image 1 all ignored
    "void_all": ((2, 4, 6, 6, 21, 21), 3.0, 0.0, 0.7, 50, "void_all"),     # no valid pixel at all
    "confident": ((2, 4, 6, 6, 21, 21), 1.0, 50.0, 0.7, 1, "confident"),   # every p = 1: nothing is kept
}
FIXTURES = ("tiny", "thr", "multi", "multik", "all", "big", "ident", "k19", "k19k", "chunk", "sat")
KTH_BRANCH = ("multik", "all", "big", "k19k")


def inputs(name):
    """Seeded inputs of a case on the CPU: seg f32 [B,K,h,w], target i64 [B,H,W], ce_weight f32 [K]."""
    (B, K, h, w, H, W), amp, boost, _, _, variant = CASES[name]
    g = torch.Generator().manual_seed(304)
    seg = torch.randn(B, K, h, w, generator=g) * amp
    blocks = torch.randint(0, K, (B, (H + 7) // 8, (W + 7) // 8), generator=g)
    target = blocks.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)[:, :H, :W].contiguous()
    if variant == "confident":
        target = (torch.arange(B) % K)[:, None, None].expand(B, H, W).contiguous()      # one class per image: no soft boundary pixel
    if boost:
        ys = torch.linspace(0, H - 1, h).round().long()
        xs = torch.linspace(0, W - 1, w).round().long()
        seg = seg + boost * F.one_hot(target[:, ys][:, :, xs], K).permute(0, 3, 1, 2).float()
    if variant == "ties":
        seg = torch.round(seg / 2.0) * 2.0
    elif variant == "narrow":
        seg = torch.zeros(B, K, h, w)
        seg[:, 1] = torch.arange(B * h * w, dtype=torch.float32).reshape(B, h, w) * 1e-7
    if variant != "no_ignore":
        target[torch.rand(B, H, W, generator=g) < 0.10] = -1
    if variant == "void":
        target[1] = -1
    elif variant == "void_all":
        target[:] = -1
    return seg.contiguous(), target, 1.0 + 0.1 * torch.arange(K, dtype=torch.float32)


def restate(seg, target, weight, thresh, min_kept, kept=None, dtype=torch.float64):
    """FSOhemCELoss on F.interpolate(seg) restated with torch ops in `dtype`; `kept` (bool [B,H,W]) replaces the selection.
    -> dict(loss, p, nll, valid, kept, thr, k, n); loss is differentiable with respect to seg."""
    K = seg.shape[1]
    up = F.interpolate(seg.to(dtype), size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
    valid = (target >= 0) & (target < K)
    tc = target.clamp(0, K - 1).unsqueeze(1)
    p = F.softmax(up, dim=1).gather(1, tc).squeeze(1)
    nll = -F.log_softmax(up, dim=1).gather(1, tc).squeeze(1)
    n = int(valid.sum())
    k = max(min(max(1, int(min_kept)), n - 1), 0)
    thr = torch.tensor(float(np.float32(thresh)), dtype=dtype, device=seg.device)
    if kept is None:
        if n:
            thr = torch.maximum(torch.sort(p.detach()[valid]).values[k], thr)
        kept = valid & (p.detach() < thr)
    w = torch.ones(K, dtype=dtype, device=seg.device) if weight is None else weight.to(dtype)
    loss = (w[tc.squeeze(1)] * nll)[kept].sum() / kept.sum()
    return dict(loss=loss, p=p.detach(), nll=nll.detach(), valid=valid, kept=kept, thr=thr, k=k, n=n)


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Inputs, the golden file (None without one), the float64 restatement and R_p, R_nll of one case, computed once and shared."""
    dev = torch.device(dev_str)
    seg, target, weight = inputs(name)
    _, _, _, thresh, min_kept, _ = CASES[name]
    with torch.no_grad():
        r32 = restate(seg, target, weight, thresh, min_kept, dtype=torch.float32)
        r64c = restate(seg, target, weight, thresh, min_kept)
    v = r64c["valid"]
    R_p = float((r32["p"].double() - r64c["p"])[v].abs().max()) if bool(v.any()) else 0.0
    R_nll = float((r32["nll"].double() - r64c["nll"])[v].abs().max()) if bool(v.any()) else 0.0
    gold = None
    if name in FIXTURES:
        gold = dict(np.load(os.path.join(GOLDEN, "ohem_%s.npz" % name)))
        assert np.array_equal(gold["target"].astype(np.int64), target.numpy()), "the fixture was made from other labels"
        assert abs(float(seg.double().sum()) - float(gold["seg_sum"])) <= 1e-6, "the fixture was made from other logits"
        R_p = float(gold["R_p"])
    r64 = {k_: (t.to(dev) if torch.is_tensor(t) else t) for k_, t in r64c.items()}
    return seg.to(dev), target.to(dev), weight.to(dev), gold, r64, R_p, R_nll


def _R(gold):
    R_loss = abs(float(gold["loss32"]) - float(gold["loss64"]))
    R_g = float(np.abs(gold["dseg32"].astype(np.float64) - gold["dseg64"]).max())
    return R_loss, R_g


def _undecided(r64, R_p):
    return r64["valid"] & ((r64["p"] - r64["thr"]).abs() <= 16 * R_p)


def _run(seg, target, weight, thresh, min_kept, **kw):
    from contrastiveseg_amd import kernels as K
    x = seg.clone().requires_grad_(True)
    before = target.clone()
    loss, out = K.ohem_ce(x, target, weight, -1, thresh, min_kept, want_terms=True, **kw)
    loss.backward()
    assert torch.equal(target, before), "the label tensor was modified"
    return loss.detach(), out, x.grad


# ---- stage 1: probabilities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_prob_matches_float64(case):
    from contrastiveseg_amd import kernels as K
    seg, target, _, _, r64, R_p, R_nll = _case(case, str(_dev()))
    p, nll, lse = K.ohem_prob(seg, target)
    assert p.shape == nll.shape == lse.shape == target.shape and p.dtype == nll.dtype == lse.dtype == torch.float32
    v = r64["valid"]
    assert bool((p[~v] == K.OHEM_SENTINEL).all()) and bool((nll[~v] == 0).all()), "invalid pixels carry the sentinel"
    assert bool(torch.isfinite(lse).all())
    if not bool(v.any()):
        return
    perr = float((p.double() - r64["p"])[v].abs().max())
    nerr = (nll.double() - r64["nll"])[v].abs()
    nbound = 2 * R_nll + 2.0 ** -20 * r64["nll"][v].abs()
    print("%s: R_p %.3e  p vs float64 %.3e  bound %.3e;  R_nll %.3e  nll vs float64 %.3e" % (
        case, R_p, perr, 2 * R_p + 2.0 ** -24, R_nll, float(nerr.max())))
    assert perr <= 2 * R_p + 2.0 ** -24, (case, perr, R_p)
    assert bool((nerr <= nbound).all()), (case, float((nerr - nbound).max()))
    assert float(p[v].min()) >= 0.0 and float(p[v].max()) <= 1.0
    if case == "sat":
        assert bool((p[v] == 0.0).any()) and bool((p[v] == 1.0).any()), "the case is there for p exactly 0 and exactly 1"
        assert bool(torch.isfinite(nll).all()) and float(nll[v & (p == 0.0)].min()) > 10.0, "nll is not -log p"


def test_bad_labels_are_dropped_and_counted():
    from contrastiveseg_amd import kernels as K
    seg, target, weight, _, r64, _, _ = _case("multi", str(_dev()))
    K_ = seg.shape[1]
    planted = target.clone()
    where = torch.nonzero(r64["valid"])[[5, 700, 1900]]
    for i, (b, y, x) in enumerate(where.tolist()):
        planted[b, y, x] = K_ if i < 2 else -7
    status = torch.zeros(4, dtype=torch.int32, device=seg.device)
    p, nll, _ = K.ohem_prob(seg, planted, status=status)
    assert int(status[1]) == 3
    assert all(float(p[b, y, x]) == K.OHEM_SENTINEL and float(nll[b, y, x]) == 0.0 for b, y, x in where.tolist())
    # the fused route counts them once per call, in the sticky word, and the term is the one of the labels with those pixels ignored
    loss, out = K.ohem_ce(seg, planted, weight, -1, 0.7, 1000, status=status, want_terms=True)
    ignored = planted.clone()
    ignored[(planted == K_) | (planted == -7)] = -1
    assert int(status[1]) == 6 and torch.equal(loss, K.ohem_ce(seg, ignored, weight, -1, 0.7, 1000))
    assert int(out[3]) == r64["n"] - 3
    # with another ignore index the -1 labels are bad labels too
    status.zero_()
    K.ohem_prob(seg, target, ignore_index=255, status=status)
    assert int(status[1]) == int((target == -1).sum())


# ---- stage 2: threshold -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shortcut", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_threshold_is_the_order_statistic_of_the_stored_p(case, shortcut):
    from contrastiveseg_amd import kernels as K
    seg, target, _, _, r64, _, _ = _case(case, str(_dev()))
    _, _, _, thresh, min_kept, _ = CASES[case]
    p, _, _ = K.ohem_prob(seg, target)
    thr, k, n = K.ohem_threshold(p, thresh, min_kept, shortcut=shortcut)
    assert thr.dtype == torch.float32 and k.dtype == n.dtype == torch.int32
    pv = p[p <= 1.0]
    assert int(n) == pv.numel() == r64["n"] and int(k) == r64["k"]
    want = torch.tensor(thresh, dtype=torch.float32, device=p.device)
    branch = "thresh"
    if pv.numel():
        kth = torch.sort(pv).values[int(k)]
        branch = "k-th" if float(kth) > float(want) else "thresh"
        want = torch.maximum(kth, want)
    print("%s shortcut=%s: n %d k %d thr %.9g (%s branch)" % (case, shortcut, int(n), int(k), float(thr), branch))
    assert thr.view(torch.int32).item() == want.view(torch.int32).item(), (case, float(thr), float(want))
    if case in KTH_BRANCH + ("ties", "narrow"):
        assert branch == "k-th", "the case is there for the k-th branch"
    if case in ("ties", "narrow"):
        assert int((pv == thr).sum()) >= 2, "the case is there for a k-th probability inside a tie group"
    if case == "narrow":
        keys = pv.view(torch.int32)
        assert int(((keys >> 10) == (thr.view(torch.int32) >> 10)).sum()) >= 100, "the lowest level decides among many candidates"


def test_threshold_of_crafted_keys():
    """Keys chosen to meet every level of the select: the rank-k key is found whatever digit it differs in."""
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    bits = torch.tensor([0x3F000000, 0x3F000001, 0x3F0003FF, 0x3F000400, 0x3F0FFC00, 0x3F100000, 0x3F800000, 0, 1, 0x00800000],
                        dtype=torch.int32)
    p = bits.view(torch.float32).repeat(3).to(dev)              # every key three times: ranks 3r .. 3r + 2 hold the r-th smallest
    p = torch.cat([p, torch.full((7,), float(K.OHEM_SENTINEL), device=dev)])
    order = torch.sort(p[:30]).values
    for k in (1, 2, 3, 8, 14, 15, 22, 27, 29, 500):
        for shortcut in (True, False):
            thr, kk, n = K.ohem_threshold(p, 0.0, k, shortcut=shortcut)
            assert int(n) == 30 and int(kk) == min(k, 29)
            assert thr.view(torch.int32).item() == order[min(k, 29)].view(torch.int32).item(), k


# ---- stage 3: reduce --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_reduce_over_the_stored_p(case):
    from contrastiveseg_amd import kernels as K
    seg, target, weight, _, r64, _, _ = _case(case, str(_dev()))
    _, _, _, thresh, min_kept, _ = CASES[case]
    p, nll, _ = K.ohem_prob(seg, target)
    thr, _, _ = K.ohem_threshold(p, thresh, min_kept)
    out, outi = K.ohem_reduce(p, nll, target, thr, weight)
    kept = p < thr
    assert int(outi[0]) == int(kept.sum()) and float(out[1]) == float(kept.sum()) and float(out[2]) == float(thr)
    if int(kept.sum()) == 0:
        assert bool(torch.isnan(out[0]))
        return
    want = float((weight.double()[target.clamp(0, seg.shape[1] - 1)] * nll.double())[kept].sum() / kept.sum())
    print("%s: kept %d  loss %.9g  float64 over the same set %.9g" % (case, int(kept.sum()), float(out[0]), want))
    assert abs(float(out[0]) - want) <= 1e-6 * abs(want)
    # the fused route selects from the level-0 histogram of the probability pass: same threshold, same set, same loss
    loss, fused = K.ohem_ce(seg, target, weight, -1, thresh, min_kept, want_terms=True)
    assert torch.equal(fused[:3], out[:3]) and torch.equal(loss, out[0]) and int(fused[3]) == r64["n"]


# ---- the fused route against the reference -------------------------------------------------------------------------------------------------
def _check_against(case, loss, out, grad, want_loss, want_grad, R_loss, R_g):
    err = abs(float(loss) - want_loss)
    gerr = float((grad.double() - want_grad).abs().max())
    gmax = float(want_grad.abs().max())
    print("%s: loss %.9g  float64 %.9g  R_loss %.3e  err %.3e  bound %.3e;  R_g %.3e  d seg err %.3e  bound %.3e  kept %d  thr %.9g" % (
        case, float(loss), want_loss, R_loss, err, 2 * R_loss + 2.0 ** -20 * abs(want_loss), R_g, gerr, 2 * R_g + 2.0 ** -20 * gmax,
        int(out[1]), float(out[2])))
    assert err <= 2 * R_loss + 2.0 ** -20 * abs(want_loss), (case, err, R_loss)
    assert bool(torch.isfinite(grad).all())
    assert gerr <= 2 * R_g + 2.0 ** -20 * gmax, (case, gerr, R_g, gmax)


def _kernel_kept(seg, target, out):
    from contrastiveseg_amd import kernels as K
    p, _, _ = K.ohem_prob(seg, target)
    return p < out[2]


@pytest.mark.parametrize("case", list(FIXTURES))
def test_loss_gradient_and_kept_set_match_the_reference(case):
    seg, target, weight, gold, r64, R_p, _ = _case(case, str(_dev()))
    _, _, _, thresh, min_kept, _ = CASES[case]
    loss, out, grad = _run(seg, target, weight, thresh, min_kept)
    kept64 = torch.from_numpy(np.unpackbits(gold["kept64"])[:target.numel()].astype(bool)).reshape(target.shape).to(seg.device)
    und = _undecided(r64, R_p)
    kept = _kernel_kept(seg, target, out)
    assert int(und.sum()) == (1 if case in KTH_BRANCH else 0)
    assert torch.equal(kept[~und], kept64[~und]), (case, int((kept != kept64).sum()))
    assert int(out[3]) == r64["n"] and abs(float(out[2]) - float(gold["thr64"])) <= 2 * R_p + 2.0 ** -24
    R_loss, R_g = _R(gold)
    _check_against(case, loss, out, grad, float(gold["loss64"]), torch.from_numpy(gold["dseg64"]).to(seg.device), R_loss, R_g)


@pytest.mark.parametrize("case", ["ties", "narrow", "multi_noweights"])
def test_cases_without_a_fixture_against_float64_with_the_kernels_kept_set(case):
    """ties / narrow: float64 cannot rank probabilities that are equal in fp32, so loss and gradient are compared with the restatement
    evaluated on the kernel's own kept set, which may differ from float64's only inside the undecided set. multi without class weights."""
    name = "multi" if case == "multi_noweights" else case
    seg, target, weight, _, r64, R_p, _ = _case(name, str(_dev()))
    _, _, _, thresh, min_kept, _ = CASES[name]
    if case == "multi_noweights":
        weight = None
    loss, out, grad = _run(seg, target, weight, thresh, min_kept)
    kept = _kernel_kept(seg, target, out)
    und = _undecided(r64, R_p)
    assert torch.equal(kept[~und], r64["kept"][~und]) and int(kept.sum()) == int(out[1]) > 0
    if case != "multi_noweights":
        assert int(und.sum()) >= 2
    x64 = seg.double().requires_grad_(True)
    want = restate(x64, target, weight, thresh, min_kept, kept=kept)
    want["loss"].backward()
    x32 = seg.clone().requires_grad_(True)
    r32 = restate(x32, target, weight, thresh, min_kept, kept=kept, dtype=torch.float32)
    r32["loss"].backward()
    R_loss = abs(float(r32["loss"].detach()) - float(want["loss"].detach()))
    R_g = float((x32.grad.double() - x64.grad).abs().max())
    _check_against(case, loss, out, grad, float(want["loss"].detach()), x64.grad, R_loss, R_g)


# ---- determinism, empty selections, refusals --------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    seg, target, weight, _, _, _, _ = _case("big", str(_dev()))
    a, b = _run(seg, target, weight, 0.7, 6003), _run(seg, target, weight, 0.7, 6003)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    with torch.no_grad():
        assert torch.equal(K.ohem_ce(seg, target, weight, -1, 0.7, 6003), a[0])


def test_void_images_and_empty_selections():
    """Image 1 all ignored: the numbers of image 0 alone. No valid pixel, or every valid pixel confident: the loss is NaN (the reference's
    value for the empty selection; without a valid pixel it raises instead) and the gradient is all zeros, finite."""
    seg, target, weight, _, r64, _, _ = _case("void", str(_dev()))
    loss, out, grad = _run(seg, target, weight, 0.7, 50)
    alone = _run(seg[:1].contiguous(), target[:1].contiguous(), weight, 0.7, 50)
    assert torch.equal(loss, alone[0]) and torch.equal(grad[:1], alone[2]) and float(grad[1].abs().max()) == 0.0
    assert abs(float(loss) - float(r64["loss"])) <= 1e-5 * float(r64["loss"]) and float(grad[0].abs().max()) > 0
    for name in ("void_all", "confident"):
        seg, target, weight, _, r64, _, _ = _case(name, str(_dev()))
        _, _, _, thresh, min_kept, _ = CASES[name]
        loss, out, grad = _run(seg, target, weight, thresh, min_kept)
        assert bool(torch.isnan(loss)) and float(out[1]) == 0.0 and int(out[3]) == r64["n"], name
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) == 0.0, name
        assert (r64["n"] == 0) == (name == "void_all") and int(r64["kept"].sum()) == 0


def _cfg(loss_type, K_, use_ohem=True, use_rmi=False, use_lovasz=False, with_memory=None, **params):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    p = {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean", "ohem_thresh": 0.7, "ohem_minkeep": 1000}
    p.update(params)
    p = {k_: v for k_, v in p.items() if v is not None}
    contrast = dict(proj_dim=16, temperature=0.1, base_temperature=0.07, max_samples=64, max_views=4, loss_weight=0.1, use_rmi=use_rmi,
                    use_lovasz=use_lovasz, warmup_iters=0)
    if use_ohem is not None:
        contrast["use_ohem"] = use_ohem
    if loss_type.startswith("mem_") if with_memory is None else with_memory:
        contrast.update(with_memory=True, memory_size=8, pixel_update_freq=2)
    return Configer(config_dict={
        "data": {"num_classes": K_}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": 4},
        "contrast": contrast, "loss": {"loss_type": loss_type, "params": p}})


def test_refusals():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import FSOhemCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg = torch.randn(1, 4, 2, 2, device=dev)
    tgt = torch.zeros(1, 7, 7, dtype=torch.int64, device=dev)
    huge = torch.zeros(1, dtype=torch.int64, device=dev).expand(1, 1 << 16, 1 << 15)       # P = 2^31 without the memory
    for fn in (K.ohem_ce, K.ohem_prob):
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            fn(seg, huge)
        with pytest.raises(RuntimeError, match="only upsampling"):
            fn(torch.randn(1, 4, 9, 9, device=dev), tgt)
        with pytest.raises(RuntimeError, match=r"\[B,K,h,w\] / \[B,H,W\]"):
            fn(seg, tgt[0])
    with pytest.raises(RuntimeError, match="share one coarse tap"):
        K.ohem_ce(seg, torch.zeros(1, 7, 40, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="float32"):
        K.ohem_threshold(torch.zeros(9, dtype=torch.float64, device=dev), 0.7, 1)
    for reduction in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="ce_reduction"):
            FSOhemCELoss(_cfg("fs_ohemce_loss", 4, ce_reduction=reduction))
    for key in ("ohem_thresh", "ohem_minkeep"):
        with pytest.raises(KeyError, match=key):
            FSOhemCELoss(_cfg("fs_ohemce_loss", 4, **{key: None}))
    rmi = dict(num_classes=4, rmi_radius=3, rmi_pool_way=0, rmi_pool_size=3, rmi_pool_stride=3, loss_weight_lambda=0.5, loss_weight=1.0,
               lambda_way=1, use_sigmoid=False)
    for loss_type in ("contrast_ce_loss", "contrast_auxce_loss", "mem_contrast_ce_loss", "mem_contrast_auxce_loss"):
        with pytest.raises(NotImplementedError, match="use_ohem together with contrast.use_rmi"):
            SEG_LOSS_DICT[loss_type](_cfg(loss_type, 4, use_rmi=True, **rmi))
    for loss_type in ("mem_contrast_ce_loss", "mem_contrast_auxce_loss"):
        with pytest.raises(NotImplementedError, match="use_ohem together with contrast.use_lovasz"):
            SEG_LOSS_DICT[loss_type](_cfg(loss_type, 4, use_lovasz=True))
    crit = FSOhemCELoss(_cfg("fs_ohemce_loss", 4, ohem_minkeep=0)).to(dev)
    assert crit.min_kept == 1 and crit.thresh == 0.7
    assert torch.equal(crit({"seg": seg}, tgt), crit(seg, tgt)) and crit.bad_label_count() == 0
    if dev.type == "cuda":
        with pytest.raises(RuntimeError, match="GPU"):
            K.ohem_ce(seg.cpu(), tgt.cpu())
        with pytest.raises(RuntimeError, match="GPU"):
            K.ohem_prob(seg.cpu(), tgt.cpu())


def test_no_host_synchronisation():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    seg, target, weight, _, _, _, _ = _case("multik", str(_dev()))
    crit = SEG_LOSS_DICT["contrast_ce_loss"](_cfg("contrast_ce_loss", seg.shape[1], ohem_minkeep=1500)).to(seg.device)

    def both():
        x = seg.clone().requires_grad_(True)
        K.ohem_ce(x, target, weight, -1, 0.7, 1500).backward()
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
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all()) and float(gx.abs().max()) > 0


# ---- the criteria ---------------------------------------------------------------------------------------------------------------------------
def _criterion_inputs(dev):
    seg, target, _ = inputs("multi")
    g = torch.Generator().manual_seed(305)
    B, K_, h, w = seg.shape
    aux = torch.randn(B, K_, h, w, generator=g) * 2
    embed = F.normalize(torch.randn(B, 16, h, w, generator=g), dim=1)
    return seg.to(dev), aux.to(dev), embed.to(dev), target.to(dev)


def test_registered_criteria():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import bad_label_total
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg, aux, _, target = _criterion_inputs(dev)
    w = [1.0 + 0.1 * c for c in range(5)]
    wt = torch.tensor(w, device=dev)
    crit = SEG_LOSS_DICT["fs_ohemce_loss"](_cfg("fs_ohemce_loss", 5, ce_weight=w)).to(dev)
    x = seg.clone().requires_grad_(True)
    crit(x, target).backward()
    y = seg.clone().requires_grad_(True)
    want = K.ohem_ce(y, target, wt, -1, 0.7, 1000)
    want.backward()
    assert torch.equal(crit(seg, target), want.detach()) and torch.equal(x.grad, y.grad) and float(x.grad.abs().max()) > 0
    auxc = SEG_LOSS_DICT["fs_auxohemce_loss"](_cfg("fs_auxohemce_loss", 5, ce_weight=w)).to(dev)
    got = auxc([aux, seg], target)
    assert torch.equal(got, 1.0 * K.ohem_ce(seg, target, wt, -1, 0.7, 1000) + 0.4 * K.upsample_ce(aux, target, wt, -1))
    bad = target.clone()
    bad[0, 0, 0] = 5
    auxc([aux, seg], bad)
    assert int(bad_label_total(auxc)) == 2, "the OHEM part and the CE part each count the label"


@pytest.mark.parametrize("loss_type", ["contrast_ce_loss", "contrast_auxce_loss", "mem_contrast_ce_loss", "mem_contrast_auxce_loss"])
def test_contrast_criteria_with_use_ohem(loss_type):
    from contrastiveseg_amd.lib.loss.loss_helper import FSAuxOhemCELoss, FSOhemCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg, aux, embed, target = _criterion_inputs(dev)
    has_aux = "aux" in loss_type
    crit = SEG_LOSS_DICT[loss_type](_cfg(loss_type, 5)).to(dev)
    assert type(crit.seg_criterion) is (FSAuxOhemCELoss if has_aux else FSOhemCELoss)
    preds = {"seg": seg.clone().requires_grad_(True), "embed": embed.clone().requires_grad_(True)}
    if has_aux:
        preds["seg_aux"] = aux.clone().requires_grad_(True)
    torch.manual_seed(304)
    total = crit(preds, target, with_embed=True)          # (the memory pair without queues: the segmentation term alone)
    total.backward()
    alone = SEG_LOSS_DICT["fs_auxohemce_loss" if has_aux else "fs_ohemce_loss"](_cfg(loss_type, 5)).to(dev)
    want = alone([aux, seg] if has_aux else seg, target)
    assert torch.equal(crit.last_terms[0], want) and bool(torch.isfinite(total.detach()))
    assert bool(torch.isfinite(preds["seg"].grad).all()) and float(preds["seg"].grad.abs().max()) > 0
    with torch.no_grad():                                  # the validation pass calls the criterion under no_grad
        torch.manual_seed(304)
        crit({k_: v.detach() for k_, v in preds.items()}, target, with_embed=True)
    assert torch.equal(crit.last_terms[0], want)


@pytest.mark.parametrize("loss_type", ["contrast_ce_loss", "contrast_auxce_loss", "mem_contrast_ce_loss", "mem_contrast_auxce_loss"])
def test_without_use_ohem_the_criteria_are_unchanged(loss_type):
    """use_ohem absent or false: the segmentation criterion is the cross-entropy one, and its value and gradient are, bit for bit, those
    of the fused upsample + CE kernel."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import FSAuxCELoss, FSCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg, aux, embed, target = _criterion_inputs(dev)
    has_aux = "aux" in loss_type
    for use_ohem in (None, False):
        crit = SEG_LOSS_DICT[loss_type](_cfg(loss_type, 5, use_ohem=use_ohem, ohem_thresh=None, ohem_minkeep=None)).to(dev)
        assert type(crit.seg_criterion) is (FSAuxCELoss if has_aux else FSCELoss) and crit.use_ohem is False
        x, a = seg.clone().requires_grad_(True), aux.clone().requires_grad_(True)
        torch.manual_seed(304)
        total = crit({"seg": x, "embed": embed, "seg_aux": a}, target, with_embed=True)
        total.backward()
        y, b = seg.clone().requires_grad_(True), aux.clone().requires_grad_(True)
        ce = K.upsample_ce(y, target, None, -1)
        if has_aux:
            ce = 1.0 * ce + 0.4 * K.upsample_ce(b, target, None, -1)
        ce.backward()
        assert torch.equal(crit.last_terms[0], ce.detach()) and torch.equal(total.detach(), ce.detach() + 0.1 * crit.last_terms[1])
        assert torch.equal(x.grad, y.grad) and (not has_aux or torch.equal(a.grad, b.grad))
