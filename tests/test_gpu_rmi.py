"""The region mutual information segmentation term (csrc/rmi.hip: kernels.rmi_pool / rmi_cov / rmi_solve / rmi_loss, lib/loss/rmi_loss.py)
and the contrast criteria with contrast.use_rmi.

Yardsticks, never the code under test:
  (a) tests/golden/rmi_<case>.npz, made by tools/gen_rmi_golden.py from the reference's own RMILoss on the CPU: loss and d loss / d seg
      in fp32 and in float64, and R_p, the deviation of the reference's fp32 pooled probabilities from float64.
  (b) `restate` below: RMILoss.forward_sigmoid -> rmi_lower_bound of the reference (lib/loss/rmi_loss.py:283-402) with torch ops in
      float64; with `route` it pools by gather instead of max_pool2d. tests/test_rmi_host.py pins (b) to (a) at 1e-10.
R = the largest deviation of the reference's fp32 result from float64 on the case, for the quantity compared (the form and floor of
tests/test_gpu_ms_eval.py):
  pooled probabilities   |p_pool - p64| <= 2 R_p + 2^-20
  route                  the float64 probability of the chosen slot is within 4 R_p of the window's float64 maximum; equal to the float64
                         argmax where the float64 top-two margin exceeds 4 R_p; on every case but `sat` at most 1 % of the windows differ
  loss                   <= 2 R_loss + 2^-20 |loss|
  d seg                  against (b) evaluated with the kernel's route: <= 2 R_g + 2^-20 max|g64| (the kernel rounds at other points than
                         torch, not more often; with the route fixed the gradient is smooth, without it one flipped near-tie moves a
                         quarter of a window's gradient between coarse cells); on `sat` additionally everything is finite
  solve                  against the reference formula in torch CPU float64 autograd (torch.inverse, Cholesky with + 1e-8); D = the largest
                         change of that yardstick under four seeded relative perturbations of size 2^-50 of Cl, Cp, Clp; the kernel is
                         within 8 D + 2^-44 max|.| (the 8: a Cholesky-based inverse against LU)
  covariances            against the centred float64 product of the same pooled maps: <= 8 M^2 2^-53 (worst case of a recursive sum of
                         M terms of magnitude <= 1, for both sides and the centring; M = number of points)
Replayed on the CPU emulation by tests/test_emu_rmi.py."""
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


# name: (B, K, h, w, H, W), amplitude, variant, (lambda, lambda_way, loss_weight)
CASES = {
    "odd": ((2, 5, 10, 13, 37, 50), 3.0, None, (0.5, 1, 1.0)),
    "city": ((1, 19, 16, 32, 64, 128), 3.0, None, (0.5, 1, 1.0)),
    "k171": ((1, 171, 9, 11, 33, 41), 3.0, None, (0.5, 1, 1.0)),
    "ident": ((1, 4, 21, 24, 21, 24), 3.0, None, (0.5, 1, 1.0)),
    "d8": ((1, 19, 9, 17, 65, 129), 3.0, None, (0.5, 1, 1.0)),
    "min9": ((2, 3, 3, 3, 9, 9), 3.0, None, (0.5, 1, 1.0)),
    "min7": ((1, 4, 2, 2, 7, 7), 3.0, None, (0.5, 1, 1.0)),
    "sat": ((1, 5, 10, 13, 37, 50), 40.0, None, (0.5, 1, 1.0)),
    "ign": ((2, 5, 10, 13, 37, 50), 3.0, "all_ignored", (0.5, 1, 1.0)),        # image 1 all-ignored: V = 0 for it
    "big": ((2, 5, 10, 13, 37, 50), 3.0, "label_ge_K", (0.5, 1, 1.0)),         # some labels >= K
    "way0": ((2, 5, 10, 13, 37, 50), 3.0, None, (0.3, 0, 0.5)),                # lambda_way 0, loss_weight 0.5
}


def inputs(name):
    """Seeded inputs of a case on the CPU: seg f32 [B,K,h,w], target i64 [B,H,W]."""
    (B, K, h, w, H, W), amp, variant, _ = CASES[name]
    g = torch.Generator().manual_seed(304)
    seg = torch.randn(B, K, h, w, generator=g) * amp
    blocks = torch.randint(0, K, (B, (H + 7) // 8, (W + 7) // 8), generator=g)
    target = blocks.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)[:, :H, :W].contiguous()
    target[torch.rand(B, H, W, generator=g) < 0.05] = -1
    target[0][target[0] == 1] = 2                     # one class absent from image 0
    if variant == "all_ignored":
        target[1] = -1
    elif variant == "label_ge_K":
        target[torch.rand(B, H, W, generator=g) < 0.03] = K + 3
    return seg, target


def windows(p):
    """[B,K,H,W] -> the 3 x 3 / stride 3 / padding 1 windows [B,K,hp,wp,9] in row-major slot order, padding = -inf."""
    B, K, H, W = p.shape
    hp, wp = (H - 1) // 3 + 1, (W - 1) // 3 + 1
    pad = F.pad(p, (1, 3 * wp - W - 1, 1, 3 * hp - H - 1), value=float("-inf"))
    return pad.reshape(B, K, hp, 3, wp, 3).permute(0, 1, 2, 4, 3, 5).reshape(B, K, hp, wp, 9)


def rmi_from_cov(la_cov, pr_cov, la_pr_cov):
    """rmi_loss.py:374-390 on float64 CPU matrices [..., 9, 9] -> rmi [...]."""
    eye = torch.eye(9, dtype=pr_cov.dtype)
    pr_cov_inv = torch.inverse(pr_cov + eye * 1e-3)
    appro_var = la_cov - torch.matmul(la_pr_cov.matmul(pr_cov_inv), la_pr_cov.transpose(-2, -1))
    chol = torch.linalg.cholesky(appro_var + eye * 1e-3)
    return 0.5 * 2.0 * torch.sum(torch.log(torch.diagonal(chol, dim1=-2, dim2=-1) + 1e-8), dim=-1)


def restate(seg, target, lam, lambda_way, loss_weight, route=None, dtype=torch.float64):
    """The reference's RMI term on F.interpolate(seg) restated with torch ops in `dtype` (the 9 x 9 algebra on the CPU). With `route`
    (u8 [B,K,hp,wp]) the probabilities are pooled by gathering that slot of every window instead of max_pool2d.
    -> dict(loss, bce, rmi, V, p_pool, l_pool, win) -- loss is differentiable with respect to seg."""
    B, K = seg.shape[:2]
    H, W = target.shape[-2:]
    x = F.interpolate(seg.to(dtype), size=(H, W), mode="bilinear", align_corners=True)
    valid = (target >= 0) & (target < K)
    onehot = F.one_hot(target * valid, K).permute(0, 3, 1, 2).to(dtype) * valid[:, None].to(dtype)
    V = valid.sum().to(dtype)
    bce = (F.binary_cross_entropy_with_logits(x, onehot, reduction="none") * valid[:, None].to(dtype)).sum() / (V + 1.0)
    p = torch.sigmoid(x) * valid[:, None].to(dtype) + 1e-6
    win = windows(p)
    if route is None:
        p_pool = F.max_pool2d(p, kernel_size=3, stride=3, padding=1)
    else:
        p_pool = win.gather(4, route.long()[..., None])[..., 0]
    l_pool = F.max_pool2d(onehot, kernel_size=3, stride=3, padding=1)
    hp, wp = p_pool.shape[-2:]
    nh, nw = hp - 2, wp - 2
    la = torch.stack([l_pool[:, :, y:y + nh, x_:x_ + nw] for y in range(3) for x_ in range(3)], dim=2).reshape(B, K, 9, -1).double()
    pr = torch.stack([p_pool[:, :, y:y + nh, x_:x_ + nw] for y in range(3) for x_ in range(3)], dim=2).reshape(B, K, 9, -1).double()
    la = la - la.mean(dim=3, keepdim=True)
    pr = pr - pr.mean(dim=3, keepdim=True)
    la_cov = torch.matmul(la, la.transpose(2, 3)).cpu()
    pr_cov = torch.matmul(pr, pr.transpose(2, 3)).cpu()
    la_pr_cov = torch.matmul(la, pr.transpose(2, 3)).cpu()
    rmi_now = rmi_from_cov(la_cov, pr_cov, la_pr_cov)
    rmi = (rmi_now.reshape(-1, K).mean(dim=0) / 9.0).sum().to(seg.device)
    final = lam * bce + (1.0 - lam) * rmi if lambda_way else bce + lam * rmi
    return dict(loss=loss_weight * final, bce=bce, rmi=rmi, V=V, p_pool=p_pool, l_pool=l_pool, win=win,
                cov=torch.stack([la_cov, pr_cov, la_pr_cov], dim=2))


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Inputs, the golden file and the free-route float64 restatement of one case, computed once and shared (never modified)."""
    dev = torch.device(dev_str)
    seg, target = inputs(name)
    seg, target = seg.to(dev), target.to(dev)
    gold = dict(np.load(os.path.join(GOLDEN, "rmi_%s.npz" % name)))
    assert np.array_equal(gold["target"].astype(np.int64), target.cpu().numpy()), "the fixture was made from other labels"
    assert abs(float(seg.double().sum()) - float(gold["seg_sum"])) <= 1e-6, "the fixture was made from other logits"
    lam, way, lw = CASES[name][3]
    with torch.no_grad():
        r64 = restate(seg, target, lam, way, lw)
    return seg, target, gold, r64


def _R(gold):
    R_p = float(gold["R_p"])
    R_loss = abs(float(gold["loss32"]) - float(gold["loss64"]))
    R_g = float(np.abs(gold["dseg32"].astype(np.float64) - gold["dseg64"]).max())
    return R_p, R_loss, R_g


@pytest.mark.parametrize("case", list(CASES))
def test_pooled_maps_and_route_match_float64(case):
    from contrastiveseg_amd import kernels as K
    seg, target, gold, r64 = _case(case, str(_dev()))
    R_p, _, _ = _R(gold)
    p_pool, route, l_pool, partial = K.rmi_pool(seg, target)
    B, K_ = seg.shape[:2]
    hp, wp = K.rmi_pooled_size(*target.shape[-2:])
    assert p_pool.shape == route.shape == l_pool.shape == (B, K_, hp, wp)
    assert p_pool.dtype == torch.float32 and route.dtype == torch.uint8 and l_pool.dtype == torch.uint8
    err = float((p_pool.double() - r64["p_pool"]).abs().max())
    print("%s: R_p %.3e  p_pool vs float64 %.3e  bound %.3e" % (case, R_p, err, 2 * R_p + 2.0 ** -20))
    assert err <= 2 * R_p + 2.0 ** -20, (case, err, R_p)
    assert torch.equal(l_pool.double(), r64["l_pool"])
    # valid pixels: exact; BCE sum against float64
    valid = (target >= 0) & (target < K_)
    sums = partial.sum(dim=0)
    assert float(sums[1]) == float(valid.sum())
    bce = float(sums[0]) / (float(sums[1]) + 1.0)
    assert abs(bce - float(r64["bce"])) <= 2 * _R(gold)[1] + 2.0 ** -20 * abs(float(r64["bce"])) + 2.0 ** -20
    # route
    win = r64["win"]
    assert int(route.max()) <= 8
    chosen = win.gather(4, route.long()[..., None])[..., 0]
    top = win.topk(2, dim=4)
    assert bool(torch.isfinite(chosen).all()), "padding won a window"
    gap = float((top.values[..., 0] - chosen).max())
    margin = top.values[..., 0] - top.values[..., 1]
    clear = margin > 4 * R_p
    differ = float((route.long() != win.argmax(dim=4)).double().mean())
    print("%s: chosen slot below the float64 maximum by at most %.3e (4 R_p = %.3e); %.4f %% of the windows within 4 R_p of a tie; "
          "%.4f %% differ from the float64 argmax" % (case, gap, 4 * R_p, 100 * (1 - float(clear.double().mean())), 100 * differ))
    assert gap <= 4 * R_p, (case, gap, R_p)
    assert bool((route.long()[clear] == top.indices[..., 0][clear]).all()), case
    if case != "sat":
        assert differ <= 0.01, (case, differ)


@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_gradient_match_the_reference(case):
    from contrastiveseg_amd import kernels as K
    seg, target, gold, r64 = _case(case, str(_dev()))
    _, R_loss, R_g = _R(gold)
    lam, way, lw = CASES[case][3]
    x = seg.clone().requires_grad_(True)
    before = target.clone()
    loss, parts = K.rmi_loss(x, target, lam, way, lw, want_terms=True)
    loss.backward()
    assert torch.equal(target, before), "the label tensor was modified"
    want = float(gold["loss64"])
    err = abs(float(loss.detach()) - want)
    print("%s: loss %.9g  float64 %.9g  R_loss %.3e  kernel vs float64 %.3e  bound %.3e" % (
        case, float(loss.detach()), want, R_loss, err, 2 * R_loss + 2.0 ** -20 * abs(want)))
    assert err <= 2 * R_loss + 2.0 ** -20 * abs(want), (case, err, R_loss)
    assert abs(float(parts[0]) - want) <= 2 * R_loss + 2.0 ** -20 * abs(want)
    assert float(parts[3]) == float(r64["V"])
    # gradient: against the restatement evaluated with the kernel's own route
    route = K.rmi_pool(seg, target)[1]
    x64 = seg.double().requires_grad_(True)
    restate(x64, target, lam, way, lw, route=route)["loss"].backward()
    g64 = x64.grad
    gerr = float((x.grad.double() - g64).abs().max())
    gmax = float(g64.abs().max())
    print("%s: R_g %.3e  d seg vs float64 with the kernel's route %.3e  bound %.3e  max|g64| %.3e" % (
        case, R_g, gerr, 2 * R_g + 2.0 ** -20 * gmax, gmax))
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(loss.detach()))
    assert gerr <= 2 * R_g + 2.0 ** -20 * gmax, (case, gerr, R_g, gmax)
    if case in ("min9", "min7"):                      # one stencil point: the centred vectors are zero, only the BCE term is left
        x2 = seg.double().requires_grad_(True)
        (lw * (lam if way else 1.0) * restate(x2, target, lam, way, lw)["bce"]).backward()
        assert float((x.grad.double() - x2.grad).abs().max()) <= 2.0 ** -20 * gmax


@pytest.mark.parametrize("case", ["odd", "k171", "sat", "min9", "ign"])
def test_covariances_match_the_centred_float64_product(case):
    from contrastiveseg_amd import kernels as K
    seg, target, gold, r64 = _case(case, str(_dev()))
    p_pool, route, l_pool, _ = K.rmi_pool(seg, target)
    cov, means = K.rmi_cov(p_pool, l_pool)
    B, K_, hp, wp = p_pool.shape
    nh, nw = hp - 2, wp - 2
    M = nh * nw
    la = torch.stack([l_pool[:, :, y:y + nh, x:x + nw] for y in range(3) for x in range(3)], dim=2).reshape(B, K_, 9, -1).double()
    pr = torch.stack([p_pool[:, :, y:y + nh, x:x + nw] for y in range(3) for x in range(3)], dim=2).reshape(B, K_, 9, -1).double()
    assert float((means[:, :, 0] - la.mean(3)).abs().max()) <= 2.0 ** -50 and float((means[:, :, 1] - pr.mean(3)).abs().max()) <= 2.0 ** -50
    la = la - la.mean(dim=3, keepdim=True)
    pr = pr - pr.mean(dim=3, keepdim=True)
    want = torch.stack([la @ la.transpose(2, 3), pr @ pr.transpose(2, 3), la @ pr.transpose(2, 3)], dim=2)
    err = float((cov - want).abs().max())
    bound = 8.0 * M * M * 2.0 ** -53
    print("%s: M %d  covariances vs the centred float64 product %.3e  bound %.3e" % (case, M, err, bound))
    assert err <= bound, (case, err, bound)


@pytest.mark.parametrize("case", ["odd", "k171", "sat", "ign"])
def test_solve_matches_torch_float64_autograd(case):
    from contrastiveseg_amd import kernels as K
    seg, target, gold, r64 = _case(case, str(_dev()))
    p_pool, route, l_pool, _ = K.rmi_pool(seg, target)
    cov, _ = K.rmi_cov(p_pool, l_pool)
    rmi, grads = K.rmi_solve(cov)
    cov_c = cov.detach().cpu()

    def yardstick(c):
        c = c.clone().requires_grad_(True)
        val = rmi_from_cov(c[:, :, 0], c[:, :, 1], c[:, :, 2])
        g, = torch.autograd.grad(val.sum(), c)
        return val.detach(), g[:, :, 1] + g[:, :, 1].transpose(-2, -1), g[:, :, 2]

    v0, gp0, glp0 = yardstick(cov_c)
    gen = torch.Generator().manual_seed(304)
    D = [0.0, 0.0, 0.0]
    for _ in range(4):
        pert = cov_c * (1.0 + 2.0 ** -50 * (2.0 * torch.rand(cov_c.shape, generator=gen, dtype=torch.float64) - 1.0))
        for i, (a, b) in enumerate(zip(yardstick(pert), (v0, gp0, glp0))):
            D[i] = max(D[i], float((a - b).abs().max()))
    for what, got, want, d in (("rmi", rmi, v0, D[0]), ("Gp + Gp^T", grads[:, :, 0], gp0, D[1]), ("Glp", grads[:, :, 1], glp0, D[2])):
        err = float((got.cpu() - want).abs().max())
        bound = 8 * d + 2.0 ** -44 * float(want.abs().max())
        print("%s %s: D %.3e  kernel vs torch float64 %.3e  bound %.3e  max|.| %.3e" % (case, what, d, err, bound, float(want.abs().max())))
        assert err <= bound, (case, what, err, bound)


def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    seg, target, _, _ = _case("city", str(_dev()))
    outs = []
    for _ in range(2):
        x = seg.clone().requires_grad_(True)
        loss, parts = K.rmi_loss(x, target, 0.5, 1, 1.0, want_terms=True)
        loss.backward()
        outs.append((loss.detach().clone(), parts.clone(), x.grad.clone()) + tuple(t.clone() for t in K.rmi_pool(seg, target)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _cfg(loss_type, K_, use_rmi=True, **params):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    p = {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}
    if use_rmi:
        p.update(num_classes=K_, rmi_radius=3, rmi_pool_way=0, rmi_pool_size=3, rmi_pool_stride=3, loss_weight_lambda=0.5,
                 loss_weight=1.0, lambda_way=1, use_sigmoid=False)
    p.update(params)
    return Configer(config_dict={
        "data": {"num_classes": K_}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": 4},
        "contrast": dict(proj_dim=16, temperature=0.1, base_temperature=0.07, max_samples=64, max_views=4, loss_weight=0.1,
                         use_rmi=use_rmi, use_lovasz=False, warmup_iters=0, with_memory="mem" in loss_type, memory_size=8,
                         pixel_update_freq=2),
        "loss": {"loss_type": loss_type, "params": p}})


def test_refusals():
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.rmi_loss import RMILoss
    dev = _dev()
    seg = torch.randn(1, 4, 2, 2, device=dev)
    with pytest.raises(RuntimeError, match="pooled map is 2 x 3"):
        K.rmi_loss(seg, torch.zeros(1, 6, 7, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="pooled map is 3 x 2"):
        K.rmi_pool(seg, torch.zeros(1, 7, 6, dtype=torch.int64, device=dev))
    tgt = torch.zeros(1, 7, 7, dtype=torch.int64, device=dev)
    for kw, name in ((dict(radius=5), "rmi_radius"), (dict(pool_way=1), "rmi_pool_way"), (dict(pool_size=2), "rmi_pool_size"),
                     (dict(pool_stride=2), "rmi_pool_stride")):
        with pytest.raises(RuntimeError, match=name):
            K.rmi_pool(seg, tgt, **kw)
    with pytest.raises(RuntimeError, match="pooled map is 2 x 2"):
        K.rmi_cov(torch.zeros(1, 1, 2, 2, device=dev), torch.zeros(1, 1, 2, 2, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match=r"\[\.\.\., 3, 9, 9\]"):
        K.rmi_solve(torch.zeros(2, 9, 9, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="only upsampling"):
        K.rmi_loss(torch.randn(1, 4, 9, 9, device=dev), tgt)
    for key, bad in (("rmi_radius", 5), ("rmi_pool_way", 1), ("rmi_pool_size", 2), ("rmi_pool_stride", 1)):
        with pytest.raises(NotImplementedError, match=key):
            RMILoss(_cfg("contrast_ce_loss", 4, **{key: bad}))
    with pytest.raises(RuntimeError, match="num_classes"):
        RMILoss(_cfg("contrast_ce_loss", 5))(seg, tgt)
    if dev.type == "cuda":
        with pytest.raises(RuntimeError, match="GPU"):
            K.rmi_loss(seg.cpu(), tgt)


def test_nothing_of_the_size_of_the_upsampled_logits_is_allocated():
    from contrastiveseg_amd import kernels as K
    seg, target, _, _ = _case("city", str(_dev()))
    dev = seg.device
    x = seg.clone().requires_grad_(True)
    B, K_ = seg.shape[:2]
    H, W = target.shape[-2:]
    if dev.type != "cuda":
        K.rmi_loss(x, target).backward()
        return
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    K.rmi_loss(x, target).backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("peak growth %d bytes; the upsampled logits would be %d" % (growth, B * K_ * H * W * 4))
    assert growth < B * K_ * H * W * 4


# ---- the contrast criteria with contrast.use_rmi ------------------------------------------------------------------------------------
def _criterion_inputs(dev, K_=5):
    seg, target = inputs("odd")
    g = torch.Generator().manual_seed(305)
    B, _, h, w = seg.shape
    aux = torch.randn(B, K_, h, w, generator=g) * 2
    embed = F.normalize(torch.randn(B, 16, h, w, generator=g), dim=1)
    return seg.to(dev), aux.to(dev), embed.to(dev), target.to(dev)


@pytest.mark.parametrize("loss_type,queues", [("contrast_ce_loss", False), ("contrast_auxce_loss", False), ("mem_contrast_ce_loss", False),
                                              ("mem_contrast_ce_loss", True), ("mem_contrast_auxce_loss", False),
                                              ("mem_contrast_auxce_loss", True)])
def test_contrast_criteria_with_use_rmi(loss_type, queues):
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    K_ = 5
    seg, aux, embed, target = _criterion_inputs(dev, K_)
    crit = SEG_LOSS_DICT[loss_type](_cfg(loss_type, K_)).to(dev)
    preds = {"seg": seg.clone().requires_grad_(True), "embed": embed.clone().requires_grad_(True)}
    has_aux = "aux" in loss_type
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
    # the segmentation term against float64
    gold = dict(np.load(os.path.join(GOLDEN, "rmi_odd.npz")))
    _, R_loss, _ = _R(gold)
    with torch.no_grad():
        want = restate(seg, target, 0.5, 1, 1.0)["loss"]
        if has_aux:
            up = F.interpolate(aux.double(), size=target.shape[-2:], mode="bilinear", align_corners=True)
            ce = F.cross_entropy(up, target, ignore_index=-1)
            R_ce = abs(float(F.cross_entropy(F.interpolate(aux, size=target.shape[-2:], mode="bilinear", align_corners=True), target,
                                             ignore_index=-1)) - float(ce))
            want = 1.0 * want + 0.4 * ce
            R_loss = R_loss + 0.4 * R_ce
    got = float(crit.last_terms[0])
    print("%s queues=%s: segmentation term %.9g  float64 %.9g  R %.3e" % (loss_type, queues, got, float(want), R_loss))
    assert abs(got - float(want)) <= 2 * R_loss + 2.0 ** -20 * abs(float(want))
    # the validation pass calls the criterion under no_grad
    with torch.no_grad():
        torch.manual_seed(304)
        again = crit({k: v.detach() for k, v in preds.items()}, target, with_embed=True)
    assert float(crit.last_terms[0]) == got and bool(torch.isfinite(again))


def test_use_lovasz_stays_refused():
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    cfg = _cfg("mem_contrast_ce_loss", 5)
    cfg.get("contrast")["use_lovasz"] = True
    with pytest.raises(NotImplementedError, match="use_lovasz"):
        SEG_LOSS_DICT["mem_contrast_ce_loss"](cfg)


def test_without_use_rmi_the_criteria_are_unchanged():
    """use_rmi false: the segmentation criterion is the cross-entropy one and the criterion's output is, bit for bit, the fused
    upsample + CE kernel's value plus the contrast term, as before."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_helper import FSAuxCELoss, FSCELoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    dev = _dev()
    seg, aux, embed, target = _criterion_inputs(dev)
    for loss_type, cls in (("contrast_ce_loss", FSCELoss), ("contrast_auxce_loss", FSAuxCELoss), ("mem_contrast_ce_loss", FSCELoss),
                           ("mem_contrast_auxce_loss", FSAuxCELoss)):
        crit = SEG_LOSS_DICT[loss_type](_cfg(loss_type, 5, use_rmi=False)).to(dev)
        assert type(crit.seg_criterion) is cls
        preds = {"seg": seg, "embed": embed, "seg_aux": aux}
        torch.manual_seed(304)
        total = crit(preds, target, with_embed=True)
        ce = K.upsample_ce(seg, target, None, -1)
        if cls is FSAuxCELoss:
            ce = 1.0 * ce + 0.4 * K.upsample_ce(aux, target, None, -1)
        assert torch.equal(crit.last_terms[0], ce)
        assert torch.equal(total, ce + 0.1 * crit.last_terms[1])
