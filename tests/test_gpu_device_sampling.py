"""Anchor sampling on the device (contrast.device_sampling: csrc/sampling.hip, the device-N kernels of csrc/contrast.hip,
kernels.sample_anchors / PixelContrastDevice, PixelContrastLoss._forward_device).

Yardstick: the host path under the same seed -- lib/loss/anchor_sampling.plan_selection on torch's CPU generator (itself pinned to the
reference's mined indices by tests/test_gpu_kernels.py and the goldens), and PixelContrastLoss / contrast_ce_loss with the switch off.
Everything the planner and the generator produce is integer arithmetic and is compared exactly; the loss and the gradients are compared
bit for bit too, because the device-N kernels are the host path's kernels for N read from device memory (same statements, same order,
the column split of the backward included).
Replayed on the CPU emulation by tests/test_emu_device_sampling.py (all but the hipGraph capture and the train step)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [304, 7]


def _dev():
    return torch.device("cuda:0")


def _cfg(max_samples, max_views, device_sampling, K=5, D=16, loss_type="contrast_ce_loss"):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    contrast = {"proj_dim": D, "temperature": 0.1, "base_temperature": 0.07, "max_samples": max_samples, "max_views": max_views,
                "loss_weight": 0.1, "use_rmi": False}
    if device_sampling is not None:
        contrast["device_sampling"] = device_sampling
    return Configer(config_dict={"data": {"num_classes": K}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}},
                                 "contrast": contrast,
                                 "loss": {"loss_type": loss_type, "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


# ---- planner and generator from hand-made counts ---------------------------------------------------------------------------------
# name: (max_samples, max_views, counts [B,K,2] (hard, easy), expected (T, n_view, N, draws of one call or None), calls)
PLAN_CASES = {
    # all three reachable keep branches, k == n for n = 2 and n = 1, n = 0, a non-qualifying segment between qualifying ones, two regenerations
    "A": (64, 10, [[(30, 40), (50, 2), (1, 60), (5, 5), (0, 0)], [(0, 700), (0, 0), (1, 11), (0, 0), (700, 0)]], (6, 10, 60, 1585), 1),
    "B": (64, 100, [[(200, 300), (150, 0), (0, 101)]], (3, 21, 63, None), 1),             # n_view = 64 // 3 = 21, odd
    "C": (1024, 100, [[(313, 313)]], (1, 100, 100, 624), 2),                              # a step ends on the regeneration boundary
}


def _counts(rows):
    return np.array(rows, dtype=np.int32)


def _mined(counts, dev):
    """What cseg_classify_partition would hand over for these counts (no images needed): seg_off = exclusive cumsum over
    (class, hard / easy) per image; part_idx only gives P."""
    B, K, _ = counts.shape
    flat = counts.reshape(B, 2 * K).astype(np.int64)
    off = (np.cumsum(flat, axis=1) - flat).astype(np.int32).reshape(B, K, 2)
    P = int(flat.sum(1).max()) + 7
    return {"counts": torch.from_numpy(counts).to(dev), "seg_off": torch.from_numpy(off).to(dev),
            "status": torch.zeros(4, dtype=torch.int32, device=dev), "part_idx": torch.zeros(B, P, dtype=torch.int32, device=dev)}, P


def _criterion(max_samples, max_views, dev):
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    crit = PixelContrastLoss(_cfg(max_samples, max_views, True))
    crit._rng_on(dev)                       # imports the state of torch's CPU generator, as the first forward does
    return crit


def _sample(crit, cp):
    from contrastiveseg_amd import kernels as K
    sel_pos, a_lab, header = K.sample_anchors(cp, crit.max_samples, crit.max_views, crit._rng_state, crit.sampling_sticky)
    return sel_pos.cpu().numpy(), a_lab.cpu().numpy(), header.cpu().numpy()


def _check_against_plan(plan, P, sel_pos, a_lab, header, draws):
    N = plan.N
    assert header[:3].tolist() == [N, plan.T, plan.n_view] and header[4] == 0, header
    if draws is not None:
        assert header[3] == draws, header
    assert np.array_equal(sel_pos[:N], plan.row_img.astype(np.int64) * P + plan.row_off)
    assert np.array_equal(a_lab[:N], plan.row_lab)
    assert (sel_pos[N:] == -1).all() and (a_lab[N:] == -1).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_planner_and_generator_match_the_host_planner(name, seed):
    from contrastiveseg_amd.lib.loss.anchor_sampling import plan_selection
    max_samples, max_views, rows, (T, n_view, N, draws), calls = PLAN_CASES[name]
    counts = _counts(rows)
    torch.manual_seed(seed)
    plans = [plan_selection(counts, max_samples, max_views) for _ in range(calls)]
    want_next = torch.randperm(50)
    assert (plans[0].T, plans[0].n_view, plans[0].N) == (T, n_view, N)
    want_draws = int(np.maximum(counts[(counts.sum(-1) > max_views)] - 1, 0).sum())
    assert draws is None or draws == want_draws

    dev = _dev()
    cp, P = _mined(counts, dev)
    torch.manual_seed(seed)
    crit = _criterion(max_samples, max_views, dev)
    for plan in plans:                                       # consecutive calls without re-seeding
        _check_against_plan(plan, P, *_sample(crit, cp), want_draws)
    assert int(crit.sampling_sticky.cpu()) == 0
    crit.export_rng_to_torch()
    assert torch.equal(torch.randperm(50), want_next), "the device generator did not advance like the host stream"


@pytest.mark.parametrize("what", ["no_segment", "too_many_segments"])
def test_status_leaves_the_generator_untouched(what):
    from contrastiveseg_amd.lib.loss.anchor_sampling import plan_selection
    max_samples, max_views, rows, _, _ = PLAN_CASES["A"]
    counts_a = _counts(rows)
    if what == "no_segment":                                 # no (image, class) has more than max_views pixels: bit 2
        bad_counts, bad_samples, bit = np.full_like(counts_a, 2), max_samples, 2
    else:                                                    # T = 6 > max_samples = 4, n_view = 0: bit 4
        bad_counts, bad_samples, bit = counts_a, 4, 4
    torch.manual_seed(SEEDS[0])
    plan = plan_selection(counts_a, max_samples, max_views)
    dev = _dev()
    torch.manual_seed(SEEDS[0])
    crit = _criterion(max_samples, max_views, dev)
    cp_bad, _ = _mined(bad_counts, dev)
    crit.max_samples = bad_samples
    sel_pos, a_lab, header = _sample(crit, cp_bad)
    assert header[0] == 0 and header[3] == 0 and header[4] == bit, header
    assert (sel_pos == -1).all() and (a_lab == -1).all() and sel_pos.shape == (bad_samples,)
    crit.max_samples = max_samples
    cp, P = _mined(counts_a, dev)
    _check_against_plan(plan, P, *_sample(crit, cp), None)   # the picks of a fresh seed
    assert int(crit.sampling_sticky.cpu()) == bit            # sticky


def test_bad_labels_set_bit_one():
    max_samples, max_views, rows, _, _ = PLAN_CASES["A"]
    dev = _dev()
    torch.manual_seed(SEEDS[0])
    crit = _criterion(max_samples, max_views, dev)
    cp, _ = _mined(_counts(rows), dev)
    cp["status"][0] = 3                                      # the mining kernel saw 3 labels outside [0, K)
    _, _, header = _sample(crit, cp)
    assert header[0] == 0 and header[4] == 1, header


# ---- criterion: host path against device path -------------------------------------------------------------------------------------
B_, K_, H_, W_, h_, w_, D_ = 2, 5, 96, 128, 24, 32, 16
LAYOUTS = {"n_lt_cap": ([0, 1, 2], [2, 3, 4]),              # T = 6, n_view = 10, N = 60 < Ncap = 64
           "n_eq_cap": ([0, 1, 2, 3], [1, 2, 3, 4])}         # T = 8, n_view = 8, N = Ncap = 64
STEPS = 3


def _inputs(layout):
    """Blocky labels (vertical stripes, a band of ignored rows), logits = 4 * one_hot(label) + noise, unit-norm embeddings per step."""
    g = torch.Generator().manual_seed(11)
    target = torch.empty(B_, H_, W_, dtype=torch.long)
    for b, classes in enumerate(LAYOUTS[layout]):
        wd = W_ // len(classes)
        for i, c in enumerate(classes):
            target[b, :, i * wd:(i + 1) * wd if i + 1 < len(classes) else W_] = c
    target[:, :8] = -1
    small = target[:, ::H_ // h_, ::W_ // w_].clamp_min(0)
    seg = 4.0 * torch.nn.functional.one_hot(small, K_).permute(0, 3, 1, 2).float() + 2.0 * torch.randn(B_, K_, h_, w_, generator=g)
    embeds = [torch.nn.functional.normalize(torch.randn(B_, D_, h_, w_, generator=g), dim=1) for _ in range(STEPS)]
    return target, seg.contiguous(), embeds


def _run(layout, kind, device_sampling, with_slot, dev, seed=SEEDS[0]):
    """STEPS consecutive calls from one seed -> per step (loss, sel_pix [N], d embed or deposited rows, N)."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    target, seg, embeds = _inputs(layout)
    target, seg = target.to(dev), seg.to(dev)
    torch.manual_seed(seed)
    cfg = _cfg(64, 10, device_sampling)
    crit = (PixelContrastLoss(cfg) if kind == "pixel" else SEG_LOSS_DICT["contrast_ce_loss"](cfg)).to(dev)
    pix = crit if kind == "pixel" else crit.contrast_criterion
    assert pix.device_sampling == bool(device_sampling)
    out = []
    for e in embeds:
        e = e.to(dev).requires_grad_(True)
        slot = None
        if with_slot:
            slot = K.SparseGradSlot()
            e._cseg_grad_slot = slot
        loss = crit(e, target, seg=seg) if kind == "pixel" else crit({"seg": seg, "embed": e}, target, with_embed=True)
        loss.backward()
        sel = pix.last_selection["sel_pix"].cpu()
        if device_sampling:
            header = pix.last_selection["header"].cpu()
            assert pix.last_selection["plan"] is None and header[4] == 0
            N = int(header[0])
            assert sel.shape == (64,) and (sel[N:] == -1).all()
        else:
            N = sel.numel()
        if with_slot:
            (rows, rows_pix), = slot.take()
            assert torch.equal(rows_pix.cpu()[:N], sel[:N])
            grad = rows.cpu()
        else:
            grad = e.grad.cpu()
        out.append((loss.detach().cpu(), sel[:N], grad, N))
    return out, pix


@functools.lru_cache(maxsize=None)
def _host_run(layout, kind, with_slot, dev_str):
    out, pix = _run(layout, kind, False, with_slot, torch.device(dev_str))
    return out, pix.last_selection["plan"]


@pytest.mark.parametrize("with_slot", [False, True], ids=["dense", "slot"])
@pytest.mark.parametrize("kind", ["pixel", "contrast_ce"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_criterion_is_bit_identical_to_the_host_path(layout, kind, with_slot):
    from contrastiveseg_amd.lib.loss.anchor_sampling import keep_rule
    dev = _dev()
    host, plan = _host_run(layout, kind, with_slot, str(dev))
    # the case exercises what it is meant to: enough segments, hard and easy picks
    assert plan.T >= 4 and plan.T == len(LAYOUTS[layout][0]) + len(LAYOUTS[layout][1])
    assert (plan.N == 64) == (layout == "n_eq_cap") and plan.N <= 64
    from contrastiveseg_amd import kernels as K
    target, seg, _ = _inputs(layout)
    cnt = K.classify_partition(target.to(dev), -1, seg=seg.to(dev))["counts"].cpu().numpy()
    keeps = [keep_rule(int(cnt[b, c, 0]), int(cnt[b, c, 1]), plan.n_view) for b, c in zip(plan.seg_img, plan.seg_cls)]
    assert any(kh > 0 for kh, _ in keeps) and any(ke > 0 for _, ke in keeps), keeps

    got, _ = _run(layout, kind, True, with_slot, dev)
    for step, ((l_h, sel_h, g_h, n_h), (l_d, sel_d, g_d, n_d)) in enumerate(zip(host, got)):
        assert n_h == n_d == plan.N, (step, n_h, n_d)
        assert torch.equal(sel_h, sel_d), "step %d: mined pixels differ" % step
        assert torch.isfinite(l_h) and l_h.view(torch.int32) == l_d.view(torch.int32), (step, float(l_h), float(l_d))
        if with_slot:
            assert g_d.shape == (64, D_) and torch.equal(g_d[:n_h], g_h), "step %d: deposited rows differ" % step
            assert (g_d[n_h:] == 0).all()
        else:
            assert g_h.abs().max() > 0 and torch.equal(g_h, g_d), "step %d: d embed differs" % step


def test_a_step_with_status_gives_nan_and_zero_gradient():
    """No segment qualifies (max_views larger than every segment): N = 0, loss = 0 / 0, the gradient is exactly zero, the status is kept."""
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    dev = _dev()
    target, seg, embeds = _inputs("n_lt_cap")
    torch.manual_seed(SEEDS[0])
    crit = PixelContrastLoss(_cfg(64, 5000, True)).to(dev)
    e = embeds[0].to(dev).requires_grad_(True)
    loss = crit(e, target.to(dev), seg=seg.to(dev))
    loss.backward()
    assert torch.isnan(loss).item() and (e.grad == 0).all()
    assert int(crit.sampling_sticky.cpu()) == 2 and (crit.last_selection["sel_pix"].cpu() == -1).all()


# ---- hipGraph capture: real GPU only (not replayed on the emulated device) ---------------------------------------------------------
def test_criterion_is_capturable_and_replays_like_the_host_steps():
    """Forward + backward of PixelContrastLoss captured after one eager warm-up call; a host synchronisation left in the route would
    fail the capture. The state of the generator is device memory, so every replay advances it like an eager step: the loss after
    replay k is the host path's k-th step."""
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    dev = _dev()
    layout = "n_lt_cap"
    host, _ = _host_run(layout, "pixel", False, str(dev))
    target, seg, embeds = _inputs(layout)
    target, seg = target.to(dev), seg.to(dev)
    crit = PixelContrastLoss(_cfg(64, 10, True)).to(dev)
    static_e = embeds[0].to(dev).clone().requires_grad_(True)
    torch.manual_seed(SEEDS[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up: allocations, the import of the generator state
        crit(static_e, target, seg=seg).backward()
    torch.cuda.current_stream().wait_stream(side)
    static_e.grad = None
    torch.manual_seed(SEEDS[0])
    crit.import_rng_from_torch()                             # the stream of the host run, into the existing device buffer
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = crit(static_e, target, seg=seg)
        static_loss.backward()
    for k in range(STEPS):
        static_e.data.copy_(embeds[k].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        l_h, sel_h, g_h, _ = host[k]
        assert static_loss.detach().cpu().view(torch.int32) == l_h.view(torch.int32), (k, float(static_loss), float(l_h))
        assert torch.equal(static_e.grad.cpu(), g_h), "replay %d: d embed differs" % k
        assert torch.equal(crit.last_selection["sel_pix"].cpu()[:sel_h.numel()], sel_h)


# ---- train step ------------------------------------------------------------------------------------------------------------------
def test_train_step_with_device_sampling_matches_the_host_path():
    """Two Trainer.train_step calls with the switch on; the loss and the mined pixels of step 1 against the host-path criterion.
    Both criteria see the SAME network outputs (taken from the step by a hook) and the same generator state: a first version built two
    trainers from one seed and compared their step-1 losses; alone it passed bit for bit, inside the whole suite the two losses were
    3.282113790512085 and 3.2821149826049805 (5 ulp) with identical mined pixels -- two builds of the network in one process do not
    always produce bit-identical logits, which is not what this test is about."""
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer

    def config(device_sampling):
        cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
        cfg.update(["train", "batch_size"], 2)
        cfg.get("train", "data_transformer")["input_size"] = [256, 128]
        cfg.update(["contrast", "max_views"], 12)
        cfg.update(["solver", "max_iters"], 2)
        cfg.add(["contrast", "device_sampling"], device_sampling)
        cfg.add(["network", "pretrained"], None)
        cfg.add(["network", "resume"], None)
        return cfg
    torch.manual_seed(304)
    cfg = config(True)
    tr = Trainer(cfg, train_loader=[])
    loader = SyntheticLoader(cfg, tr.module_runner.device(), length=2, seed=304, mode="blocky")
    tr.seg_net.train()
    pix = tr.pixel_loss.contrast_criterion
    assert pix.device_sampling is True
    host_crit = SEG_LOSS_DICT[cfg.get("loss", "loss_type")](config(False)).to(tr.module_runner.device())
    assert host_crit.contrast_criterion.device_sampling is False
    seen = []
    hook = tr.pixel_loss.register_forward_pre_hook(
        lambda mod, args, kwargs: seen.append((args, kwargs, torch.get_rng_state())), with_kwargs=True)
    steps = []
    for batch in loader:
        loss = tr.train_step(batch)
        sel = pix.last_selection["sel_pix"].cpu()
        steps.append((loss.cpu(), sel[sel >= 0]))
    hook.remove()
    tr._display()                                            # reads the sticky status with the loss: nothing to raise
    assert all(torch.isfinite(l).item() for l, _ in steps)
    (preds, target), kwargs, rng = seen[0]
    torch.set_rng_state(rng)                                 # the state the device generator was imported from
    with torch.no_grad():
        l_h = host_crit({k: (v.detach() if torch.is_tensor(v) else v) for k, v in preds.items()}, target, **kwargs).cpu()
    sel_h = host_crit.contrast_criterion.last_selection["sel_pix"].cpu()
    l_d, sel_d = steps[0]
    assert kwargs.get("with_embed") is True and sel_h.numel() > 0 and torch.equal(sel_h, sel_d)
    assert l_h.view(torch.int32) == l_d.view(torch.int32), (float(l_h), float(l_d))
