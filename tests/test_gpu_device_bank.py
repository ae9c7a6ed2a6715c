"""The memory-bank criteria with anchor sampling and the enqueue on the device (contrast.device_bank: cseg_queue_enqueue_device of
csrc/queue.hip, the bank-mode device-N kernels of csrc/contrast.hip, kernels.PixelContrastDeviceBank / queue_enqueue_device,
PixelContrastLoss._forward_device with the queues, Trainer._dequeue_and_enqueue).

Yardstick: the host path under the same seed -- anchor_sampling.plan_selection, trainer_contrastive.plan_enqueue /
Trainer._dequeue_and_enqueue and the mode-2 kernels with the switch off (themselves pinned by the reference's goldens and
tests/test_gpu_queue_edges.py). The planners, the generator and the picks are integer arithmetic; the writers and the contrast kernels
are the host path's statements in the host path's order. Every comparison is therefore exact; no test shape reaches N * M >= 2^24, from
where the host path takes the one-launch forward.
Replayed on the CPU emulation by tests/test_emu_device_bank.py (all but the hipGraph capture and the train step)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [304, 7]
K_, D_ = 5, 16
STEPS = 3


def _dev():
    return torch.device("cuda:0")


def _cfg(device_bank, max_samples=64, max_views=10, ms=8, freq=3, loss_type="mem_contrast_ce_loss", stride=4):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    contrast = {"proj_dim": D_, "temperature": 0.1, "base_temperature": 0.07, "max_samples": max_samples, "max_views": max_views,
                "loss_weight": 0.1, "use_rmi": False, "with_memory": True, "memory_size": ms, "pixel_update_freq": freq}
    if device_bank is not None:
        contrast["device_bank"] = device_bank
    return Configer(config_dict={"data": {"num_classes": K_},
                                 "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": stride},
                                 "contrast": contrast,
                                 "loss": {"loss_type": loss_type, "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


def _pixel_criterion(cfg):
    from contrastiveseg_amd.lib.loss.loss_contrast_mem import PixelContrastLoss
    return PixelContrastLoss(cfg)


def _trainer(stride, ms, freq, pixel_loss=None):
    """Trainer._dequeue_and_enqueue needs three attributes; with `pixel_loss` holding a criterion whose device_bank is on it takes the
    device route, otherwise the host route."""
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    me = Trainer.__new__(Trainer)
    me.network_stride, me.memory_size, me.pixel_update_freq = stride, ms, freq
    if pixel_loss is not None:
        me.pixel_loss = pixel_loss
    return me


def _unit_banks(ms, seed=5):
    g = torch.Generator().manual_seed(seed)
    sq = torch.nn.functional.normalize(torch.randn(K_, ms, D_, generator=g), dim=2)
    pq = torch.nn.functional.normalize(torch.randn(K_, ms, D_, generator=g), dim=2)
    return sq, pq


# ---- 1. the enqueue against the host enqueue ------------------------------------------------------------------------------------
def _strided_to_full(small, stride):
    """Label map whose [::stride, ::stride] positions are `small`; every other position holds class 3 (the stride must skip them)."""
    B, hs, ws = small.shape
    full = torch.full((B, hs * stride, ws * stride), 3, dtype=torch.long)
    full[:, ::stride, ::stride] = small
    return full


def _fill(counts, size):
    """One strided label map (flattened, then shuffled by a fixed permutation) with counts[c] pixels of class c; counts[-1] of -1."""
    vals = []
    for c, n in counts.items():
        vals += [c] * n
    assert len(vals) == size, (len(vals), size)
    t = torch.tensor(vals, dtype=torch.long)
    return t[torch.randperm(size, generator=torch.Generator().manual_seed(size + len(counts)))]


def _enq_case(name):
    """-> dict(labels [B,H,W], stride, ms, freq, seg_ptr, pix_ptr, key_hw)"""
    if name in ("a", "b"):
        # image 0: classes 0 and -1 present, class 1 with n = 1 (no draw, k = 1), class 2 with n = 2, class 4 absent; image 1: class 2 absent
        small = torch.stack([_fill({0: 5, -1: 3, 1: 1, 2: 2, 3: 13}, 24), _fill({0: 4, -1: 2, 1: 6, 3: 5, 4: 7}, 24)]).reshape(2, 4, 6)
        seg_ptr, pix_ptr = [0] * K_, [0] * K_
        if name == "b":
            # class 1: image 0 writes k = 1 at 7 (7 + 1 == ms: reset at equality); class 2: k = 2 at 6 (== ms); class 3: k = 3 at 6 (> ms);
            # class 4: k = 3 at 5 (== ms); every segment pointer at ms - 1
            seg_ptr, pix_ptr = [7] * K_, [0, 7, 6, 6, 5]
        return dict(labels=_strided_to_full(small, 2), stride=2, ms=8, freq=3, seg_ptr=seg_ptr, pix_ptr=pix_ptr, key_hw=(4, 6))
    if name == "c":
        # every image holds class 2 with n >= 3 (and class 1): all pixel writes land on rows 0..2, the segment rows wrap inside one step
        small = torch.stack([_fill({0: 3, 1: 4 + b, 2: 17 - b}, 24) for b in range(4)]).reshape(4, 4, 6)
        return dict(labels=_strided_to_full(small, 2), stride=2, ms=3, freq=3, seg_ptr=[0] * K_, pix_ptr=[0] * K_, key_hw=(4, 6))
    assert name == "d"
    small = _fill({0: 300, -1: 24, 4: 700}, 1024).reshape(1, 32, 32)      # 699 draws: crosses a regeneration of the 624 words
    return dict(labels=_strided_to_full(small, 2), stride=2, ms=8, freq=3, seg_ptr=[0] * K_, pix_ptr=[0] * K_, key_hw=(32, 32))


def _enq_keys(c, step):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(c["labels"].shape[0], D_, *c["key_hw"], generator=g)


def _enq_run(name, seed, device_bank, dev):
    """STEPS consecutive enqueues from one seed -> per step (segment queue, pixel queue, both pointers, the next randperm(50) of the stream)."""
    c = _enq_case(name)
    sq, pq = _unit_banks(c["ms"])
    sq, pq = sq.to(dev), pq.to(dev)
    sp = torch.tensor(c["seg_ptr"], dtype=torch.long, device=dev)
    pp = torch.tensor(c["pix_ptr"], dtype=torch.long, device=dev)
    labels = c["labels"].to(dev)
    torch.manual_seed(seed)
    crit = None
    if device_bank:
        crit = _pixel_criterion(_cfg(True, ms=c["ms"], freq=c["freq"], max_samples=8, stride=c["stride"]))
        assert crit.device_bank is True
    me = _trainer(c["stride"], c["ms"], c["freq"], crit)
    out = []
    for step in range(STEPS):
        me._dequeue_and_enqueue(_enq_keys(c, step).to(dev), labels, sq, sp, pq, pp)
        state = torch.get_rng_state()
        if device_bank:
            crit.export_rng_to_torch()
        nxt = torch.randperm(50)
        torch.set_rng_state(state)
        out.append((sq.cpu().clone(), pq.cpu().clone(), sp.cpu().clone(), pp.cpu().clone(), nxt))
    return out


@functools.lru_cache(maxsize=None)
def _enq_host(name, seed, dev_str):
    return _enq_run(name, seed, False, torch.device(dev_str))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_enqueue_matches_the_host_enqueue(name, seed):
    c = _enq_case(name)
    counts = torch.stack([(c["labels"][:, ::c["stride"], ::c["stride"]] == k).flatten(1).sum(1) for k in range(K_)], dim=1)
    if name in ("a", "b"):                                    # the case holds what it is meant to
        assert counts[0].tolist()[1:] == [1, 2, 13, 0] and counts[1, 2] == 0 and (c["labels"] == -1).any()
    elif name == "c":
        assert (counts[:, 2] >= 3).all() and counts.shape[0] == 4
    else:
        assert counts[0, 4] == 700
    dev = _dev()
    host = _enq_host(name, seed, str(dev))
    got = _enq_run(name, seed, True, dev)
    sq0, pq0 = _unit_banks(c["ms"])
    assert not torch.equal(host[0][0], sq0) and not torch.equal(host[0][1], pq0) and torch.equal(host[0][0][0], sq0[0])
    for step, (h, d) in enumerate(zip(host, got)):
        assert torch.equal(h[2], d[2]), "step %d: segment pointers %s / %s" % (step, h[2].tolist(), d[2].tolist())
        assert torch.equal(h[3], d[3]), "step %d: pixel pointers %s / %s" % (step, h[3].tolist(), d[3].tolist())
        assert torch.equal(h[0], d[0]), "step %d: segment queue differs" % step
        assert torch.equal(h[1], d[1]), "step %d: pixel queue differs" % step
        assert torch.equal(h[4], d[4]), "step %d: the device generator did not advance like the host stream" % step


# ---- 2. criterion + enqueue: host path against device path --------------------------------------------------------------------------
B_, H_, W_, h_, w_ = 2, 96, 128, 24, 32
LAYOUTS = {"n_lt_cap": ([0, 1, 2], [2, 3, 4]),              # T = 6, n_view = 10, N = 60 < Ncap = 64
           "n_eq_cap": ([0, 1, 2, 3], [1, 2, 3, 4])}         # T = 8, n_view = 8, N = Ncap = 64


def _inputs(layout):
    """Blocky labels (vertical stripes, a band of ignored rows), logits = 4 * one_hot(label) + noise, unit-norm embeddings per step:
    the inputs of tests/test_gpu_device_sampling.py."""
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


def _cycle_run(layout, kind, device_bank, with_slot, dev, seed=SEEDS[0], max_views=10):
    """STEPS cycles of forward, backward, enqueue from one seed -> per cycle (loss, sel_pix [N], d embed or deposited rows, N, banks)."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    target, seg, embeds = _inputs(layout)
    target, seg = target.to(dev), seg.to(dev)
    sq, pq = _unit_banks(8)
    sq, pq = sq.to(dev), pq.to(dev)
    sp = torch.zeros(K_, dtype=torch.long, device=dev)
    pp = torch.zeros(K_, dtype=torch.long, device=dev)
    torch.manual_seed(seed)
    cfg = _cfg(device_bank, max_views=max_views)
    crit = (_pixel_criterion(cfg) if kind == "pixel" else SEG_LOSS_DICT["mem_contrast_ce_loss"](cfg)).to(dev)
    pix = crit if kind == "pixel" else crit.contrast_criterion
    assert pix.device_bank == bool(device_bank) and pix.device_sampling is False
    me = _trainer(4, 8, 3, crit if device_bank else None)
    out = []
    for e in embeds:
        e = e.to(dev).requires_grad_(True)
        slot = None
        if with_slot:
            slot = K.SparseGradSlot()
            e._cseg_grad_slot = slot
        if kind == "pixel":
            loss = crit(e, target, seg=seg, segment_queue=sq, pixel_queue=pq)
        else:
            loss = crit({"seg": seg, "embed": e, "segment_queue": sq, "pixel_queue": pq}, target, with_embed=True)
        loss.backward()
        sel = pix.last_selection["sel_pix"].cpu()
        if device_bank:
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
        me._dequeue_and_enqueue(e.detach(), target, sq, sp, pq, pp)          # after the backward, as Trainer.train_step
        out.append((loss.detach().cpu(), sel[:N], grad, N, (sq.cpu().clone(), pq.cpu().clone(), sp.cpu().clone(), pp.cpu().clone())))
    return out, pix


@functools.lru_cache(maxsize=None)
def _cycle_host(layout, kind, with_slot, dev_str):
    out, pix = _cycle_run(layout, kind, False, with_slot, torch.device(dev_str))
    return out, pix.last_selection["plan"]


def _same_banks(h, d, what):
    for name, a, b in zip(("segment queue", "pixel queue", "segment pointers", "pixel pointers"), h, d):
        assert torch.equal(a, b), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("with_slot", [False, True], ids=["dense", "slot"])
@pytest.mark.parametrize("kind", ["pixel", "mem_contrast_ce"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_criterion_and_enqueue_are_bit_identical_to_the_host_path(layout, kind, with_slot):
    dev = _dev()
    host, plan = _cycle_host(layout, kind, with_slot, str(dev))
    assert plan.T == len(LAYOUTS[layout][0]) + len(LAYOUTS[layout][1])
    assert (plan.N == 64) == (layout == "n_eq_cap") and plan.N <= 64 <= K_ * 2 * 8
    got, _ = _cycle_run(layout, kind, True, with_slot, dev)
    for step, ((l_h, sel_h, g_h, n_h, b_h), (l_d, sel_d, g_d, n_d, b_d)) in enumerate(zip(host, got)):
        assert n_h == n_d == plan.N, (step, n_h, n_d)
        assert torch.equal(sel_h, sel_d), "cycle %d: mined pixels differ" % step
        assert torch.isfinite(l_h) and l_h.view(torch.int32) == l_d.view(torch.int32), (step, float(l_h), float(l_d))
        if with_slot:
            assert g_d.shape == (64, D_) and torch.equal(g_d[:n_h], g_h), "cycle %d: deposited rows differ" % step
            assert (g_d[n_h:] == 0).all()
        else:
            assert g_h.abs().max() > 0 and torch.equal(g_h, g_d), "cycle %d: d embed differs" % step
        _same_banks(b_h, b_d, "cycle %d" % step)
    assert not torch.equal(host[0][0], host[1][0])           # the bank of cycle 0 entered the loss of cycle 1


def test_the_bank_must_not_change_between_forward_and_backward():
    dev = _dev()
    target, seg, embeds = _inputs("n_lt_cap")
    sq, pq = _unit_banks(8)
    sq, pq = sq.to(dev), pq.to(dev)
    torch.manual_seed(SEEDS[0])
    crit = _pixel_criterion(_cfg(True)).to(dev)
    e = embeds[0].to(dev).requires_grad_(True)
    loss = crit(e, target.to(dev), seg=seg.to(dev), segment_queue=sq, pixel_queue=pq)
    _trainer(4, 8, 3, crit)._dequeue_and_enqueue(e.detach(), target.to(dev), sq, torch.zeros(K_, dtype=torch.long, device=dev), pq,
                                                  torch.zeros(K_, dtype=torch.long, device=dev))
    with pytest.raises(RuntimeError, match="memory bank was modified"):
        loss.backward()


# ---- 3. status ------------------------------------------------------------------------------------------------------------------------
def test_a_step_with_status_gives_nan_zero_gradient_and_an_untouched_generator():
    """No segment qualifies (max_views larger than every segment): N = 0, loss = 0 / 0, the gradient is exactly zero, the sticky bit is
    set, no draw is made -- so the enqueue of that step draws what the host enqueue draws from the fresh seed."""
    dev = _dev()
    target, seg, embeds = _inputs("n_lt_cap")
    target, seg = target.to(dev), seg.to(dev)

    def banks():
        sq, pq = _unit_banks(8)
        return sq.to(dev), torch.zeros(K_, dtype=torch.long, device=dev), pq.to(dev), torch.zeros(K_, dtype=torch.long, device=dev)
    torch.manual_seed(SEEDS[0])
    h = banks()
    _trainer(4, 8, 3)._dequeue_and_enqueue(embeds[0].to(dev), target, *h)
    want_next = torch.randperm(50)

    torch.manual_seed(SEEDS[0])
    crit = _pixel_criterion(_cfg(True, max_views=5000)).to(dev)
    d = banks()
    e = embeds[0].to(dev).requires_grad_(True)
    loss = crit(e, target, seg=seg, segment_queue=d[0], pixel_queue=d[2])
    loss.backward()
    assert torch.isnan(loss).item() and (e.grad == 0).all()
    assert int(crit.sampling_sticky.cpu()) == 2 and (crit.last_selection["sel_pix"].cpu() == -1).all()
    _trainer(4, 8, 3, crit)._dequeue_and_enqueue(e.detach(), target, *d)
    _same_banks([t.cpu() for t in (h[0], h[2], h[1], h[3])], [t.cpu() for t in (d[0], d[2], d[1], d[3])], "after a step with status")
    crit.export_rng_to_torch()
    assert torch.equal(torch.randperm(50), want_next)


# ---- 4. hipGraph capture: real GPU only (not replayed on the emulated device) ----------------------------------------------------------
def test_cycle_is_capturable_and_replays_like_the_host_steps():
    """Forward + backward + enqueue captured after one eager warm-up cycle; a host synchronisation left in either half would fail the
    capture. Generator state, banks and pointers are device memory, so every replay advances them like an eager cycle."""
    dev = _dev()
    layout = "n_lt_cap"
    host, _ = _cycle_host(layout, "pixel", False, str(dev))
    target, seg, embeds = _inputs(layout)
    target, seg = target.to(dev), seg.to(dev)
    sq0, pq0 = _unit_banks(8)
    sq, pq = sq0.to(dev), pq0.to(dev)
    sp = torch.zeros(K_, dtype=torch.long, device=dev)
    pp = torch.zeros(K_, dtype=torch.long, device=dev)
    crit = _pixel_criterion(_cfg(True)).to(dev)
    me = _trainer(4, 8, 3, crit)
    static_e = embeds[0].to(dev).clone().requires_grad_(True)

    def cycle():
        loss = crit(static_e, target, seg=seg, segment_queue=sq, pixel_queue=pq)
        loss.backward()
        me._dequeue_and_enqueue(static_e.detach(), target, sq, sp, pq, pp)
        return loss
    torch.manual_seed(SEEDS[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up: allocations, the import of the generator state
        cycle()
    torch.cuda.current_stream().wait_stream(side)
    static_e.grad = None
    sq.copy_(sq0.to(dev)), pq.copy_(pq0.to(dev)), sp.zero_(), pp.zero_()
    torch.manual_seed(SEEDS[0])
    crit.import_rng_from_torch()                             # the stream of the host run, into the existing device buffer
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = cycle()
    for k in range(STEPS):
        static_e.data.copy_(embeds[k].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        l_h, sel_h, g_h, _, b_h = host[k]
        assert static_loss.detach().cpu().view(torch.int32) == l_h.view(torch.int32), (k, float(static_loss), float(l_h))
        assert torch.equal(static_e.grad.cpu(), g_h), "replay %d: d embed differs" % k
        assert torch.equal(crit.last_selection["sel_pix"].cpu()[:sel_h.numel()], sel_h)
        _same_banks(b_h, (sq.cpu(), pq.cpu(), sp.cpu(), pp.cpu()), "replay %d" % k)


# ---- 5. train step --------------------------------------------------------------------------------------------------------------------
def test_train_step_with_device_bank_matches_the_host_path():
    """Two Trainer.train_step calls of a memory model with the switch on. Step 1 against the host path on the SAME network outputs,
    banks and generator state (taken from the step by a hook; tests/test_gpu_device_sampling.py says why two trainers are not compared):
    loss and mined pixels of the criterion, then bank and pointers of the enqueue."""
    from contrastiveseg_amd.lib.loss.loss_manager import SEG_LOSS_DICT
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    QUEUES = ("segment_queue", "segment_queue_ptr", "pixel_queue", "pixel_queue_ptr")

    def config(device_bank):
        cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
        cfg.update(["network", "model_name"], "deeplab_v3_mem")
        cfg.update(["loss", "loss_type"], "mem_contrast_auxce_loss")
        cfg.update(["train", "batch_size"], 2)
        cfg.get("train", "data_transformer")["input_size"] = [256, 128]
        cfg.update(["contrast", "max_views"], 12)
        cfg.update(["solver", "max_iters"], 2)
        cfg.add(["contrast", "with_memory"], True)
        cfg.add(["contrast", "memory_size"], 64)
        cfg.add(["contrast", "pixel_update_freq"], 10)
        cfg.add(["contrast", "device_bank"], device_bank)
        cfg.add(["network", "pretrained"], None)
        cfg.add(["network", "resume"], None)
        return cfg
    torch.manual_seed(304)
    cfg = config(True)
    tr = Trainer(cfg, train_loader=[])
    loader = SyntheticLoader(cfg, tr.module_runner.device(), length=2, seed=304, mode="blocky")
    tr.seg_net.train()
    pix = tr.pixel_loss.contrast_criterion
    assert pix.device_bank is True and tr._device_bank_criterion() is pix
    host_crit = SEG_LOSS_DICT[cfg.get("loss", "loss_type")](config(False)).to(tr.module_runner.device())
    assert host_crit.contrast_criterion.device_bank is False
    seen = []

    def hook(mod, args, kwargs):
        preds = {k: (v.detach().clone() if k in QUEUES else v) for k, v in args[0].items()}     # the banks as the criterion saw them
        seen.append(((preds, args[1]), kwargs, torch.get_rng_state()))
    handle = tr.pixel_loss.register_forward_pre_hook(hook, with_kwargs=True)
    net = tr.seg_net.module if hasattr(tr.seg_net, "module") else tr.seg_net
    steps = []
    for batch in loader:
        loss = tr.train_step(batch)
        sel = pix.last_selection["sel_pix"].cpu()
        steps.append((loss.cpu(), sel[sel >= 0], [getattr(net, q).detach().cpu().clone() for q in QUEUES]))
    handle.remove()
    tr._display()                                            # reads the sticky status with the loss: nothing to raise
    assert all(torch.isfinite(l).item() for l, _, _ in steps)
    (preds, target), kwargs, rng = seen[0]
    torch.set_rng_state(rng)                                 # the state the device generator was imported from
    with torch.no_grad():
        l_h = host_crit({k: (v.detach() if torch.is_tensor(v) else v) for k, v in preds.items()}, target, **kwargs).cpu()
    sel_h = host_crit.contrast_criterion.last_selection["sel_pix"].cpu()
    l_d, sel_d, banks_d = steps[0]
    assert kwargs.get("with_embed") is True and sel_h.numel() > 0 and torch.equal(sel_h, sel_d)
    assert l_h.view(torch.int32) == l_d.view(torch.int32), (float(l_h), float(l_d))
    # the host enqueue of the same keys goes on in the same CPU stream, behind the criterion's draws
    _trainer(cfg.get("network", "stride"), 64, 10)._dequeue_and_enqueue(preds["key"], preds["lb_key"], *[preds[q] for q in QUEUES])
    for q, d in zip(QUEUES, banks_d):
        assert torch.equal(preds[q].cpu(), d), "%s after step 1 differs from the host enqueue" % q
    assert int(banks_d[1].sum()) > 0 and int(banks_d[3].sum()) > 0
