"""Time and peak memory of the OHEM cross entropy (kernels.ohem_ce, csrc/ohem.hip), forward + backward of the term alone, against
  (b) the reference's op sequence as torch ops on the same device (lib/loss/loss_helper.py:215-261: interpolate, softmax, gather, mask,
      a full sort, the Python max that synchronises, cross_entropy, two masked gathers, mean), and
  (c) kernels.upsample_ce forward + backward, the floor OHEM adds to,
at ohem_thresh 0.9 / ohem_minkeep 100000 in two regimes: "early" (random logits: most pixels are hard, the threshold branch wins, the
select takes its shortcut) and "late" (one class per image, its logit boosted by 12: every probability is crowded just below 1.0, fewer
than min_kept pixels lie below the threshold, the k-th branch wins and all three radix levels run). The three are timed in alternation
inside one process; the stage split of (a) comes from device events around each stage in a loop of its own. Writes
profiles/ohem_timing.json; when the composition fails at a shape (out of memory) the error is recorded instead.

    python tools/ohem_timing.py [--iters 10] [--warmup 3]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("cityscapes_b8", 8, 19, 128, 256, 512, 1024), ("coco_stuff_b16", 16, 171, 130, 130, 520, 520)]
THRESH, MIN_KEPT = 0.9, 100000


def composition(seg, target, weight):
    predict = F.interpolate(seg, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
    prob_out = F.softmax(predict, dim=1)
    tmp_target = target.clone()
    tmp_target[tmp_target == -1] = 0
    prob = prob_out.gather(1, tmp_target.unsqueeze(1))
    mask = target.contiguous().view(-1) != -1
    sort_prob, sort_indices = prob.contiguous().view(-1)[mask].contiguous().sort()
    min_threshold = sort_prob[min(MIN_KEPT, sort_prob.numel() - 1)]
    threshold = max(min_threshold, THRESH)                          # synchronises, as in the reference
    loss_matrix = F.cross_entropy(predict, target, weight=weight, ignore_index=-1, reduction="none").contiguous().view(-1)
    sort_loss_matrix = loss_matrix[mask][sort_indices]
    return sort_loss_matrix[sort_prob < threshold].mean()


def inputs(B, K_, h, w, H, W, regime, dev):
    g = torch.Generator().manual_seed(304)
    if regime == "early":
        seg = torch.randn(B, K_, h, w, generator=g) * 3
        target = torch.randint(0, K_, (B, (H + 7) // 8, (W + 7) // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        target = target[:, :H, :W].contiguous()
    else:
        seg = torch.randn(B, K_, h, w, generator=g)
        cls = torch.randint(0, K_, (B,), generator=g)
        seg[torch.arange(B), cls] += 12.0
        target = cls[:, None, None].expand(B, H, W).contiguous()
    target[torch.rand(B, H, W, generator=g) < 0.10] = -1
    return seg.to(dev), target.to(dev), (1.0 + 0.1 * torch.arange(K_, dtype=torch.float32) / K_).to(dev)


def once(fn, seg, target, weight):
    x = seg.detach().requires_grad_(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a.record()
    loss = fn(x, target, weight)
    loss.backward()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, float(loss)


def stages(K, _hip, seg, target, weight, iters, warmup):
    """Device time of each stage of (a), medians over `iters` calls."""
    names = ("prob", "select", "reduce", "bwd")
    times = {n: [] for n in names}
    B, K_, h, w = seg.shape
    P = target.numel()
    for i in range(warmup + iters):
        x = seg.detach().requires_grad_(True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        p, nll, lse, sel = K._ohem_prob(x.detach(), target, -1, THRESH, None, True)
        ev[1].record()
        _hip.call("cseg_ohem_select", K._pf(p), P, THRESH, MIN_KEPT, 1, 1, K._pf(sel), _hip.stream_ptr())
        ev[2].record()
        out, outi = K._ohem_reduce(p, nll, target, weight, K_, sel)
        ev[3].record()
        d_seg = torch.empty_like(seg)
        g = torch.ones(1, device=seg.device)
        _hip.call("cseg_ohem_bwd", K._pf(seg), K._pf(target), K._pf(weight), -1, B, K_, h, w, target.shape[1], target.shape[2], K._pf(p),
                  K._pf(lse), K._pf(out), K._pf(outi), K._pf(g), K._pf(d_seg), _hip.stream_ptr())
        ev[4].record()
        torch.cuda.synchronize()
        if i >= warmup:
            for j, n in enumerate(names):
                times[n].append(ev[j].elapsed_time(ev[j + 1]))
    return {n: sorted(v)[len(v) // 2] for n, v in times.items()}, [int(v) for v in outi.tolist()], [float(v) for v in out.tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ohem_timing.json"))
    args = ap.parse_args()
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    dev = torch.device("cuda:0")
    fns = {"fused": lambda x, t, wt: K.ohem_ce(x, t, wt, -1, THRESH, MIN_KEPT),
           "torch_composition": composition,
           "upsample_ce": lambda x, t, wt: K.upsample_ce(x, t, wt, -1)}
    rows = []
    for name, B, K_, h, w, H, W in SHAPES:
        for regime in ("early", "late"):
            seg, target, weight = inputs(B, K_, h, w, H, W, regime, dev)
            row = {"shape": name, "regime": regime, "B": B, "K": K_, "coarse": [h, w], "labels": [H, W],
                   "upsampled_logits_bytes": B * K_ * H * W * 4, "ohem_thresh": THRESH, "ohem_minkeep": MIN_KEPT}
            res = {k: {"ms_all": [], "peak_bytes_above_inputs": 0} for k in fns}
            for i in range(args.warmup + args.iters):                # (a), (b), (c) in alternation
                for k, fn in fns.items():
                    if "error" in res[k]:
                        continue
                    try:
                        ms, peak, loss = once(fn, seg, target, weight)
                    except Exception as e:                           # recorded, not hidden
                        res[k] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
                        torch.cuda.empty_cache()
                        continue
                    if i >= args.warmup:
                        res[k]["ms_all"].append(ms)
                    res[k]["peak_bytes_above_inputs"] = max(res[k]["peak_bytes_above_inputs"], peak)
                    res[k]["loss"] = loss
            for k in fns:
                if "error" not in res[k]:
                    res[k]["ms_all"].sort()
                    res[k]["ms_median"] = res[k]["ms_all"][len(res[k]["ms_all"]) // 2]
            row.update(res)
            row["fused_stage_ms"], outi, out = stages(K, _hip, seg, target, weight, args.iters, args.warmup)
            row["kept"], row["n_valid"], row["k"], row["shortcut_taken"], row["thr"] = outi[0], outi[1], outi[2], bool(outi[3]), out[2]
            if "error" not in row["torch_composition"]:
                row["fused_over_composition"] = row["fused"]["ms_median"] / row["torch_composition"]["ms_median"]
            row["fused_over_upsample_ce"] = row["fused"]["ms_median"] / row["upsample_ce"]["ms_median"]
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "what": "forward + backward of the OHEM cross entropy, ms per call (device events) and peak allocator bytes above the inputs; "
                   "fused_stage_ms: medians of the stages of the fused route timed in a loop of their own",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
