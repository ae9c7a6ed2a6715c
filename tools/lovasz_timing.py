"""Time and peak memory of the Lovasz-softmax segmentation term (kernels.lovasz_softmax, csrc/lovasz.hip) against the reference's op
sequence as torch ops on the same device (lib/loss/lovasz_loss.py: upsample, softmax, permuted copy, nonzero, and per class a presence
test on the host, one torch.sort over all valid pixels and the cumulative sums of lovasz_grad), forward + backward of the term alone.
Writes profiles/lovasz_timing.json. Both sides are recorded; when the composition fails at a shape (out of memory) the error is recorded
instead.

    python tools/lovasz_timing.py [--iters 5] [--warmup 2]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("cityscapes_b8", 8, 19, 128, 256, 512, 1024), ("coco_stuff_b16", 16, 171, 130, 130, 520, 520)]


def _lovasz_grad(gt_sorted):
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    jaccard[1:] = jaccard[1:] - jaccard[:-1]
    return jaccard


def composition(seg, target, ignore=-1):
    K = seg.shape[1]
    pred = F.softmax(F.interpolate(seg, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True), dim=1)
    pred = pred.permute(0, 2, 3, 1).contiguous().view(-1, K)
    labels = target.view(-1)
    valid = labels != ignore
    pred = pred[valid.nonzero().squeeze()]
    labels = labels[valid]
    losses = []
    for c in range(K):
        fg = (labels == c).float()
        if fg.sum() == 0:
            continue
        errors = (fg - pred[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        losses.append(torch.dot(errors_sorted, _lovasz_grad(fg[perm])))
    return sum(losses) / len(losses)


def measure(fn, seg, target, iters, warmup):
    times = []
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = None
    for i in range(warmup + iters):
        x = seg.detach().requires_grad_(True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = fn(x, target)
        loss.backward()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
        del x
    times.sort()
    return {"ms_median": times[len(times) // 2], "ms_all": times, "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base,
            "loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lovasz_timing.json"))
    args = ap.parse_args()
    from contrastiveseg_amd import kernels as K
    dev = torch.device("cuda:0")
    rows = []
    for name, B, K_, h, w, H, W in SHAPES:
        g = torch.Generator().manual_seed(304)
        seg = (torch.randn(B, K_, h, w, generator=g) * 3).to(dev)
        target = torch.randint(0, K_, (B, (H + 7) // 8, (W + 7) // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        target = target[:, :H, :W].contiguous()
        target[torch.rand(B, H, W, generator=g) < 0.10] = -1
        target = target.to(dev)
        row = {"shape": name, "B": B, "K": K_, "coarse": [h, w], "labels": [H, W], "upsampled_logits_bytes": B * K_ * H * W * 4,
               "class_chunk": K.LOVASZ_CLASS_CHUNK}
        row["fused"] = measure(lambda x, t: K.lovasz_softmax(x, t), seg, target, args.iters, args.warmup)
        torch.cuda.empty_cache()
        try:
            row["torch_composition"] = measure(composition, seg, target, args.iters, args.warmup)
        except Exception as e:                                   # recorded, not hidden
            row["torch_composition"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "what": "forward + backward of the Lovasz-softmax segmentation term, ms per call and peak allocator bytes above the inputs",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
