"""Time and peak memory of the fused RMI segmentation term (kernels.rmi_loss, csrc/rmi.hip) against the torch composition of the
reference (lib/loss/rmi_loss.py: upsample, one-hot, sigmoid, max-pool, nine shifted views in float64, covariances, inverse, Cholesky)
on the same device, forward + backward. Writes profiles/rmi_timing.json. Both sides are recorded; when the composition fails at a
shape (out of memory, a batched factorisation the torch build lacks) the error is recorded instead.

    python tools/rmi_timing.py [--iters 5] [--warmup 2]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("cityscapes_b8", 8, 19, 128, 256, 512, 1024), ("coco_stuff_b16", 16, 171, 130, 130, 520, 520)]


def composition(seg, target, lam=0.5):
    K = seg.shape[1]
    x = F.interpolate(seg, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
    mask = (target >= 0) & (target < K)
    onehot = F.one_hot(target * mask, K).float() * mask.float().unsqueeze(3)
    flat = x.permute(0, 2, 3, 1).contiguous().view(-1, K)
    bce = F.binary_cross_entropy_with_logits(flat, onehot.view(-1, K), weight=mask.float().view(-1, 1), reduction="sum")
    bce = bce / (mask.float().sum() + 1.0)
    probs = x.sigmoid() * mask.float().unsqueeze(1) + 1e-6
    labels = F.max_pool2d(onehot.permute(0, 3, 1, 2), 3, 3, 1)
    probs = F.max_pool2d(probs, 3, 3, 1)
    B, _, hp, wp = probs.shape
    nh, nw = hp - 2, wp - 2
    la = torch.stack([labels[:, :, y:y + nh, x_:x_ + nw] for y in range(3) for x_ in range(3)], dim=2).view(B, K, 9, -1).double()
    pr = torch.stack([probs[:, :, y:y + nh, x_:x_ + nw] for y in range(3) for x_ in range(3)], dim=2).view(B, K, 9, -1).double()
    eye = torch.eye(9, dtype=torch.float64, device=seg.device)
    la = la - la.mean(dim=3, keepdim=True)
    pr = pr - pr.mean(dim=3, keepdim=True)
    la_cov = la @ la.transpose(2, 3)
    pr_inv = torch.inverse(pr @ pr.transpose(2, 3) + eye * 1e-3)
    la_pr = la @ pr.transpose(2, 3)
    appro = la_cov - (la_pr @ pr_inv) @ la_pr.transpose(-2, -1)
    chol = torch.linalg.cholesky(appro + eye * 1e-3)
    rmi = 0.5 * 2.0 * torch.log(torch.diagonal(chol, dim1=-2, dim2=-1) + 1e-8).sum(-1)
    rmi = (rmi.view(-1, K).mean(0).float() / 9.0).sum()
    return lam * bce + (1 - lam) * rmi


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmi_timing.json"))
    args = ap.parse_args()
    from contrastiveseg_amd import kernels as K
    dev = torch.device("cuda:0")
    rows = []
    for name, B, K_, h, w, H, W in SHAPES:
        g = torch.Generator().manual_seed(304)
        seg = (torch.randn(B, K_, h, w, generator=g) * 3).to(dev)
        target = torch.randint(0, K_, (B, (H + 7) // 8, (W + 7) // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        target = target[:, :H, :W].contiguous()
        target[torch.rand(B, H, W, generator=g) < 0.05] = -1
        target = target.to(dev)
        row = {"shape": name, "B": B, "K": K_, "coarse": [h, w], "labels": [H, W], "upsampled_logits_bytes": B * K_ * H * W * 4}
        row["fused"] = measure(lambda x, t: K.rmi_loss(x, t, 0.5, 1, 1.0), seg, target, args.iters, args.warmup)
        try:
            row["torch_composition"] = measure(composition, seg, target, args.iters, args.warmup)
        except Exception as e:                                   # recorded, not hidden: out of memory or a missing batched routine
            row["torch_composition"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
            torch.cuda.empty_cache()
        print(json.dumps(row))
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "what": "forward + backward of the RMI segmentation term, ms per call and peak allocator bytes above the inputs", "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
