"""Times kernels.crop_fuse_argmax against the torch composition of the reference's sliding-crop test phase (segmentor/tester.py:351-378,
505-523: per scale and flip a logits canvas and a count canvas of [B,K,H*scale,W*scale], a slice-add per crop, a divide, a resize back, the
flip, the add, the accumulation) followed by argmax, given the same coarse maps, in one process on the GPU, and records peak allocated
memory of both.

    python tools/crop_eval_probe.py [--calls 20] [--out profiles/crop_eval_probe.json]

Shapes: the Cityscapes mscrop_test (B 1, K 19, 1024 x 2048, the seven scales 0.5 ... 2.0 with flips, coarse maps at stride 4) with the crop
512 x 1024 and with the crop 769 x 769. Scales below 1 are plain terms (ss_test), the others tiled. Inputs are seeded. Both routes are
warmed up, then timed call by call with device events, alternating A/B/A/B; median (min - max) over the calls. A composition that runs out
of memory is recorded as such."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)


def starts(total, crop):
    """_decide_intersection (:525-533) with its stride = the crop length"""
    return [min(i * crop, total - crop) for i in range(-(-total // crop))]


def sscrop(stack, canvas, crop, H, W):
    (hs, ws), (ch, cw) = canvas, crop
    B, K = stack.shape[1:3]
    full = torch.zeros(B, K, hs, ws, dtype=torch.float32, device=stack.device)
    count = torch.zeros(B, K, hs, ws, dtype=torch.float32, device=stack.device)
    t = 0
    for y0 in starts(hs, ch):
        for x0 in starts(ws, cw):
            count[:, :, y0:y0 + ch, x0:x0 + cw] += 1
            full[:, :, y0:y0 + ch, x0:x0 + cw] += F.interpolate(stack[t], size=(ch, cw), mode="bilinear", align_corners=True)
            t += 1
    full /= count
    return F.interpolate(full, size=(H, W), mode="bilinear", align_corners=True)


def compose_argmax(terms, H, W):
    first = terms[0][0]
    B, K = first.shape[-4:-2]
    full = torch.zeros(B, K, H, W, dtype=torch.float32, device=first.device)
    for term in terms:
        if len(term) == 2:
            one = lambda t: F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)
        else:
            one = lambda t: sscrop(t, term[2], term[3], H, W)
        full += one(term[0]) + torch.flip(one(term[1]), dims=[3])
    return full.argmax(1)


def make_terms(B, K, H, W, crop, dev):
    g = torch.Generator(device=dev).manual_seed(304)
    ch, cw = crop
    terms = []
    for s in SCALES:
        hs, ws = int(H * s), int(W * s)
        if s < 1:
            shape = (B, K, math.ceil(hs / 4), math.ceil(ws / 4))
            terms.append((torch.randn(shape, device=dev, generator=g) * 4, torch.randn(shape, device=dev, generator=g) * 4))
        else:
            shape = (len(starts(hs, ch)) * len(starts(ws, cw)), B, K, math.ceil(ch / 4), math.ceil(cw / 4))
            terms.append((torch.randn(shape, device=dev, generator=g) * 4, torch.randn(shape, device=dev, generator=g) * 4, (hs, ws), crop))
    return terms


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "calls": len(us)}


def probe(name, B, K, H, W, crop, calls, dev):
    from contrastiveseg_amd import kernels as Kn
    terms = make_terms(B, K, H, W, crop, dev)
    routes = {"kernel": lambda: Kn.crop_fuse_argmax(terms, H, W), "torch": lambda: compose_argmax(terms, H, W)}
    res = {"shape": {"B": B, "K": K, "H": H, "W": W, "crop": list(crop), "scales": list(SCALES), "flips": True,
                     "tiles": [len(starts(t[2][0], crop[0])) * len(starts(t[2][1], crop[1])) if len(t) == 4 else 0 for t in terms]},
           "coarse_map_bytes": sum(4 * t.numel() for term in terms for t in term[:2]),
           "largest_canvas_bytes": 4 * B * K * int(H * SCALES[-1]) * int(W * SCALES[-1])}
    try:
        agree = float((routes["kernel"]().long() == routes["torch"]()).double().mean())
        peaks = {r: peak_of(fn) for r, fn in routes.items()}
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        agree, peaks = None, {"kernel": peak_of(routes["kernel"]), "torch": None}
        del routes["torch"]
        res["torch_composition_argmax"] = "out of memory"
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    for _ in range(calls):
        for r, fn in routes.items():                         # A/B/A/B
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            times[r].append(e0.elapsed_time(e1) * 1e3)
            del out
    res["kernel"] = dict(stats(times["kernel"]), peak_alloc_bytes=peaks["kernel"])
    res["argmax_agreement"] = agree
    if "torch" in routes:
        res["torch_composition_argmax"] = dict(stats(times["torch"]), peak_alloc_bytes=peaks["torch"])
        k, t = res["kernel"], res["torch_composition_argmax"]
        res["torch_over_kernel"] = round(t["median_us"] / k["median_us"], 3)
        res["kernel_faster_beyond_spread"] = bool(k["max_us"] < t["min_us"])
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_eval_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "method": "device events around every call after 3 warm-up calls per route; %d calls per route alternating kernel / torch in one "
                     "process; median (min - max); peak = growth of torch.cuda.max_memory_allocated around one call" % args.calls,
           "cityscapes_crop_512x1024": probe("cityscapes_crop_512x1024", 1, 19, 1024, 2048, (512, 1024), args.calls, dev),
           "cityscapes_crop_769x769": probe("cityscapes_crop_769x769", 1, 19, 1024, 2048, (769, 769), args.calls, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
