"""Times kernels.ms_fuse_argmax against the torch composition of the reference's test phase (segmentor/tester.py:310-327, 380-398:
per scale two F.interpolate(bilinear, align_corners=True) to full size, a flip, an add, a scale, an accumulate) followed by argmax,
in one process on the GPU, and records peak allocated memory of both and the kernel's algorithmic bytes (every coarse map once + one
byte per output pixel).

    python tools/ms_eval_probe.py [--calls 50] [--out profiles/ms_eval_probe.json]

Shapes: the Cityscapes ms_test (B 1, K 19, 1024 x 2048, the seven scales 0.5 ... 2.0 at stride 4, plain + flipped maps) and one
COCO-Stuff validation batch (16 x 171 x 520 x 520 from one 130 x 130 map, the CSEG_VAL_FUSED shape). Inputs are seeded like the
tests'. Both routes are warmed up, then timed call by call with device events, alternating A/B/A/B; median (min - max) over the calls."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def compose_argmax(terms, H, W):
    B, K = terms[0][0].shape[:2]
    full = torch.zeros(B, K, H, W, dtype=torch.float32, device=terms[0][0].device)
    for a, b, w in terms:
        probs = F.interpolate(a, size=(H, W), mode="bilinear", align_corners=True)
        if b is not None:
            probs = probs + torch.flip(F.interpolate(b, size=(H, W), mode="bilinear", align_corners=True), dims=[3])
        full += probs if w == 1.0 else w * probs
    return full.argmax(1)


def make_terms(B, K, sizes, paired, dev):
    g = torch.Generator().manual_seed(304)
    terms = []
    for h, w in sizes:
        a = torch.randn(B, K, h, w, generator=g) * 4
        b = (torch.flip(a, dims=[3]) + 0.5 * torch.randn(B, K, h, w, generator=g)).to(dev) if paired else None
        terms.append((a.to(dev), b, 1.0))
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


def probe(name, B, K, H, W, sizes, paired, calls, dev):
    from contrastiveseg_amd import kernels as Kn
    terms = make_terms(B, K, sizes, paired, dev)
    routes = {"kernel": lambda: Kn.ms_fuse_argmax(terms, H, W), "torch": lambda: compose_argmax(terms, H, W)}
    agree = float((routes["kernel"]().long() == routes["torch"]()).double().mean())
    peaks = {r: peak_of(fn) for r, fn in routes.items()}
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
    src_bytes = sum(4 * t.numel() for a, b, _ in terms for t in (a, b) if t is not None)
    alg = src_bytes + B * H * W
    res = {"shape": {"B": B, "K": K, "H": H, "W": W, "terms": [list(s) for s in sizes], "paired": paired},
           "kernel": dict(stats(times["kernel"]), peak_alloc_bytes=peaks["kernel"]),
           "torch_composition_argmax": dict(stats(times["torch"]), peak_alloc_bytes=peaks["torch"]),
           "algorithmic_bytes": alg, "fused_map_bytes": 4 * B * K * H * W, "argmax_agreement": agree}
    k, t = res["kernel"], res["torch_composition_argmax"]
    res["torch_over_kernel"] = round(t["median_us"] / k["median_us"], 3)
    res["kernel_faster_beyond_spread"] = bool(k["max_us"] < t["min_us"])
    res["kernel_GB_per_s_algorithmic"] = round(alg / k["median_us"] * 1e-3, 1)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_eval_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s4 = [(int(1024 * s) // 4, int(2048 * s) // 4) for s in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)]
    out = {"device": torch.cuda.get_device_name(0),
           "method": "device events around every call after 3 warm-up calls per route; %d calls per route alternating kernel / torch in one "
                     "process; median (min - max); peak = growth of torch.cuda.max_memory_allocated around one call" % args.calls,
           "cityscapes_ms_test": probe("cityscapes_ms_test", 1, 19, 1024, 2048, s4, True, args.calls, dev),
           "coco_stuff_val_batch": probe("coco_stuff_val_batch", 16, 171, 520, 520, [(130, 130)], False, args.calls, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
