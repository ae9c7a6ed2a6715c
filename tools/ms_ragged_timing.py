"""Device time of the ragged test-phase scoring (csrc/ms_eval_ragged.hip), recorded, not gated: 8 images of COCO-like sizes (640 x 480,
480 x 640, 500 x 375, ...), each padded right / down to a multiple of 8, K = 171, seven scales (0.5 ... 2.0) with their flips, the
coarse maps given (stride 4: ceil(int(Hp * s) / 4) x ceil(int(Wp * s) / 4)):
  ragged      one kernels.ms_fuse_argmax_ragged call: predictions of every image's own h x w in one packed buffer;
  per_image   eight kernels.ms_fuse_argmax calls at the padded sizes plus eight border crops (pred[0, :h, :w].contiguous()), what the
              Tester would do without the ragged kernel.
Each timing is `--launches` repetitions between two device events, divided by the count; the figure reported is the median over
`--iters` such timings after `--warmup` untimed ones, the candidates timed in alternation. Also recorded: the growth of the peak
allocated memory over one repetition of each, and whether the two give the same bytes. Writes profiles/ms_ragged_timing.json.

    python tools/ms_ragged_timing.py [--iters 11] [--warmup 3] [--launches 20]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COCO_SIZES = [(640, 480), (480, 640), (500, 375), (375, 500), (640, 427), (427, 640), (612, 612), (500, 333)]      # (W, H)
SCALES = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
K_CLS = 171


def medians(fns, iters, warmup, launches):
    """{name: callable} -> {name: median ms per repetition}, candidates in alternation."""
    times = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches if i >= warmup else 1):
                fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b) / launches)
    return {k: {"ms_median": sorted(v)[len(v) // 2], "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}


def peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_ragged_timing.json"))
    args = ap.parse_args()
    from contrastiveseg_amd import kernels as K
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(304)
    images = []
    for w, h in COCO_SIZES:
        Hp, Wp = h + (-h) % 8, w + (-w) % 8
        terms = []
        for s in SCALES:
            hc, wc = math.ceil(int(Hp * s) / 4), math.ceil(int(Wp * s) / 4)
            a = torch.randn(1, K_CLS, hc, wc, generator=g, device=dev) * 4
            b = torch.flip(a, dims=[3]) + 0.5 * torch.randn(1, K_CLS, hc, wc, generator=g, device=dev)
            terms.append((a, b, 1.0))
        images.append((terms, (Hp, Wp), (h, w)))

    def ragged():
        return K.ms_fuse_argmax_ragged(images).pred

    def per_image():
        return [K.ms_fuse_argmax(terms, Hp, Wp)[0, :h, :w].contiguous() for terms, (Hp, Wp), (h, w) in images]

    same = bool(torch.equal(ragged(), torch.cat([p.reshape(-1) for p in per_image()])))
    res = medians({"ragged": ragged, "per_image": per_image}, args.iters, args.warmup, args.launches)
    row = dict({"workload": "coco_8_mixed_k171_7_scales_with_flips", "sizes_wh": COCO_SIZES, "scales": SCALES, "classes": K_CLS,
                "border_pixels": sum(w * h for w, h in COCO_SIZES), "padded_pixels": sum(p[0] * p[1] for _, p, _ in images),
                "coarse_map_bytes": sum(t.numel() * 4 for terms, _, _ in images for a, b, _ in terms for t in (a, b)),
                "outputs_equal": same, "ragged_over_per_image": res["ragged"]["ms_median"] / res["per_image"]["ms_median"],
                "peak_growth_bytes": {"ragged": peak_growth(ragged), "per_image": peak_growth(per_image)}}, **res)
    print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
                   "launches_per_timing": args.launches,
                   "what": "ms per repetition (device events around `launches_per_timing` repetitions; median, min, max over `iters` "
                           "timings); no threshold is set", "rows": [row]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
