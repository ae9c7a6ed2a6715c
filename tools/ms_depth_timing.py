"""Times the depth-aware multi-scale fusion of the test phase (ms_test_depth) on given coarse maps: the kernel route -- upload of the
uint16 disparity map, kernels.lut_u16_u8, kernels.ms_fuse_argmax(pixel_weights=...) -- against the torch composition of the same
commit, which is the reference's (segmentor/tester.py:426-475): per scale two F.interpolate(bilinear, align_corners=True) to full
size, a flip, an add; then per scale a float64 weight map computed with numpy on the host from the disparity map, uploaded as fp32,
a multiply and an accumulate; then argmax. Both routes start from the same host disparity array and end with the prediction on the
device. Records peak allocated memory of both.

    python tools/ms_depth_timing.py [--calls 30] [--out profiles/ms_depth_timing.json]

Shape: the Cityscapes recipe of configs/cityscapes/H_48_D_4_TEST_DEPTH.json (B 1, K 19, 1024 x 2048, the seven scales 0.5 ... 2.0 at
stride 4, plain + flipped maps). Inputs are seeded like the tests'. Both routes are warmed up, then timed call by call on the host
clock between two device synchronisations (the torch route does host work that device events would not bracket), alternating
A/B/A/B; median (min - max) over the calls. A measurement, not a gate: nothing is asserted about the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)


def compose_argmax(terms, H, W, disp, scales):
    """ms_test_depth + fuse_with_depth of the reference on given coarse maps, weight maps on the host as there."""
    B, K = terms[0][0].shape[:2]
    dev = terms[0][0].device
    probs = []
    for a, b, _ in terms:
        p = F.interpolate(a, size=(H, W), mode="bilinear", align_corners=True)
        probs.append(p + torch.flip(F.interpolate(b, size=(H, W), mode="bilinear", align_corners=True), dims=[3]))
    full = torch.zeros(B, K, H, W, dtype=torch.float32, device=dev)
    for index in range(B):
        with np.errstate(divide="ignore"):
            depth_map = 500 * (0.5 / (disp[index] / 256.0))
        depth_map = np.clip(depth_map, 0, 63)
        depth_map = depth_map // (63 // len(scales))
        for i, prob in enumerate(probs):
            weight_map = np.power(0.8, np.abs(depth_map - scales.index(scales[i])))
            full[index] += torch.from_numpy(np.expand_dims(weight_map, axis=0)).to(dev).float() * prob[index]
    return full.argmax(1)


def make_inputs(B, K, H, W, sizes, dev):
    g = torch.Generator().manual_seed(304)
    terms = []
    for h, w in sizes:
        a = torch.randn(B, K, h, w, generator=g) * 4
        b = torch.flip(a, dims=[3]) + 0.5 * torch.randn(B, K, h, w, generator=g)
        terms.append((a.to(dev), b.to(dev), 1.0))
    rs = np.random.RandomState(304)
    disp = rs.randint(0, 65536, size=(B, H, W)).astype(np.uint16)
    disp[:, :H // 2] %= 12000
    disp[:, 0, 0] = 0
    return terms, disp


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


def probe(B, K, H, W, sizes, calls, dev):
    from contrastiveseg_amd import kernels as Kn
    from contrastiveseg_amd.segmentor.tester import depth_fusion_tables
    scales = list(SCALES)
    terms, disp = make_inputs(B, K, H, W, sizes, dev)
    lut, table = depth_fusion_tables(scales)                  # once per Tester
    lut_d, table_d = torch.from_numpy(lut).to(dev), torch.from_numpy(table).to(dev)

    def kernel_route():
        bins = Kn.lut_u16_u8(torch.from_numpy(disp).to(dev), lut_d)
        return Kn.ms_fuse_argmax(terms, H, W, pixel_weights=(bins, table_d))

    routes = {"kernel": kernel_route, "torch": lambda: compose_argmax(terms, H, W, disp, scales)}
    agree = float((routes["kernel"]().long() == routes["torch"]()).double().mean())
    peaks = {r: peak_of(fn) for r, fn in routes.items()}
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    for _ in range(calls):
        for r, fn in routes.items():                         # A/B/A/B
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) * 1e6)
            del out
    res = {"shape": {"B": B, "K": K, "H": H, "W": W, "terms": [list(s) for s in sizes], "paired": True, "bins": int(table.shape[1])},
           "kernel_route": dict(stats(times["kernel"]), peak_alloc_bytes=peaks["kernel"]),
           "torch_composition_argmax": dict(stats(times["torch"]), peak_alloc_bytes=peaks["torch"]),
           "fused_map_bytes": 4 * B * K * H * W, "argmax_agreement": agree}
    k, t = res["kernel_route"], res["torch_composition_argmax"]
    res["torch_over_kernel"] = round(t["median_us"] / k["median_us"], 3)
    res["kernel_faster_beyond_spread"] = bool(k["max_us"] < t["min_us"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_depth_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s4 = [(int(1024 * s) // 4, int(2048 * s) // 4) for s in SCALES]
    out = {"device": torch.cuda.get_device_name(0),
           "method": "host clock between two device synchronisations around every call, after 3 warm-up calls per route; %d calls per "
                     "route alternating kernel / torch in one process; median (min - max); both routes start from the host uint16 "
                     "disparity array; peak = growth of torch.cuda.max_memory_allocated around one call" % args.calls,
           "cityscapes_ms_test_depth": probe(1, 19, 1024, 2048, s4, args.calls, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
