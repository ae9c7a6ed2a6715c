"""Times the SegFix refinement of the test phase on one batch: kernels.segfix_shift (csrc/segfix.hip) with int8 and with fp32 offsets,
with and without the host-to-device copy of the offsets, against the reference's `shift` composition
(scripts/cityscapes/segfix.py:64-79: coordinate maps, a grid tensor, F.grid_sample on the float image, round) run on device tensors
of the same commit, batched. Both routes start from the prediction on the device and end with the refined train ids on the device.

    python tools/segfix_timing.py [--calls 10] [--out profiles/segfix_timing.json]

Shape: 8 x 1024 x 2048, a blocky 19-class prediction, offsets in {-1, 0, 1} (about half of them zero), scale 2. Inputs are seeded.
Every route is warmed up, then timed call by call on the host clock between two device synchronisations, the routes alternating;
median (min - max) over the calls. Peak memory growth is torch's max_memory_allocated over one call minus the allocation before it
(inputs excluded, outputs included). The composition runs torch's GPU grid_sample, whose order of fp32 operations is not the CPU
one: the number of labels on which it differs from the kernel is recorded, not asserted. A measurement, not a gate."""
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


def make_inputs(B, H, W):
    rs = np.random.RandomState(304)
    bh, bw = H // 24, W // 24
    coarse = rs.randint(0, 19, size=(B, (H + bh - 1) // bh, (W + bw - 1) // bw))
    pred = np.repeat(np.repeat(coarse, bh, axis=1), bw, axis=2)[:, :H, :W].astype(np.uint8)
    off = rs.randint(-1, 2, size=(B, H, W, 2)).astype(np.int8)
    off[rs.random_sample((B, H, W)) < 0.5] = 0
    return np.ascontiguousarray(pred), off


def torch_composition(pred, offsets, scale):
    """The reference's shift, batched, on the device: pred u8 [B,H,W], offsets fp32 [B,H,W,2] -> refined u8 [B,H,W]."""
    B, H, W = pred.shape
    dev = pred.device
    ch, cw = torch.meshgrid([torch.arange(H, dtype=torch.float, device=dev), torch.arange(W, dtype=torch.float, device=dev)], indexing="ij")
    norm = torch.tensor([(W - 1) / 2, (H - 1) / 2], dtype=torch.float, device=dev)
    off = offsets * scale
    grid = torch.stack([off[..., 1] + cw, off[..., 0] + ch], dim=-1) / norm - 1
    out = F.grid_sample(pred.unsqueeze(1).float(), grid, padding_mode="border", mode="bilinear", align_corners=False)
    return torch.round(out.squeeze(1)).to(torch.uint8)


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "calls": len(us)}


def peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return int(grown)


def probe(B, H, W, calls, dev):
    from contrastiveseg_amd import kernels as K
    pred_np, off_np = make_inputs(B, H, W)
    records = [(0, 0, W, H)] * B
    pred = torch.from_numpy(pred_np).to(dev)
    host_i8 = torch.from_numpy(off_np).pin_memory()
    host_f32 = torch.from_numpy(off_np.astype(np.float32)).pin_memory()
    dev_i8, dev_f32 = host_i8.to(dev), host_f32.to(dev)
    lut = torch.arange(256, dtype=torch.uint8, device=dev)
    routes = {
        "kernel_int8": lambda: K.segfix_shift(pred, dev_i8, records, 2.0, lut),
        "kernel_fp32": lambda: K.segfix_shift(pred, dev_f32, records, 2.0, lut),
        "kernel_int8_with_h2d": lambda: K.segfix_shift(pred, host_i8.to(dev), records, 2.0, lut),
        "kernel_fp32_with_h2d": lambda: K.segfix_shift(pred, host_f32.to(dev), records, 2.0, lut),
        "torch_composition": lambda: torch_composition(pred, dev_f32, 2.0),
        "torch_composition_with_h2d": lambda: torch_composition(pred, host_f32.to(dev), 2.0),
    }
    a, b = routes["kernel_int8"]()[0], routes["kernel_fp32"]()[0]
    assert torch.equal(a, b)
    t = routes["torch_composition"]()
    differing = int((t != a).sum())
    changed = int(routes["kernel_int8"]()[2].sum())
    del t
    for fn in routes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    for _ in range(calls):
        for r, fn in routes.items():                       # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) * 1e6)
            del out
    res = {"shape": {"B": B, "H": H, "W": W, "scale": 2.0, "pixels_changed": changed},
           "offset_bytes": {"int8": int(off_np.nbytes), "fp32": int(off_np.nbytes) * 4},
           "int8_and_fp32_outputs_equal": True,
           "labels_differing_from_torch_gpu_grid_sample": differing}
    for r in routes:
        res[r] = stats(times[r])
    res["peak_memory_growth_bytes"] = {"kernel_int8": peak_growth(routes["kernel_int8"]), "kernel_fp32": peak_growth(routes["kernel_fp32"]),
                                       "torch_composition": peak_growth(routes["torch_composition"])}
    res["torch_over_kernel_int8"] = round(res["torch_composition"]["median_us"] / res["kernel_int8"]["median_us"], 2)
    res["torch_over_kernel_int8_with_h2d"] = round(res["torch_composition_with_h2d"]["median_us"] / res["kernel_int8_with_h2d"]["median_us"], 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segfix_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "method": "host clock between two device synchronisations around every call, after 2 warm-up calls per route; %d calls per "
                     "route, the routes alternating in one process; median (min - max); every route starts from the prediction on the "
                     "device and ends with the refined train ids on the device; with_h2d: the offsets start in pinned host memory; the "
                     "kernel routes go through the Python wrapper and also write the dataset ids and the changed-pixel counts" % args.calls,
           "cityscapes_batch": probe(8, 1024, 2048, args.calls, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
