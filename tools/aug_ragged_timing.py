"""Device time of the ragged data pipeline (csrc/augment_ragged.hip), recorded, not gated:
  (a) 16 images of COCO-like sizes (640 x 480, 480 x 640, 500 x 375, ...) through the reference's COCO-Stuff train sequence
      (random_hflip, resize min side 520, random_resize 0.5-2.0, random_crop 520 x 520, random_brightness) -> 16 x 3 x 520 x 520:
      stage 1 (cseg_resize_ragged) and stage 2 (cseg_augment_ragged), records drawn by GPUBatchTransform under a fixed seed;
  (b) a uniform batch of 8 images of 2048 x 1024 -> 1024 x 512 with the Cityscapes sequence: cseg_augment_ragged beside
      cseg_augment_batch on the same decisions (outputs compared with torch.equal).
Each timing is `--launches` launches between two device events, divided by the count; the figure reported is the median over `--iters`
such timings after `--warmup` untimed ones, the candidates timed in alternation. Buffers, records and outputs are allocated once, so
only the kernels are timed. Writes profiles/aug_ragged_timing.json.

    python tools/aug_ragged_timing.py [--iters 11] [--warmup 3] [--launches 20]"""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD, DIV = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], 255.0
COCO_SIZES = [(640, 480), (480, 640), (500, 375), (375, 500), (640, 427), (427, 640), (612, 612), (500, 333)] * 2      # (W, H)


def configer(trans, input_size):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    return Configer(config_dict={
        "data": {"num_classes": 171},
        "train": {"data_transformer": {"size_mode": "fix_size", "input_size": input_size, "align_method": "only_pad",
                                       "pad_mode": "random"}},
        "train_trans": trans, "normalize": {"div_value": DIV, "mean": MEAN, "std": STD}})


def coco_trans():
    return {"trans_seq": ["random_hflip", "resize", "random_resize", "random_crop", "random_brightness"],
            "random_brightness": {"ratio": 1.0, "shift_value": 10}, "resize": {"min_side_length": 520},
            "random_hflip": {"ratio": 0.5, "swap_pair": []},
            "random_resize": {"ratio": 1.0, "method": "random", "scale_range": [0.5, 2.0], "aspect_range": [0.9, 1.1]},
            "random_crop": {"ratio": 1.0, "crop_size": [520, 520], "method": "random", "allow_outside_center": False}}


def city_trans():
    return {"trans_seq": ["random_resize", "random_crop", "random_hflip", "random_brightness"],
            "random_brightness": {"ratio": 1.0, "shift_value": 10}, "random_hflip": {"ratio": 0.5, "swap_pair": []},
            "random_resize": {"ratio": 1.0, "method": "random", "scale_range": [0.5, 2.0], "aspect_range": [0.9, 1.1]},
            "random_crop": {"ratio": 1.0, "crop_size": [1024, 512], "method": "random", "allow_outside_center": False}}


def medians(fns, iters, warmup, launches):
    """{name: callable that launches once} -> {name: median ms per launch}, candidates in alternation."""
    times = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b) / launches)
    return {k: {"ms_median": sorted(v)[len(v) // 2], "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_ragged_timing.json"))
    args = ap.parse_args()
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    dev = torch.device("cuda:0")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    mean3, std3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    rs = np.random.RandomState(0)
    rows = []

    # (a) the COCO-Stuff workload
    t = GPUBatchTransform(configer(coco_trans(), [520, 520]))
    random.seed(304)
    params, offsets, (Wt, Ht) = t.plan_ragged(COCO_SIZES)
    n = sum(w * h for w, h in COCO_SIZES)
    img = torch.from_numpy(rs.randint(0, 256, size=(n, 3)).astype(np.uint8)).to(dev)
    lab = torch.from_numpy(rs.randint(0, 171, size=(n,)).astype(np.uint8)).to(dev)
    mid_img, mid_lab = K.resize_ragged(img, lab, params, offsets)
    m = mid_img.shape[0]
    pd, od = params.to(dev), offsets.to(dev)
    B = params.shape[0]
    out = torch.empty(B, 3, Ht, Wt, device=dev)
    out_lab = torch.empty(B, Ht, Wt, dtype=torch.int64, device=dev)

    def stage1():
        _hip.call("cseg_resize_ragged", P(img), P(lab), n, P(pd), P(od), P(params), P(offsets), B, P(mid_img), P(mid_lab), m,
                  _hip.stream_ptr())

    def stage2():
        _hip.call("cseg_augment_ragged", P(img), P(lab), n, P(mid_img), P(mid_lab), m, ctypes.c_void_p(None), P(pd), P(od), P(params),
                  P(offsets), B, Ht, Wt, DIV, mean3, std3, P(out), P(out_lab), _hip.stream_ptr())

    def both():
        stage1()
        stage2()
    res = medians({"stage1_resize_ragged": stage1, "stage2_augment_ragged": stage2, "stage1_plus_stage2": both}, args.iters,
                  args.warmup, args.launches)
    rows.append(dict({"workload": "coco_stuff_16_mixed_to_520x520", "sizes_wh": COCO_SIZES, "raw_pixels": n, "stage1_pixels": m,
                      "samples_with_two_resamplings": int((params[:, 2] > 0).sum()),
                      "bytes_moved_stage2_out": B * Ht * Wt * (12 + 8)}, **res))
    print(json.dumps(rows[-1]), flush=True)

    # (b) a uniform Cityscapes batch: the ragged stage 2 beside the one-kernel entry point, same decisions
    Bc, Hs, Ws, Ht, Wt = 8, 1024, 2048, 512, 1024
    t = GPUBatchTransform(configer(city_trans(), [Wt, Ht]))
    random.seed(304)
    rows12 = t.plan([(Ws, Hs)] * Bc)
    recs = torch.tensor([[Ws, Hs, 0, 0, 0, r[0], r[1], 0] + r[2:10] for r in rows12.tolist()], dtype=torch.int32)
    offs = torch.tensor([[b * Hs * Ws, 0] for b in range(Bc)], dtype=torch.int64)
    img = torch.from_numpy(rs.randint(0, 256, size=(Bc, Hs, Ws, 3)).astype(np.uint8)).to(dev)
    lab = torch.from_numpy(rs.randint(0, 34, size=(Bc, Hs, Ws)).astype(np.uint8)).to(dev)
    p12, pd, od = rows12.to(dev), recs.to(dev), offs.to(dev)
    out_a, out_b = torch.empty(Bc, 3, Ht, Wt, device=dev), torch.empty(Bc, 3, Ht, Wt, device=dev)
    lab_a, lab_b = (torch.empty(Bc, Ht, Wt, dtype=torch.int64, device=dev) for _ in range(2))
    n = Bc * Hs * Ws

    def batch():
        _hip.call("cseg_augment_batch", P(img), P(lab), ctypes.c_void_p(None), P(p12), Bc, Hs, Ws, Ht, Wt, DIV, mean3, std3, P(out_a),
                  P(lab_a), _hip.stream_ptr())

    def ragged():
        _hip.call("cseg_augment_ragged", P(img), P(lab), n, ctypes.c_void_p(None), ctypes.c_void_p(None), 0, ctypes.c_void_p(None),
                  P(pd), P(od), P(recs), P(offs), Bc, Ht, Wt, DIV, mean3, std3, P(out_b), P(lab_b), _hip.stream_ptr())
    res = medians({"augment_batch": batch, "augment_ragged": ragged}, args.iters, args.warmup, args.launches)
    torch.cuda.synchronize()
    rows.append(dict({"workload": "cityscapes_8x2048x1024_to_1024x512", "outputs_equal": bool(torch.equal(out_a, out_b) and
                                                                                              torch.equal(lab_a, lab_b)),
                      "ragged_over_batch": res["augment_ragged"]["ms_median"] / res["augment_batch"]["ms_median"]}, **res))
    print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
                   "launches_per_timing": args.launches,
                   "what": "ms per launch (device events around `launches_per_timing` launches; median, min, max over `iters` timings); "
                           "no threshold: the pipeline runs one batch ahead of a training step of tens of milliseconds and is not on "
                           "the critical chain", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
