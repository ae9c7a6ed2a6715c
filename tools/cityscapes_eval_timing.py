"""Times the pixel-level Cityscapes evaluation of the test phase on one batch: the kernel route -- kernels.cs_eval_update (with the
read-back of its status words) and kernels.cs_eval_reduce -- against a torch composition of the same commit that computes the same
numbers on the device the way the reference does on the host (lib/metrics/cityscapes_evaluator.py:607-649): torch.bincount for the
34 x 34 matrix, then per image torch.unique over the instance ids above 1000 and, per instance, one full-image mask with its three
counts; the float64 sums are accumulated on the host in the reference's order in both routes' comparisons. Both routes start from the
prediction, the raw label ids and the instance ids on the device.

    python tools/cityscapes_eval_timing.py [--calls 10] [--out profiles/cityscapes_eval_timing.json]

Shape: one batch of 8 x 1024 x 2048 with a few dozen synthetic instances per image (rectangles of labels 24..33 on a background of
label patches; predictions = the truth with block errors). Inputs are seeded. Both routes are warmed up, then timed call by call on
the host clock between two device synchronisations, alternating A/B/A/B; median (min - max) over the calls. The two routes' matrices and
integer sums must agree and the weighted sums must be bit-equal before anything is timed. A measurement, not a gate: nothing is
asserted about the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LABEL_LIST = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


def make_inputs(B, H, W, n_inst, dev):
    rs = np.random.RandomState(304)
    inv = np.full(34, 255, np.uint8)
    inv[LABEL_LIST] = np.arange(len(LABEL_LIST))
    raw = np.full((B, H, W), 7, np.uint8)
    for b in range(B):
        for _ in range(40):
            y, x = rs.randint(0, H - 64), rs.randint(0, W - 128)
            raw[b, y:y + rs.randint(32, 256), x:x + rs.randint(64, 512)] = [0, 3, 4, 7, 8, 11, 21, 23, 9, 17][rs.randint(10)]
    inst = raw.astype(np.uint16)
    for b in range(B):
        for n in range(n_inst):
            l = 24 + rs.randint(10)
            y, x = rs.randint(0, H - 32), rs.randint(0, W - 32)
            h, w = rs.randint(16, 200), rs.randint(16, 300)
            raw[b, y:y + h, x:x + w], inst[b, y:y + h, x:x + w] = l, l * 1000 + n
    pred = np.where(inv[raw] == 255, 0, inv[raw]).astype(np.uint8)
    for b in range(B):
        for _ in range(60):
            y, x = rs.randint(0, H - 64), rs.randint(0, W - 64)
            pred[b, y:y + rs.randint(8, 128), x:x + rs.randint(8, 256)] = rs.randint(len(LABEL_LIST))
    lut = np.zeros(256, np.uint8)
    lut[:len(LABEL_LIST)] = LABEL_LIST
    return (torch.from_numpy(pred).to(dev), torch.from_numpy(lut).to(dev), torch.from_numpy(raw).to(dev),
            torch.from_numpy(inst.view(np.int16)).to(dev))


def kernel_route(pred, lut, raw, inst, records):
    from contrastiveseg_amd import kernels as K
    dev = pred.device
    conf = torch.zeros(34, 34, dtype=torch.int64, device=dev)
    si = torch.zeros(10, 2, dtype=torch.int64, device=dev)
    sf = torch.zeros(10, 2, dtype=torch.float64, device=dev)
    K.cs_eval_reduce(K.cs_eval_update(pred, lut, raw, inst, records, conf), si, sf)
    return conf, si, sf


def torch_route(pred, lut, raw, inst, records):
    """The same numbers from torch ops: one bincount, then one mask per instance; the counts of an image come to the host in one copy and
    the float64 chains run there, in the reference's order."""
    from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
    p = lut[pred.long()].long()
    ids = inst.long() & 0xFFFF
    conf = torch.bincount(raw.long().reshape(-1) * 34 + p.reshape(-1), minlength=34 * 34).reshape(34, 34)
    rows = {name: [0, 0, 0.0, 0.0] for name in CS.STAT_ROWS}
    human = (p == 24) | (p == 25)
    vehicle = (p >= 26) & (p <= 33)
    for b in range(pred.shape[0]):
        found = torch.unique(ids[b][ids[b] > 1000])
        counts = []
        for i in found.tolist():
            l = i // 1000
            mask = ids[b] == i
            counts.append(torch.stack([mask.sum(), (mask & (p[b] == l)).sum(), (mask & (human[b] if l <= 25 else vehicle[b])).sum()]))
        counts = torch.stack(counts).cpu().tolist() if counts else []
        for i, (size, tp, cat_tp) in zip(found.tolist(), counts):
            label = CS.ID2LABEL[i // 1000]
            if label.ignore_in_eval:
                continue
            weight = CS.AVG_CLASS_SIZE[label.name] / float(size)
            for row, t in ((label.name, tp), (label.category, cat_tp)):
                acc = rows[row]
                acc[0] += t
                acc[1] += size - t
                acc[2] += float(t) * weight
                acc[3] += float(size - t) * weight
    si = torch.tensor([[rows[r][0], rows[r][1]] for r in CS.STAT_ROWS], dtype=torch.int64)
    sf = torch.tensor([[rows[r][2], rows[r][3]] for r in CS.STAT_ROWS], dtype=torch.float64)
    return conf, si, sf


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "calls": len(us)}


def probe(B, H, W, n_inst, calls, dev):
    args = make_inputs(B, H, W, n_inst, dev) + ([(0, 0, W, H)] * B,)
    routes = {"kernel": lambda: kernel_route(*args), "torch": lambda: torch_route(*args)}
    (kc, ki, kf), (tc, ti, tf) = routes["kernel"](), routes["torch"]()
    assert torch.equal(kc.cpu(), tc.cpu()) and torch.equal(ki.cpu(), ti) and torch.equal(kf.cpu().view(torch.int64), tf.view(torch.int64))
    for fn in routes.values():
        for _ in range(2):
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
    from contrastiveseg_amd import kernels as K
    conf = torch.zeros(34, 34, dtype=torch.int64, device=dev)
    si, sf = torch.zeros(10, 2, dtype=torch.int64, device=dev), torch.zeros(10, 2, dtype=torch.float64, device=dev)
    table = K.cs_eval_update(*args, conf)
    parts = {"update": [], "reduce": []}
    for _ in range(calls):
        for name, fn in (("update", lambda: K.cs_eval_update(*args, conf)), ("reduce", lambda: K.cs_eval_reduce(table, si, sf))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            parts[name].append((time.perf_counter() - t0) * 1e6)
    res = {"shape": {"B": B, "H": H, "W": W, "instances_per_image": n_inst, "instance_pixels": int(((args[3].long() & 0xFFFF) > 1000).sum())},
           "kernel_route": stats(times["kernel"]), "torch_composition": stats(times["torch"]),
           "cs_eval_update_with_status_readback": stats(parts["update"]), "cs_eval_reduce": stats(parts["reduce"]),
           "results_equal": True}
    res["torch_over_kernel"] = round(res["torch_composition"]["median_us"] / res["kernel_route"]["median_us"], 3)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cityscapes_eval_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "method": "host clock between two device synchronisations around every call, after 2 warm-up calls per route; %d calls per "
                     "route alternating kernel / torch in one process; median (min - max); both routes start from device tensors and "
                     "end with the matrix and the sums; the kernel route includes the read-back of its status words" % args.calls,
           "cityscapes_batch": probe(8, 1024, 2048, 40, args.calls, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
