"""Times the any-rate dilated 3x3 kernels (csrc/conv3x3_dilany.hip) against what the step runs without them (the libraries: the route
CSEG_CONV3X3_DIL_ANY=0 takes for these shapes), on the GPU, at the shapes of DeepLab-V3-R101-d8 at batch 8:
    ASPP branches (2048 -> 512 on 65 x 129, rates 12 / 24 / 36): forward, backward-data, weight gradient of both routes, one at a
        time, and module forward + backward (SplitConv2d with the switch on / off)
    layer3 (256 -> 256, rate 2) and layer4 (512 -> 512, rate 4): the weight gradient against the library
    --bench   `bench.py --workload cfg4` in fresh child processes, CSEG_CONV3X3_DIL_ANY=1 / 0 alternating (A/B/A/B), then A again (A/A)
Device events after warm-up; every entry repeats until its window is at least --window seconds; the two routes alternate inside this
process, --rounds times, and the spread of the rounds is reported next to the median. "algorithmic_tflops" counts 2 flops per
multiply-add of every (output pixel, tap) pair whose source pixel lies inside the map -- the taps that can be valid -- over the
kernel's time; "share_of_split_roof" divides it by the 833 TFLOP/s roof of the f16x3 split arithmetic. Algorithmic flops over time,
not a utilisation counter.
Results are merged into --out (JSON). Run it once, under a time limit:
    timeout -k 10 900 python tools/dilany_timing.py --out profiles/dilany_timing.json [--bench]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPLIT_ROOF_TFLOPS = 833.0

SHAPES = [  # name, B, Cin, Cout, H, W, rate, which entries
    ("aspp_r101_rate12", 8, 2048, 512, 65, 129, 12, "all"),
    ("aspp_r101_rate24", 8, 2048, 512, 65, 129, 24, "all"),
    ("aspp_r101_rate36", 8, 2048, 512, 65, 129, 36, "all"),
    ("layer3_rate2", 8, 256, 256, 65, 129, 2, "wgrad"),
    ("layer4_rate4", 8, 512, 512, 65, 129, 4, "wgrad"),
]


def timed(fn, window):
    """repeat fn until `window` seconds of device time; returns microseconds per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(3, int(window * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, n


def summarise(samples):
    s = sorted(samples)
    return {"median_us": round(s[len(s) // 2], 1), "min_us": round(s[0], 1), "max_us": round(s[-1], 1)}


def valid_pairs(H, W, d):
    """(output pixel, tap) pairs whose source pixel lies inside the map"""
    rows = [max(0, H - abs(k) * d) for k in (-1, 0, 1)]
    cols = [max(0, W - abs(k) * d) for k in (-1, 0, 1)]
    return sum(r * c for r in rows for c in cols)


def measure_shape(shape, window, rounds):
    import torch
    import torch.nn.functional as F
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.models.tools.module_helper import SplitConv2d
    name, B, ci, co, H, W, d, which = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, ci, H, W, generator=g).relu_().to(dev)
    w = (torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)).to(dev)
    dy = torch.randn(B, co, H, W, generator=g).to(dev)
    ax, ady = K.tensor_amax(x), K.tensor_amax(dy)
    conv_bwd = torch.ops.aten.convolution_backward
    cb_args = (None, [1, 1], [d, d], [d, d], False, [0, 0], 1)
    entries = {"wgrad": {"dilany": lambda: K.conv3x3_dilany_wrw(x, dy, d, ax=ax, ady=ady),
                         "library": lambda: conv_bwd(dy, x, w, *cb_args, [False, True, False])}}
    if which == "all":
        entries["fwd"] = {"dilany": lambda: K.conv3x3_dilany_run(x, w, d, False, None, ax=ax),
                          "library": lambda: F.conv2d(x, w, None, 1, d, d)}
        entries["bwd_data"] = {"dilany": lambda: K.conv3x3_dilany_run(dy, w, d, True, None, ax=ady),
                               "library": lambda: conv_bwd(dy, x, w, *cb_args, [True, False, False])}

        def module(on):
            conv = SplitConv2d(ci, co, kernel_size=3, padding=d, dilation=d, bias=False).to(dev).train()
            with torch.no_grad():
                conv.weight.copy_(w)
            xg = x.clone().requires_grad_(True)

            def step():
                K.CONV3X3_DIL_ANY = on
                xg.grad = None
                conv.weight.grad = None
                conv(xg).backward(dy)
            return step
        calls = []
        orig = K.Conv3x3DilAny.apply
        K.Conv3x3DilAny.apply = staticmethod(lambda *a: (calls.append(1), orig(*a))[1])
        entries["module_fwd_bwd"] = {"dilany": module(True), "library": module(False)}
        entries["module_fwd_bwd"]["dilany"]()
        entries["module_fwd_bwd"]["library"]()
        K.Conv3x3DilAny.apply = orig
        assert len(calls) == 1, "the module must take the new route with the switch on and only then"
    flops = 2.0 * B * ci * co * valid_pairs(H, W, d)
    out = {"shape": {"B": B, "Cin": ci, "Cout": co, "H": H, "W": W, "rate": d},
           "algorithmic_gflop_per_operator": round(flops / 1e9, 2), "valid_tap_share": round(valid_pairs(H, W, d) / (9.0 * H * W), 3)}
    for ename, routes in entries.items():
        samples = {"dilany": [], "library": []}
        reps = {}
        for _ in range(rounds):                       # the two routes alternate inside one process
            for route in ("dilany", "library"):
                us, n = timed(routes[route], window)
                samples[route].append(us)
                reps[route] = n
        row = {}
        for route in ("dilany", "library"):
            row[route] = dict(summarise(samples[route]), calls_per_window=reps[route])
            if ename != "module_fwd_bwd":
                tf = flops / (row[route]["median_us"] * 1e-6) / 1e12
                row[route]["algorithmic_tflops"] = round(tf, 1)
                if route == "dilany":
                    row[route]["share_of_split_roof_833"] = round(tf / SPLIT_ROOF_TFLOPS, 3)
        row["library_over_dilany"] = round(row["library"]["median_us"] / row["dilany"]["median_us"], 3)
        # faster by more than the spread of the rounds: the slowest round of the new route is below the fastest library round
        row["dilany_faster_beyond_spread"] = row["dilany"]["max_us"] < row["library"]["min_us"]
        out[ename] = row
        print(name, ename, json.dumps(row), flush=True)
    K.CONV3X3_DIL_ANY = False
    return out


def bench_ab(steps, warmup, limit):
    """bench.py --workload cfg4 in fresh processes: route on (A) / off (B: the library route, what the step ran before) A/B/A/B, then A
    again for the A/A spread. Stops at the first child that fails."""
    runs = []
    for tag, env_v in (("A", "1"), ("B", "0"), ("A", "1"), ("B", "0"), ("A", "1")):
        env = dict(os.environ, CSEG_CONV3X3_DIL_ANY=env_v)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg4",
                            "--steps", str(steps), "--warmup", str(warmup)], env=env, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            runs.append({"tag": tag, "CSEG_CONV3X3_DIL_ANY": env_v, "returncode": r.returncode, "stderr_tail": r.stderr[-600:]})
            print("bench", tag, "FAILED", r.returncode, r.stderr[-600:], flush=True)
            break
        d = json.loads(lines[-1])
        runs.append({"tag": tag, "CSEG_CONV3X3_DIL_ANY": env_v, "ms_per_step": d["ms_per_step"], "images_per_sec": d["value"],
                     "final_loss": d.get("config", {}).get("final_loss"), "wall_s": round(time.time() - t0, 1)})
        print("bench", json.dumps(runs[-1]), flush=True)
    a = [r["ms_per_step"] for r in runs if r["tag"] == "A" and "ms_per_step" in r]
    b = [r["ms_per_step"] for r in runs if r["tag"] == "B" and "ms_per_step" in r]
    res = {"command": "bench.py --gpus 1 --workload cfg4 --steps %d --warmup %d" % (steps, warmup), "runs": runs}
    if a and b:
        res.update(a_ms=a, b_ms=b, a_spread_ms=round(max(a) - min(a), 3), b_spread_ms=round(max(b) - min(b), 3) if len(b) > 1 else None,
                   a_mean_ms=round(sum(a) / len(a), 3), b_mean_ms=round(sum(b) / len(b), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dilany_timing.json"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--bench-limit", type=int, default=400, help="time limit of one bench.py child, seconds")
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if not args.no_kernels:
        import torch
        if not torch.cuda.is_available():
            sys.exit("needs the GPU: a timing taken anywhere else says nothing")
        res["device"] = torch.cuda.get_device_name(0)
        res["method"] = ("device events after warm-up; windows of >= %.2f s; %d rounds alternating the routes in one process; "
                         "library = F.conv2d / aten.convolution_backward (MIOpen / rocBLAS / CK), the route with CSEG_CONV3X3_DIL_ANY=0; "
                         "TF/s = algorithmic flops of the taps that can be valid over time, not a counter" % (args.window, args.rounds))
        res["shapes"] = {s[0]: measure_shape(s, args.window, args.rounds) for s in SHAPES}
    if args.bench:
        res["bench_cfg4"] = bench_ab(args.bench_steps, args.bench_warmup, args.bench_limit)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
