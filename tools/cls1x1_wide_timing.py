"""Times the classifier kernels for 33 .. 256 classes (csrc/cls1x1_wide.hip) against what the step runs without them
(nn.Dropout2d + nn.Conv2d on the libraries: the route CSEG_CLS1X1_WIDE=0 takes), on the GPU, at the shapes of the shipped
configurations:
    kernels   forward, backward-data and weight gradient of both routes, one at a time
    module    FoldedDropout2d + ClassifierConv1x1 against nn.Dropout2d + nn.Conv2d: forward + backward in training mode
    --bench   `bench.py --workload cfg5` in fresh child processes, CSEG_CLS1X1_WIDE=1 / 0 alternating (A/B/A/B), then A again (A/A)
Device events after warm-up; every entry repeats until its window is at least --window seconds; the two routes alternate inside this
process, --rounds times, and the spread of the rounds is reported next to the median. "share_of_fp32_peak" is the ALGORITHMIC
2 B C K P flops over the kernel's time as a share of the 157.3 TFLOP/s fp32 matrix peak -- not a utilisation counter.
Results are merged into --out (JSON). Run it once, under a time limit:
    timeout -k 10 900 python tools/cls1x1_wide_timing.py --out profiles/cls1x1_wide_timing.json [--bench]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_PEAK_TFLOPS = 157.3

SHAPES = [  # name, B, C, K, H, W, bias, dropout p
    ("cfg5_hrnet_head", 16, 720, 171, 130, 130, False, 0.10),
    ("cfg5_ocr_classifier", 16, 512, 171, 130, 130, True, 0.0),
    ("ade20k_head", 8, 720, 150, 128, 128, False, 0.10),
]


def timed(fn, window):
    """median-free single window: repeat fn until `window` seconds of device time; returns microseconds per call"""
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


def measure_shape(shape, window, rounds):
    import ctypes
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.models.tools.module_helper import ClassifierConv1x1, FoldedDropout2d
    name, B, C, Kc, H, W, bias, p = shape
    dev = torch.device("cuda:0")
    P, KP = H * W, K.cls1x1_wide_kp(Kc)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=g).relu_().to(dev)
    w = (torch.randn(Kc, C, 1, 1, generator=g) / C ** 0.5).to(dev)
    b = torch.randn(Kc, generator=g).to(dev) if bias else None
    dy = torch.randn(B, Kc, H, W, generator=g).to(dev)
    wt = K.cls1x1_weights(w, B, None, KP).contiguous()
    y, dx, dwt = torch.empty_like(dy), torch.empty_like(x), torch.empty(B, C, KP, device=dev)
    ws = torch.empty(_hip.lib().cseg_cls1x1_wide_wrw_ws_floats(B, C, KP, ctypes.c_long(P)), device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    cP = ctypes.c_long(P)
    conv_bwd = torch.ops.aten.convolution_backward
    cb_args = ([Kc] if bias else None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1)
    entries = {
        "fwd": {"wide": lambda: _hip.call("cseg_cls1x1_wide_fwd", ptr(x), ptr(wt), ptr(b), B, C, Kc, KP, cP, ptr(y), _hip.stream_ptr()),
                "library": lambda: F.conv2d(x, w, b)},
        "bwd_data": {"wide": lambda: _hip.call("cseg_cls1x1_wide_bwd", ptr(dy), ptr(wt), B, C, Kc, KP, cP, ptr(dx), _hip.stream_ptr()),
                     "library": lambda: conv_bwd(dy, x, w, *cb_args, [True, False, False])},
        "wgrad": {"wide": lambda: _hip.call("cseg_cls1x1_wide_wrw", ptr(x), ptr(dy), B, C, Kc, KP, cP, ptr(ws), ptr(dwt), _hip.stream_ptr()),
                  "library": lambda: conv_bwd(dy, x, w, *cb_args, [False, True, False])},
    }

    def module(fast):
        conv = ClassifierConv1x1(C, Kc, kernel_size=1, bias=bias) if fast else nn.Conv2d(C, Kc, kernel_size=1, bias=bias)
        net = nn.Sequential(FoldedDropout2d(p, conv) if fast else nn.Dropout2d(p), conv).to(dev).train()
        with torch.no_grad():
            conv.weight.copy_(w)
        xg = x.clone().requires_grad_(True)

        def step():
            xg.grad = None
            conv.weight.grad = None
            net(xg).backward(dy)
        return step
    K.CLS1X1_WIDE = True                               # route (a), whatever the default of the switch
    calls = []
    orig = K.Cls1x1Wide.apply
    K.Cls1x1Wide.apply = staticmethod(lambda *a: (calls.append(1), orig(*a))[1])
    entries["module_fwd_bwd_train"] = {"wide": module(True), "library": module(False)}
    entries["module_fwd_bwd_train"]["wide"]()
    K.Cls1x1Wide.apply = orig
    assert calls, "the module did not take the wide route"
    flops = 2.0 * B * C * Kc * P
    out = {"shape": {"B": B, "C": C, "K": Kc, "KP": KP, "H": H, "W": W, "bias": bias, "dropout_p": p}, "algorithmic_gflop_per_operator": round(flops / 1e9, 2)}
    for ename, routes in entries.items():
        samples = {"wide": [], "library": []}
        reps = {}
        for _ in range(rounds):                       # the two routes alternate inside one process
            for route in ("wide", "library"):
                us, n = timed(routes[route], window)
                samples[route].append(us)
                reps[route] = n
        row = {}
        for route in ("wide", "library"):
            row[route] = dict(summarise(samples[route]), calls_per_window=reps[route])
            if ename != "module_fwd_bwd_train":
                tf = flops / (row[route]["median_us"] * 1e-6) / 1e12
                row[route]["algorithmic_tflops"] = round(tf, 1)
                row[route]["share_of_fp32_peak_157.3"] = round(tf / FP32_PEAK_TFLOPS, 3)
        row["library_over_wide"] = round(row["library"]["median_us"] / row["wide"]["median_us"], 3)
        # faster by more than the spread of the rounds: the slowest wide round is below the fastest library round
        row["wide_faster_beyond_spread"] = row["wide"]["max_us"] < row["library"]["min_us"]
        out[ename] = row
        print(name, ename, json.dumps(row), flush=True)
    return out


def bench_ab(steps, warmup, limit):
    """bench.py --workload cfg5 in fresh processes: wide on (A) / off (B: the library route, what the step ran before) A/B/A/B, then A
    again for the A/A spread. Stops at the first child that fails."""
    runs = []
    for tag, env_v in (("A", "1"), ("B", "0"), ("A", "1"), ("B", "0"), ("A", "1")):
        env = dict(os.environ, CSEG_CLS1X1_WIDE=env_v)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg5",
                            "--steps", str(steps), "--warmup", str(warmup)], env=env, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            runs.append({"tag": tag, "CSEG_CLS1X1_WIDE": env_v, "returncode": r.returncode, "stderr_tail": r.stderr[-600:]})
            print("bench", tag, "FAILED", r.returncode, r.stderr[-600:], flush=True)
            break
        d = json.loads(lines[-1])
        runs.append({"tag": tag, "CSEG_CLS1X1_WIDE": env_v, "ms_per_step": d["ms_per_step"], "images_per_sec": d["value"],
                     "final_loss": d.get("config", {}).get("final_loss"), "wall_s": round(time.time() - t0, 1)})
        print("bench", json.dumps(runs[-1]), flush=True)
    a = [r["ms_per_step"] for r in runs if r["tag"] == "A" and "ms_per_step" in r]
    b = [r["ms_per_step"] for r in runs if r["tag"] == "B" and "ms_per_step" in r]
    res = {"command": "bench.py --gpus 1 --workload cfg5 --steps %d --warmup %d" % (steps, warmup), "runs": runs}
    if a and b:
        res.update(a_ms=a, b_ms=b, a_spread_ms=round(max(a) - min(a), 3), b_spread_ms=round(max(b) - min(b), 3) if len(b) > 1 else None,
                   a_mean_ms=round(sum(a) / len(a), 3), b_mean_ms=round(sum(b) / len(b), 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls1x1_wide_timing.json"))
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
                         "library = nn.Dropout2d + nn.Conv2d (rocBLAS / MIOpen), the route with CSEG_CLS1X1_WIDE=0" % (args.window, args.rounds))
        res["shapes"] = {s[0]: measure_shape(s, args.window, args.rounds) for s in SHAPES}
    if args.bench:
        res["bench_cfg5"] = bench_ab(args.bench_steps, args.bench_warmup, args.bench_limit)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
