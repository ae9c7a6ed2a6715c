"""Times the fused object-context kernels (csrc/ocr.hip, CSEG_OCR_FUSED=1) against what the step runs without them (the torch
composition of lib/models/modules/spatial_ocr_block.py on rocBLAS: the route CSEG_OCR_FUSED=0 takes), on the GPU, at the shapes of the
shipped OCR configurations:
    gather_fwd / attn_fwd   each forward of both routes under torch.no_grad(), one at a time
    gather_bwd / attn_bwd   each backward alone: the autograd graph of ONE forward is retained and its backward is repeated
    both_fwd_bwd            gather -> attention, forward + backward of both, the way the model chains them
    --bench   `bench.py --workload cfg5` in fresh child processes, CSEG_OCR_FUSED=0 / 1 / 0 / 1
Device events after warm-up; every entry repeats until its window is at least --window seconds; the two routes alternate inside this
process, --rounds times; median (min - max) of the rounds. torch.cuda.max_memory_allocated of one forward + backward of each route is
recorded per shape. Results are merged into --out (JSON). Run it once, under a time limit:
    timeout -k 10 900 python tools/ocr_fused_timing.py --out profiles/ocr_fused_timing.json [--bench]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # name, B, feature channels (gather), key channels (attention), K, H, W
    ("cfg5_coco_stuff", 16, 512, 256, 171, 130, 130),
    ("cityscapes_ocr", 8, 512, 256, 19, 128, 256),
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


def measure_shape(shape, window, rounds):
    import torch
    import torch.nn.functional as F
    from contrastiveseg_amd import kernels as K
    name, B, Cf, Ck, Kc, H, W = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(B, Cf, H, W, generator=g).relu_().to(dev).requires_grad_(True)
    probs = torch.randn(B, Kc, H, W, generator=g).to(dev).requires_grad_(True)
    dctx = torch.randn(B, Cf, Kc, 1, generator=g).to(dev)
    q = torch.randn(B, Ck, H, W, generator=g).relu_().to(dev).requires_grad_(True)
    key = torch.randn(B, Ck, Kc, generator=g).relu_().to(dev).requires_grad_(True)
    value = torch.randn(B, Ck, Kc, generator=g).relu_().to(dev).requires_grad_(True)
    dout = torch.randn(B, Ck, H, W, generator=g).to(dev)
    w_obj = (torch.randn(Ck, Cf, generator=g) / Cf ** 0.5).to(dev)             # stands in for f_object / f_down between the two modules
    scale = Ck ** -0.5

    def lib_gather(f, p):                                  # SpatialGather_Module.forward, switch off
        s = F.softmax(p.reshape(B, Kc, -1), dim=2)
        return torch.matmul(s, f.reshape(B, Cf, -1).permute(0, 2, 1)).permute(0, 2, 1).unsqueeze(3)

    def lib_attn(q_, k_, v_):                              # ObjectAttentionBlock2D.forward between the convolutions, switch off
        sim = F.softmax(scale * torch.matmul(q_.reshape(B, Ck, -1).permute(0, 2, 1), k_), dim=-1)
        return torch.matmul(sim, v_.permute(0, 2, 1)).permute(0, 2, 1).contiguous().reshape(B, Ck, H, W)

    routes = {"fused": (lambda f, p: K.ocr_gather(f, p, 1.0), lambda a, b, c: K.ocr_attention(a, b, c, scale)),
              "library": (lib_gather, lib_attn)}

    def entries(route):
        gather, attn = routes[route]

        def gather_fwd():
            with torch.no_grad():
                gather(feats, probs)

        def attn_fwd():
            with torch.no_grad():
                attn(q, key, value)

        y_gather, y_attn = gather(feats, probs), attn(q, key, value)   # graphs kept alive for the backward-only entries

        def gather_bwd():
            torch.autograd.grad(y_gather, (feats, probs), dctx, retain_graph=True)

        def attn_bwd():
            torch.autograd.grad(y_attn, (q, key, value), dout, retain_graph=True)

        def both_fwd_bwd():
            proxy = torch.matmul(w_obj, gather(feats, probs).squeeze(3))
            torch.autograd.grad(attn(q, proxy, proxy), (feats, probs, q), dout)
        return {"gather_fwd": gather_fwd, "attn_fwd": attn_fwd, "gather_bwd": gather_bwd, "attn_bwd": attn_bwd, "both_fwd_bwd": both_fwd_bwd}

    ents = {r: entries(r) for r in routes}
    out = {"shape": {"B": B, "C_feats": Cf, "C_key": Ck, "K": Kc, "KP": K.ocr_kp(Kc), "H": H, "W": W},
           "map_bytes_B_K_P": 4 * B * Kc * H * W}
    for ename in ents["fused"]:
        samples = {r: [] for r in routes}
        for _ in range(rounds):                            # the two routes alternate inside one process
            for r in routes:
                samples[r].append(timed(ents[r][ename], window)[0])
        row = {r: summarise(samples[r]) for r in routes}
        row["library_over_fused"] = round(row["library"]["median_us"] / row["fused"]["median_us"], 3)
        row["fused_faster_beyond_spread"] = row["fused"]["max_us"] < row["library"]["min_us"]
        out[ename] = row
        print(name, ename, json.dumps(row), flush=True)
    del ents                                               # (drops the retained graphs of the backward-only entries)
    mem = {}
    for r in routes:
        fn = entries(r)["both_fwd_bwd"]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        mem[r] = torch.cuda.max_memory_allocated() - base
    out["max_memory_allocated_above_inputs_bytes_both_fwd_bwd"] = mem
    print(name, "memory", json.dumps(mem), flush=True)
    return out


def bench_ab(steps, warmup, limit):
    """bench.py --workload cfg5 in fresh processes, the switch at 0, 1, 0, 1. Stops at the first child that fails."""
    runs = []
    for env_v in ("0", "1", "0", "1"):
        env = dict(os.environ, CSEG_OCR_FUSED=env_v)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg5",
                            "--steps", str(steps), "--warmup", str(warmup)], env=env, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            runs.append({"CSEG_OCR_FUSED": env_v, "returncode": r.returncode, "stderr_tail": r.stderr[-600:]})
            print("bench", env_v, "FAILED", r.returncode, r.stderr[-600:], flush=True)
            break
        d = json.loads(lines[-1])
        runs.append({"CSEG_OCR_FUSED": env_v, "ms_per_step": d["ms_per_step"], "images_per_sec": d["value"],
                     "final_loss": d.get("config", {}).get("final_loss"), "wall_s": round(time.time() - t0, 1)})
        print("bench", json.dumps(runs[-1]), flush=True)
    return {"command": "bench.py --gpus 1 --workload cfg5 --steps %d --warmup %d" % (steps, warmup), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocr_fused_timing.json"))
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per timed window")
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
        res["method"] = ("device events after warm-up; windows of >= %.2f s; %d rounds alternating the routes in one process; median "
                         "(min - max); library = the torch composition of spatial_ocr_block.py (softmax + matmul on rocBLAS), the route "
                         "with CSEG_OCR_FUSED=0" % (args.window, args.rounds))
        res["shapes"] = {s[0]: measure_shape(s, args.window, args.rounds) for s in SHAPES}
    if args.bench:
        res["bench_cfg5"] = bench_ab(args.bench_steps, args.bench_warmup, args.bench_limit)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
