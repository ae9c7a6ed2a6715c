"""Time of the contrastive criterion with anchor sampling on the host (default) and on the device (contrast.device_sampling,
csrc/sampling.hip), on the same box in one process, alternating the two. Writes profiles/device_sampling_timing.json.

  criterion   PixelContrastLoss forward + backward at the benched shape (8 x 19 x 128 x 256 logits, 512 x 1024 labels, D = 256,
              max_samples 1024, max_views 100) and at one image. Host wall clock from the call to the end of a device synchronise: the
              host path's cost is its host synchronisation and planning, which device events alone would not see.
  generator   the mt19937 kernel alone (device events), for the number of draws a step of that shape makes: one block, a serial chain
              of about draws / 624 * 4 barrier phases.
  bench       bench.py --gpus 1 with and without CSEG_DEVICE_SAMPLING=1, at batch 8 and batch 1 (child processes; --bench 0 skips).
Recorded, not gated: the default stays the host path whatever these numbers say.

    python tools/device_sampling_timing.py [--iters 20] [--warmup 5] [--bench 1] [--bench-steps 10]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("bench_b8", 8), ("one_image", 1)]
K_, h_, w_, H_, W_, D_ = 19, 128, 256, 512, 1024, 256


def _cfg(device_sampling):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    return Configer(config_dict={"data": {"num_classes": K_}, "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}},
                                 "contrast": {"proj_dim": D_, "temperature": 0.1, "base_temperature": 0.07, "max_samples": 1024,
                                              "max_views": 100, "loss_weight": 0.1, "use_rmi": False, "device_sampling": device_sampling},
                                 "loss": {"loss_type": "contrast_ce_loss",
                                          "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


def _inputs(B, dev):
    g = torch.Generator().manual_seed(304)
    blocks = torch.randint(0, K_, (B, H_ // 32, W_ // 32), generator=g)
    target = blocks.repeat_interleave(32, dim=1).repeat_interleave(32, dim=2).contiguous()
    small = target[:, ::H_ // h_, ::W_ // w_]
    seg = 4.0 * torch.nn.functional.one_hot(small, K_).permute(0, 3, 1, 2).float() + 2.0 * torch.randn(B, K_, h_, w_, generator=g)
    embed = torch.nn.functional.normalize(torch.randn(B, D_, h_, w_, generator=g), dim=1)
    return target.to(dev), seg.contiguous().to(dev), embed.to(dev)


def criterion_rows(iters, warmup, dev):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    rows = []
    for name, B in SHAPES:
        target, seg, embed = _inputs(B, dev)
        torch.manual_seed(304)
        crits = {"host": PixelContrastLoss(_cfg(False)).to(dev), "device": PixelContrastLoss(_cfg(True)).to(dev)}
        times = {"host": [], "device": []}
        loss = {}
        for it in range(warmup + iters):
            for side in ("host", "device"):                # alternate: both see the same box in the same minute
                e = embed.detach().requires_grad_(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = crits[side](e, target, seg=seg)
                out.backward()
                torch.cuda.synchronize()
                if it >= warmup:
                    times[side].append((time.perf_counter() - t0) * 1e3)
                loss[side] = float(out)
        header = crits["device"].last_selection["header"].cpu().tolist()
        # the generator alone, for the draws of one step of this shape
        draws = int(header[3])
        rng = crits["device"]._rng_state.clone()
        ev = []
        for it in range(warmup + iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            K.mt_draw(rng, draws)
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ev.append(a.elapsed_time(b) * 1e3)
        row = {"shape": name, "B": B, "N": header[0], "T": header[1], "n_view": header[2], "draws_per_step": draws,
               "host_path_ms": {"median": statistics.median(times["host"]), "min": min(times["host"]), "max": max(times["host"])},
               "device_path_ms": {"median": statistics.median(times["device"]), "min": min(times["device"]), "max": max(times["device"])},
               "generator_kernel_us": {"median": statistics.median(ev), "min": min(ev), "max": max(ev),
                                       "note": "two device events around one launch + a small header fill: an upper bound"},
               "last_loss": loss}
        row["faster"] = "device" if row["device_path_ms"]["median"] < row["host_path_ms"]["median"] else "host"
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_rows(steps, warmup):
    rows = []
    for batch in (8, 1):
        for flag in ("0", "1"):
            env = dict(os.environ, CSEG_DEVICE_SAMPLING=flag)
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                   "--global-batch", str(batch), "--no-cpu-baseline", "--no-kernels", "--no-fp32-pass"]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=420)
            except subprocess.TimeoutExpired:
                rows.append({"global_batch": batch, "CSEG_DEVICE_SAMPLING": flag, "error": "no result after 420 s"})
                return rows                                # nothing more on the GPU after a child that had to be ended
            line = None
            for ln in r.stdout.splitlines():
                if ln.startswith("{") and '"metric"' in ln:
                    line = json.loads(ln)
            row = {"global_batch": batch, "CSEG_DEVICE_SAMPLING": flag, "returncode": r.returncode}
            if line is not None:
                row.update(ms_per_step=line.get("ms_per_step"), images_per_sec=line.get("value"),
                           step_graph=(line.get("config") or {}).get("step_graph") if isinstance(line.get("config"), dict) else None)
            else:
                row["error"] = (r.stderr or r.stdout)[-400:]
            rows.append(row)
            print(json.dumps(row), flush=True)
            if r.returncode not in (0,):
                return rows                                # nothing more on the GPU after a child that did not end cleanly
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--bench", type=int, default=1)
    p.add_argument("--bench-steps", type=int, default=10)
    p.add_argument("--bench-warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_sampling_timing.json"))
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "what": "PixelContrastLoss forward + backward, host wall ms per call ending in a device synchronise; host path (default) "
                   "against contrast.device_sampling, alternated in one process; the mt19937 kernel alone; bench.py on either path",
           "criterion": criterion_rows(args.iters, args.warmup, dev)}
    del dev
    torch.cuda.synchronize()
    if args.bench:
        out["bench"] = bench_rows(args.bench_steps, args.bench_warmup)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
