"""Time of one cycle of a memory-bank criterion -- forward + backward of the contrastive term, then the enqueue -- on the host path
(default) and with contrast.device_bank (anchor sampling and enqueue on the device: csrc/sampling.hip, csrc/queue.hip, the bank-mode
device-N kernels of csrc/contrast.hip), on the same box in one process, alternating the two. Writes profiles/device_bank_timing.json.

  shape 1     8 x 19 x 128 x 256 logits, 512 x 1024 labels, D = 256, memory_size 5000 (190 000 bank columns), pixel_update_freq 10,
              max_samples 1024, max_views 1 -- the contrast section of configs/cityscapes/H_48_D_4_MEM.json
  shape 2     one image of it
Host wall clock from the call to the end of a device synchronise: the host path's cost is its two host round trips and the planning in
Python, which device events alone would not see. At this bank size N * M >= 2^24, so the HOST path runs the one-launch forward
(cseg_contrast_fwd_fused) while the DEVICE path runs the three-launch forward (there is no one-launch forward with N on the device):
the two columns differ in more than where the planning happens. The two paths draw from different generator streams here (the tool
measures time, not parity). Recorded, not gated: the default stays off whatever these numbers say.

    python tools/device_bank_timing.py [--iters 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("bench_b8", 8), ("one_image", 1)]
K_, h_, w_, H_, W_, D_ = 19, 128, 256, 512, 1024, 256
MS, FREQ, STRIDE, MAX_SAMPLES, MAX_VIEWS = 5000, 10, 4, 1024, 1


def _cfg(device_bank):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    return Configer(config_dict={"data": {"num_classes": K_},
                                 "network": {"loss_weights": {"aux_loss": 0.4, "seg_loss": 1.0}, "stride": STRIDE},
                                 "contrast": {"proj_dim": D_, "temperature": 0.07, "base_temperature": 0.07, "max_samples": MAX_SAMPLES,
                                              "max_views": MAX_VIEWS, "loss_weight": 1, "use_rmi": False, "with_memory": True,
                                              "memory_size": MS, "pixel_update_freq": FREQ, "device_bank": device_bank},
                                 "loss": {"loss_type": "mem_contrast_ce_loss",
                                          "params": {"ce_ignore_index": -1, "ce_reduction": "elementwise_mean"}}})


def _inputs(B, dev):
    g = torch.Generator().manual_seed(304)
    blocks = torch.randint(0, K_, (B, H_ // 32, W_ // 32), generator=g)
    target = blocks.repeat_interleave(32, dim=1).repeat_interleave(32, dim=2).contiguous()
    small = target[:, ::H_ // h_, ::W_ // w_]
    seg = 4.0 * torch.nn.functional.one_hot(small, K_).permute(0, 3, 1, 2).float() + 2.0 * torch.randn(B, K_, h_, w_, generator=g)
    embed = torch.nn.functional.normalize(torch.randn(B, D_, h_, w_, generator=g), dim=1)
    return target.to(dev), seg.contiguous().to(dev), embed.to(dev)


def _side(device_bank, dev):
    """criterion, the trainer's enqueue bound to it, and a bank of its own (random unit rows)."""
    from contrastiveseg_amd.lib.loss.loss_contrast_mem import PixelContrastLoss
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    crit = PixelContrastLoss(_cfg(device_bank)).to(dev)
    me = Trainer.__new__(Trainer)
    me.network_stride, me.memory_size, me.pixel_update_freq = STRIDE, MS, FREQ
    if device_bank:
        me.pixel_loss = crit
    g = torch.Generator().manual_seed(5)
    bank = [torch.nn.functional.normalize(torch.randn(K_, MS, D_, generator=g), dim=2).to(dev), torch.zeros(K_, dtype=torch.long, device=dev),
            torch.nn.functional.normalize(torch.randn(K_, MS, D_, generator=g), dim=2).to(dev), torch.zeros(K_, dtype=torch.long, device=dev)]
    return crit, me, bank


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def rows(iters, warmup, dev):
    from contrastiveseg_amd import kernels as K
    out = []
    for name, B in SHAPES:
        target, seg, embed = _inputs(B, dev)
        torch.manual_seed(304)
        sides = {"host": _side(False, dev), "device": _side(True, dev)}
        total = {"host": [], "device": []}
        loss = {}
        for it in range(warmup + iters):
            for side in ("host", "device"):                # alternate: both see the same box in the same minute
                crit, me, bank = sides[side]
                e = embed.detach().requires_grad_(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                val = crit(e, target, seg=seg, segment_queue=bank[0], pixel_queue=bank[2])
                val.backward()
                me._dequeue_and_enqueue(e.detach(), target, *bank)
                torch.cuda.synchronize()
                if it >= warmup:
                    total[side].append((time.perf_counter() - t0) * 1e3)
                loss[side] = float(val.detach())
        header = sides["device"][0].last_selection["header"].cpu().tolist()
        N = int(header[0])
        M = K_ * 2 * MS
        row = {"shape": name, "B": B, "N": N, "T": header[1], "n_view": header[2], "M": M,
               "host_forward": "one launch (cseg_contrast_fwd_fused)" if (K.CONTRAST_FUSED == "1" or (
                   K.CONTRAST_FUSED == "auto" and N * M >= K.CONTRAST_FUSED_MIN_NM)) else "three launches",
               "device_forward": "three launches (cseg_contrast_fwd_dn_bank)",
               "host_path_ms": _stats(total["host"]), "device_path_ms": _stats(total["device"]),
               "last_loss": loss}
        row["faster"] = "device" if row["device_path_ms"]["median"] < row["host_path_ms"]["median"] else "host"
        out.append(row)
        print(json.dumps(row), flush=True)
        del sides
        torch.cuda.empty_cache()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bank_timing.json"))
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "what": "memory-bank PixelContrastLoss forward + backward + Trainer._dequeue_and_enqueue, host wall ms per cycle "
                   "ending in a device synchronise; host path (default) against contrast.device_bank, alternated in one process. At "
                   "this bank size the host path runs the one-launch forward and the device path the three-launch forward.",
           "cycle": rows(args.iters, args.warmup, dev)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
