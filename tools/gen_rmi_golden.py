"""Writes tests/golden/rmi_<case>.npz: the reference's own RMILoss (lib/loss/rmi_loss.py) on the CPU, on the seeded inputs of
tests/test_gpu_rmi.py, in fp32 and in float64.

    python tools/gen_rmi_golden.py --reference /path/to/the/reference/checkout

Per case: target (int16), seg_sum (checksum of the logits, which the tests regenerate from the seed), loss32 / loss64, dseg32 (f32) /
dseg64 (f64) = d loss / d coarse logits through F.interpolate(bilinear, align_corners=True), and R_p = the largest deviation of the
reference's fp32 pooled probabilities (sigmoid * mask + 1e-6, max-pooled) from float64. The float64 run is the same code with
Tensor.float() returning float64 (the reference casts its one-hot labels, its mask and the per-class result to fp32)."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Cfg(object):
    def __init__(self, params):
        self.params = params

    def get(self, *key):
        assert key == ("loss", "params"), key
        return self.params


def _run(RMILoss, seg, target, K, lam, way, lw, dtype):
    params = dict(use_sigmoid=False, num_classes=K, rmi_radius=3, rmi_pool_way=0, rmi_pool_size=3, rmi_pool_stride=3,
                  loss_weight_lambda=lam, loss_weight=lw, lambda_way=way)
    crit = RMILoss(_Cfg(params))
    x = seg.to(dtype).detach().clone().requires_grad_(True)
    pooled = []
    orig_pool, orig_float = F.max_pool2d, torch.Tensor.float
    if not hasattr(torch, "cholesky"):
        torch.cholesky = lambda m, upper=False: torch.linalg.cholesky(m, upper=upper)
    F.max_pool2d = lambda *a, **k: (pooled.append(orig_pool(*a, **k)), pooled[-1])[1]
    if dtype == torch.float64:
        torch.Tensor.float = lambda self: self.double()
    try:
        up = F.interpolate(x, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
        label = target.clone()
        loss = crit(up, label)
        loss.backward()
    finally:
        F.max_pool2d, torch.Tensor.float = orig_pool, orig_float
    assert torch.equal(label, target)
    return loss.detach(), x.grad.detach(), pooled[1].detach()       # the second pooling is the probabilities'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    torch.cuda.DoubleTensor = torch.DoubleTensor          # the reference's .type(torch.cuda.DoubleTensor), on the CPU
    from lib.loss.rmi_loss import RMILoss
    from tests.test_gpu_rmi import CASES, inputs
    for name, (dims, amp, variant, (lam, way, lw)) in CASES.items():
        seg, target = inputs(name)
        K = dims[1]
        l32, g32, p32 = _run(RMILoss, seg, target, K, lam, way, lw, torch.float32)
        l64, g64, p64 = _run(RMILoss, seg, target, K, lam, way, lw, torch.float64)
        assert g32.dtype == torch.float32 and g64.dtype == torch.float64 and p64.dtype == torch.float64
        R_p = float((p32.double() - p64).abs().max())
        path = os.path.join(args.out, "rmi_%s.npz" % name)
        np.savez_compressed(path, target=target.numpy().astype(np.int16), seg_sum=np.float64(seg.double().sum()),
                            loss32=np.float32(l32), loss64=np.float64(l64), dseg32=g32.numpy(), dseg64=g64.numpy(), R_p=np.float64(R_p))
        print("%-6s loss32 %.9g loss64 %.12g |d| %.3e  R_p %.3e  R_g %.3e  %d bytes" % (
            name, float(l32), float(l64), abs(float(l32) - float(l64)), R_p, float((g32.double() - g64).abs().max()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
