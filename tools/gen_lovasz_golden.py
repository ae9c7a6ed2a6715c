"""Writes tests/golden/lovasz_<case>.npz: the reference's own lovasz_softmax_flat(*flatten_probas(...), only_present=True)
(lib/loss/lovasz_loss.py, as FSCELOVASZLoss of lib/loss/loss_helper.py calls it) on softmax(F.interpolate(seg)) on the CPU, on the seeded
inputs of tests/test_gpu_lovasz.py, in fp32 and in float64.

    python tools/gen_lovasz_golden.py --reference /path/to/the/reference/checkout

Per case: target (int16), seg_sum (checksum of the logits, which the tests regenerate from the seed), loss32 / loss64, dseg32 (f32) /
dseg64 (f64) = d loss / d coarse logits through F.interpolate(bilinear, align_corners=True) and the softmax, and R_e = the largest
deviation of the reference's fp32 probabilities from float64. The float64 run is the same code with Tensor.float() returning float64
(the reference casts its foreground mask to fp32). Cases without a valid pixel have no fixture: the reference returns an empty tensor."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(lovasz_softmax_flat, flatten_probas, seg, target, dtype):
    x = seg.to(dtype).detach().clone().requires_grad_(True)
    orig_float = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self: self.double()
    try:
        up = F.interpolate(x, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
        pred = F.softmax(up, dim=1)
        label = target.clone()
        loss = lovasz_softmax_flat(*flatten_probas(pred, label, -1), only_present=True)
        loss.backward()
    finally:
        torch.Tensor.float = orig_float
    assert torch.equal(label, target)
    return loss.detach(), x.grad.detach(), pred.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from lib.loss.lovasz_loss import flatten_probas, lovasz_softmax_flat
    from tests.test_gpu_lovasz import FIXTURES, inputs
    for name in FIXTURES:
        seg, target = inputs(name)
        l32, g32, p32 = _run(lovasz_softmax_flat, flatten_probas, seg, target, torch.float32)
        l64, g64, p64 = _run(lovasz_softmax_flat, flatten_probas, seg, target, torch.float64)
        assert l32.dtype == torch.float32 and g32.dtype == torch.float32 and l64.dtype == torch.float64 and g64.dtype == torch.float64
        R_e = float((p32.double() - p64).abs().max())
        path = os.path.join(args.out, "lovasz_%s.npz" % name)
        np.savez_compressed(path, target=target.numpy().astype(np.int16), seg_sum=np.float64(seg.double().sum()),
                            loss32=np.float32(l32), loss64=np.float64(l64), dseg32=g32.numpy(), dseg64=g64.numpy(), R_e=np.float64(R_e))
        print("%-6s loss32 %.9g loss64 %.12g R_loss %.3e  R_e %.3e  R_g %.3e  max|g64| %.3e  %d bytes" % (
            name, float(l32), float(l64), abs(float(l32) - float(l64)), R_e, float((g32.double() - g64).abs().max()),
            float(g64.abs().max()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
