"""Writes tests/golden/ohem_<case>.npz: the reference's own FSOhemCELoss (lib/loss/loss_helper.py:215-261) on F.interpolate(seg, bilinear,
align_corners=True) on the CPU, on the seeded inputs of tests/test_gpu_ohem.py, in fp32 and in float64.

    python tools/gen_ohem_golden.py --reference /path/to/the/reference/checkout

Per case: target (int16), seg_sum (checksum of the logits, which the tests regenerate from the seed), loss32 / loss64, dseg32 (f32) /
dseg64 (f64) = d loss / d coarse logits, thr32 / thr64 (the threshold the reference compares with), kept32 / kept64 (the kept set as
packed bits over the B * H * W label pixels) and R_p = the largest deviation of the reference's fp32 probabilities of the true class from
float64 over the valid pixels. The reference's constructor moves ce_weight to a GPU; here the criterion is built without the key and its
nn.CrossEntropyLoss is replaced by the one that constructor builds, on the CPU. Threshold and kept set are derived next to the forward by
its own expressions (:245-252), and the mean over that set is checked against the loss the forward returned (it sums in sorted order).

Asserted for every case (a case that fails is moved: min_kept by single steps, or the seed; never the factor):
  * the reference's fp32 and float64 kept sets are equal;
  * the undecided set {valid pixels with |p64 - thr64| <= 16 R_p} is empty when the threshold branch wins and is exactly the rank-k
    pixel when the k-th probability wins."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Cfg(object):
    def __init__(self, params):
        self.params = params

    def exists(self, *key):
        return tuple(key) == ("loss", "params")

    def get(self, *key):
        assert tuple(key) == ("loss", "params")
        return self.params


def _run(FSOhemCELoss, seg, target, weight, thresh, min_kept, dtype):
    crit = FSOhemCELoss(_Cfg({"ohem_thresh": thresh, "ohem_minkeep": min_kept, "ce_reduction": "elementwise_mean", "ce_ignore_index": -1}))
    crit.ce_loss = nn.CrossEntropyLoss(weight=weight.to(dtype), ignore_index=-1, reduction="none")
    x = seg.to(dtype).detach().clone().requires_grad_(True)
    up = F.interpolate(x, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
    label = target.clone()
    loss = crit(up, label)
    loss.backward()
    assert torch.equal(label, target)
    # the quantities the forward derives on the way, by the same expressions (loss_helper.py:245-252)
    with torch.no_grad():
        prob = F.softmax(up, dim=1).gather(1, target.clamp(min=0).unsqueeze(1)).squeeze(1)
        valid = target != -1
        sort_prob = prob[valid].sort().values
        k = min(crit.min_kept, sort_prob.numel() - 1)
        thr = max(sort_prob[k], crit.thresh)
        thr = thr if torch.is_tensor(thr) else torch.tensor(thr, dtype=dtype)
        kept = valid & (prob < thr)
        check = (crit.ce_loss(up, target)[kept]).mean()
        assert abs(float(check) - float(loss)) <= (1e-5 if dtype == torch.float32 else 1e-12) * abs(float(loss)), \
            "the restated selection is not the one the reference's forward made"
    return loss.detach(), x.grad.detach(), prob, thr.to(dtype), kept, valid, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from lib.loss.loss_helper import FSOhemCELoss
    from tests.test_gpu_ohem import CASES, FIXTURES, KTH_BRANCH, inputs
    for name in FIXTURES:
        seg, target, weight = inputs(name)
        _, _, _, thresh, min_kept, _ = CASES[name]
        l32, g32, p32, t32, k32, valid, k = _run(FSOhemCELoss, seg, target, weight, thresh, min_kept, torch.float32)
        l64, g64, p64, t64, k64, _, _ = _run(FSOhemCELoss, seg, target, weight, thresh, min_kept, torch.float64)
        assert l32.dtype == torch.float32 and g32.dtype == torch.float32 and l64.dtype == torch.float64 and g64.dtype == torch.float64
        R_p = float((p32.double() - p64)[valid].abs().max())
        assert torch.equal(k32, k64), "%s: the reference's fp32 and float64 kept sets differ in %d pixels" % (name, int((k32 != k64).sum()))
        dist = (p64 - t64).abs()
        und = valid & (dist <= 16 * R_p)
        kth_wins = float(t64) > float(thresh)
        assert kth_wins == (name in KTH_BRANCH), "%s: the %s branch wins" % (name, "k-th" if kth_wins else "threshold")
        if kth_wins:
            assert int(und.sum()) == 1 and float(p64[und]) == float(t64), "%s: %d undecided pixels" % (name, int(und.sum()))
            gap = float(dist[valid & ~und].min())
        else:
            assert int(und.sum()) == 0, "%s: %d undecided pixels" % (name, int(und.sum()))
            gap = float(dist[valid].min())
        path = os.path.join(args.out, "ohem_%s.npz" % name)
        np.savez_compressed(path, target=target.numpy().astype(np.int16), seg_sum=np.float64(seg.double().sum()),
                            loss32=np.float32(l32), loss64=np.float64(l64), dseg32=g32.numpy(), dseg64=g64.numpy(),
                            thr32=np.float32(t32), thr64=np.float64(t64), kept32=np.packbits(k32.numpy().reshape(-1)),
                            kept64=np.packbits(k64.numpy().reshape(-1)), R_p=np.float64(R_p))
        print("%-6s n %5d k %5d %-6s thr64 %.9g kept %5d  loss64 %.12g R_loss %.3e  R_p %.3e  gap/R_p %.3g  R_g %.3e  max|g64| %.3e  %d bytes"
              % (name, int(valid.sum()), k, "k-th" if kth_wins else "thresh", float(t64), int(k64.sum()), float(l64),
                 abs(float(l32) - float(l64)), R_p, gap / R_p, float((g32.double() - g64).abs().max()), float(g64.abs().max()),
                 os.path.getsize(path)))


if __name__ == "__main__":
    main()
