"""Dilated 3x3 convolutions at any rate on the MI355X (csrc/conv3x3_dilany.hip, kernels.Conv3x3DilAny): output, input gradient,
weight gradient and bias gradient against F.conv2d in float64 with padding = dilation = d, at the yardstick of
tests/test_gpu_conv3x3_sb.py (`_bound`: within 8x the library's own fp32 deviation from float64, floor 4e-6 of the scale) -- the
edge cases tests/test_emu_dilany.py replays on the emulated device, ASPP-like shapes, and one full-size ASPP branch; determinism of
the weight gradient; and the DeepLab goldens (model forward, one SGD step) with the route switched on, at the tolerances of the
files that own them."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EDGE_CASES = [  # B, Cin, Cout, H, W, d  (tests/test_emu_dilany.py CASES)
    (1, 64, 64, 7, 33, 12), (2, 128, 64, 30, 20, 24), (1, 64, 128, 9, 10, 36), (1, 256, 64, 13, 65, 12), (1, 64, 48, 6, 17, 2),
    (1, 48, 64, 8, 36, 4), (1, 64, 64, 5, 16, 1)]
ASPP_CASES = [(2, 512, 512, 33, 65, 12), (1, 2048, 512, 17, 33, 24), (1, 512, 512, 65, 129, 36)]
FULL_SIZE = (8, 2048, 512, 65, 129, 12)      # one ASPP branch of DeepLab-V3-R101-d8 at batch 8 (the test prints its errors; DESIGN.md section 15.3 says what has been recorded)


def _count(monkeypatch, fn_class, calls):
    orig = fn_class.apply
    monkeypatch.setattr(fn_class, "apply", staticmethod(lambda *a: (calls.append(fn_class.__name__), orig(*a))[1]))


@pytest.mark.parametrize("case", EDGE_CASES + ASPP_CASES + [FULL_SIZE])
def test_dilated_convolution_any_rate_matches_fp64(case):
    from test_gpu_conv3x3_sb import _bound
    from contrastiveseg_amd import kernels as K
    B, ci, co, H, W, d = case
    g = torch.Generator().manual_seed(41 + W + d)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)
    b = torch.randn(co, generator=g)
    dy = torch.randn(B, co, H, W, generator=g)
    dev = torch.device("cuda:0")
    # float64 on the device (the full-size case is 1.3 TFLOP per direction: minutes on the host)
    x64, w64, b64 = (t.to(dev).double().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv2d(x64, w64, b64, 1, d, d)
    y64.backward(dy.to(dev).double())
    ref = {"y": y64.detach().cpu(), "dx": x64.grad.cpu(), "dw": w64.grad.cpu(), "db": b64.grad.cpu()}
    del x64, w64, b64, y64
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    assert K.conv3x3_dilany_eligible(xd, wd, (d, d))
    y = K.conv3x3_dilany_split(xd, wd, bd, d)
    y.backward(dy.to(dev))
    got = {"y": y.detach().cpu(), "dx": xd.grad.cpu(), "dw": wd.grad.cpu(), "db": bd.grad.cpu()}
    del xd, y
    xr, wr, br = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    yr = F.conv2d(xr, wr, br, 1, d, d)
    yr.backward(dy.to(dev))
    lib = {"y": yr.detach().cpu(), "dx": xr.grad.cpu(), "dw": wr.grad.cpu(), "db": br.grad.cpu()}
    figures = {}
    for name in ("y", "dx", "dw", "db"):
        err, tol = _bound(ref[name], got[name], lib[name])
        figures[name] = (err, tol, float((lib[name].double() - ref[name]).abs().max()), float(ref[name].abs().max()))
    print("dilany", case, {k: "err %.2e bound %.2e library %.2e scale %.2e" % v for k, v in figures.items()})
    for name, (err, tol, _, _) in figures.items():
        assert err <= tol, (case, name, err, tol)


def test_weight_gradient_is_deterministic():
    from contrastiveseg_amd import kernels as K
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 512, 33, 65, generator=g).to(dev)
    dy = torch.randn(2, 256, 33, 65, generator=g).to(dev)
    a = K.conv3x3_dilany_wrw(x, dy, 12)
    for _ in range(3):
        assert torch.equal(a, K.conv3x3_dilany_wrw(x, dy, 12))


def test_entry_points_refuse_shapes_outside_the_contract():
    import ctypes
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    t = torch.zeros(1 << 14, device=dev)
    rec = torch.zeros(K.AMAX_WORDS, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    for cin, cout, dil in ((24, 64, 12), (64, 80, 12), (64, 64, 0)):
        assert lib.cseg_conv3x3_split_dilany_fwd(p(t), p(t), None, None, 1, cin, cout, 4, 8, dil, p(rec), p(rec), p(t), None, None) == 0
        assert b"conv3x3_dilany" in lib.cseg_last_error()
    assert lib.cseg_conv3x3_split_dilany_wrw(p(t), p(t), 1, 24, 64, 4, 8, 12, p(rec), p(rec), p(t), p(t), None) == 0
    assert lib.cseg_conv3x3_split_dilany_wrw_ws_floats(1, 24, 64, 4, 8, 12) == 0


@pytest.mark.parametrize("name", ["deeplab_v3_contrast", "deeplab_v3_contrast_train"])
def test_deeplab_model_golden_with_the_route_on(name, golden_dir, monkeypatch):
    """tests/test_models_golden.py's GPU leg for the DeepLab fixtures with CSEG_CONV3X3_DIL_ANY on: the same 1e-3 absolute bar, and
    ASPP's three dilated branches must have taken Conv3x3DilAny."""
    from oracle.make_golden import MODEL_CASES
    from test_models_golden import _build, _check, _forward
    from contrastiveseg_amd import kernels as K
    c = MODEL_CASES[name]
    g = np.load(os.path.join(golden_dir, "model_%s.npz" % name))
    assert os.environ.get("MIOPEN_USER_DB_PATH"), "the shipped MIOpen solver records must be active (as in bench.py)"
    torch.backends.cudnn.benchmark = False
    monkeypatch.setattr(K, "CONV3X3_DIL_ANY", True)
    calls = []
    _count(monkeypatch, K.Conv3x3DilAny, calls)
    net = _build(name, c).cuda()
    out = _forward(net, c, "cuda")
    per_forward = 3
    assert len(calls) > 0 and len(calls) % per_forward == 0, calls        # (a primed fixture runs the network twice)
    _check(out, g, 1e-3)


def test_deeplab_step_golden_with_the_route_on(golden_dir, monkeypatch):
    """tests/test_step_golden.py's GPU leg for step_resnet50_deeplab with the route on, at that file's own bounds: ASPP on
    Conv3x3DilAny in all three directions, the rate-2/4 weight gradients of layer3 / layer4 on conv3x3_dilany_wrw."""
    from oracle.make_golden import STEP_CASES
    from test_step_golden import _compare, _run
    from contrastiveseg_amd import kernels as K
    torch.backends.cudnn.benchmark = False
    monkeypatch.setattr(K, "CONV3X3_DIL_ANY", True)
    calls = []
    _count(monkeypatch, K.Conv3x3DilAny, calls)
    orig_wrw = K.conv3x3_dilany_wrw
    monkeypatch.setattr(K, "conv3x3_dilany_wrw", lambda *a, **k: (calls.append("wrw"), orig_wrw(*a, **k))[1])
    name = "step_resnet50_deeplab"
    c = STEP_CASES[name]
    g = np.load(os.path.join(golden_dir, "%s.npz" % name))
    worst = _compare(_run(c, torch.device("cuda:0")), g, c, 1e-3, 1e-3, 8e-2)
    print(name, {k: "%.1e (bound %.1e)" % v for k, v in worst.items()})
    assert calls.count("Conv3x3DilAny") >= 3, calls
    assert calls.count("wrw") > 3, "the rate-2/4 layers' weight gradients did not take conv3x3_dilany_wrw"
