"""The classifier convolution for 33 .. 256 classes (csrc/cls1x1_wide.hip, kernels.cls1x1_wide): module_helper.FoldedDropout2d +
ClassifierConv1x1 against the reference's nn.Dropout2d + nn.Conv2d on the same device with the same generator state (same mask
draws; outputs and all gradients within fp32 summation-order noise, fp64 as the yardstick -- the rule of tests/test_gpu_cls1x1.py:
the arithmetic class is the same, an fp32 chain in another order), the raw C-ABI against fp64 einsums, determinism, the routing, and
the whole model with a 171-class head against logits of the reference itself (tests/golden/model_*_k171.part*.npz; the CPU leg of
those fixtures is tests/test_models_golden_wide.py).
Replayed on the CPU emulation by tests/test_emu_cls1x1_wide.py (all but the full-size case and the GPU model leg)."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

from tests.golden_wide_cases import WIDE_CALLS, WIDE_MODEL_CASES, load

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


CASES = [  # B, C, K, H, W, bias, dropout p
    (2, 64, 40, 5, 13, True, 0.25),        # 65 pixels: the scalar loaders of the weight gradient, a ragged pixel tile
    (1, 720, 171, 4, 36, False, 0.10),     # the HRNet head: 22 channel chunks + 16 channels, 171 of 192 columns
    (2, 512, 171, 3, 24, True, 0.0),       # the OCR classifier: bias, no dropout
    (1, 96, 150, 6, 20, False, 0.10),      # ADE20K's class count (KP = 160)
    (2, 40, 33, 8, 32, True, 0.0),         # just over the limit of the streaming kernels (KP = 64)
    (1, 48, 256, 4, 16, True, 0.5),        # the upper limit: no pad column
    (3, 50, 60, 7, 9, False, 0.10),        # Pascal-Context's class count; C and P both ragged
]
FULL_SIZE = (2, 720, 171, 130, 130, False, 0.10)       # the benched feature size: 16 900 pixels, not a multiple of 128 (GPU only)


def _count(monkeypatch, fn_class, calls):
    orig = fn_class.apply
    monkeypatch.setattr(fn_class, "apply", staticmethod(lambda *a: (calls.append(fn_class.__name__), orig(*a))[1]))


@pytest.mark.parametrize("case", CASES + [FULL_SIZE])
def test_wide_classifier_with_folded_dropout_matches_the_reference_modules(case, monkeypatch):
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.models.tools.module_helper import ClassifierConv1x1, FoldedDropout2d
    B, C, Kc, H, W, bias, p = case
    dev = _dev()
    monkeypatch.setattr(K, "CLS1X1_WIDE", True)                    # the route under test, whatever the shipped default of the switch
    g = torch.Generator().manual_seed(100 + C + Kc)
    x0 = torch.randn(B, C, H, W, generator=g).relu_()
    w0 = torch.randn(Kc, C, 1, 1, generator=g) / C ** 0.5
    b0 = torch.randn(Kc, generator=g) if bias else None
    dy0 = torch.randn(B, Kc, H, W, generator=g)

    def run(fast, dtype):
        conv = ClassifierConv1x1(C, Kc, kernel_size=1, bias=bias) if fast else nn.Conv2d(C, Kc, kernel_size=1, bias=bias)
        drop = FoldedDropout2d(p, conv) if fast else nn.Dropout2d(p)
        if dtype == torch.float64:
            # the fp64 yardstick multiplies by the mask the fp32 runs draw (see tests/test_gpu_cls1x1.py)
            torch.manual_seed(77)
            m = nn.functional.dropout2d(torch.ones(B, C, 1, 1, device=dev), p, True).double()
            drop = type("Mask", (nn.Module,), {"forward": lambda self, t: t * m})()
        net = nn.Sequential(drop, conv).to(dev).to(dtype)
        with torch.no_grad():
            conv.weight.copy_(w0.to(dtype))
            if bias:
                conv.bias.copy_(b0.to(dtype))
        net.train()
        x = x0.to(dev).to(dtype).clone().requires_grad_(True)
        torch.manual_seed(77)
        calls = []
        if fast:
            orig = K.Cls1x1Wide.apply
            monkeypatch.setattr(K.Cls1x1Wide, "apply", staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
        y = net(x)
        if fast:
            monkeypatch.setattr(K.Cls1x1Wide, "apply", orig)
            assert calls, "the classifier did not take the wide cls1x1 kernels"
        after = torch.rand(4, device=dev)                           # the generator must be where the reference leaves it
        y.backward(dy0.to(dev).to(dtype))
        return [t.detach().double().cpu() for t in (y, x.grad, conv.weight.grad) + ((conv.bias.grad,) if bias else ())] + [after.double().cpu()]

    ref64 = run(False, torch.float64)
    ref32 = run(False, torch.float32)
    got = run(True, torch.float32)
    assert torch.equal(got[-1], ref32[-1]), "the folded dropout consumed other generator draws than nn.Dropout2d"
    for name, a, r32, r64 in zip(("y", "dx", "dw", "db"), got[:-1], ref32[:-1], ref64[:-1]):
        scale = float(r64.abs().max())
        err, base = float((a - r64).abs().max()), float((r32 - r64).abs().max())
        print("%s %s: err %.3e, library fp32 %.3e, scale %.3e" % (case, name, err, base, scale))
        assert err <= max(8.0 * base, 4e-6 * scale), (name, err, base, scale)
    # zeroed channels of the mask get exactly zero gradient, as under nn.Dropout2d
    if p > 0:
        zero_ref = (ref32[1].abs().amax((2, 3)) == 0)
        assert torch.equal(got[1].abs().amax((2, 3)) == 0, zero_ref)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


RAW = [  # B, C, K, P, bias
    (2, 50, 60, 63, True),                 # C, K and P ragged; the scalar loaders
    (1, 96, 171, 144, False),
    (2, 33, 256, 40, True),                # no pad column; one channel over a chunk
    (1, 130, 33, 260, True),               # two channels over a weight-gradient channel tile; three pixel tiles
]


def _raw_inputs(case, dev):
    from contrastiveseg_amd import kernels as K
    B, C, Kc, P, bias = case
    KP = K.cls1x1_wide_kp(Kc)
    g = torch.Generator().manual_seed(7 + C + Kc + P)
    x = torch.randn(B, C, P, generator=g)
    wt = torch.randn(B, C, KP, generator=g) / C ** 0.5
    wt[:, :, Kc:] = 0
    dy = torch.randn(B, Kc, P, generator=g)
    b = torch.randn(Kc, generator=g) if bias else None
    return KP, x.to(dev), wt.to(dev), dy.to(dev), (b.to(dev) if bias else None)


def _raw_run(case, dev):
    """The four entry points once: y (with a guard region behind it), dx, dwt."""
    from contrastiveseg_amd import _hip
    B, C, Kc, P, _ = case
    KP, x, wt, dy, b = _raw_inputs(case, dev)
    GUARD = 4096
    ybuf = torch.full((B * Kc * P + GUARD,), -7.0, device=dev)
    _hip.call("cseg_cls1x1_wide_fwd", _ptr(x), _ptr(wt), _ptr(b) if b is not None else None, B, C, Kc, KP, ctypes.c_long(P), _ptr(ybuf),
              _hip.stream_ptr())
    dx = torch.full((B, C, P), float("nan"), device=dev)
    _hip.call("cseg_cls1x1_wide_bwd", _ptr(dy), _ptr(wt), B, C, Kc, KP, ctypes.c_long(P), _ptr(dx), _hip.stream_ptr())
    n = _hip.lib().cseg_cls1x1_wide_wrw_ws_floats(B, C, KP, ctypes.c_long(P))
    assert n > 0
    ws = torch.full((n,), float("nan"), device=dev)
    dwt = torch.full((B, C, KP), float("nan"), device=dev)
    _hip.call("cseg_cls1x1_wide_wrw", _ptr(x), _ptr(dy), B, C, Kc, KP, ctypes.c_long(P), _ptr(ws), _ptr(dwt), _hip.stream_ptr())
    return ybuf.cpu(), dx.cpu(), dwt.cpu()


@pytest.mark.parametrize("case", RAW)
def test_wide_entry_points_match_fp64_einsums(case):
    B, C, Kc, P, bias = case
    dev = _dev()
    KP, x, wt, dy, b = _raw_inputs(case, dev)
    ybuf, dx, dwt = _raw_run(case, dev)
    x, wt, dy = x.double().cpu(), wt.double().cpu(), dy.double().cpu()
    y64 = torch.einsum("bck,bcp->bkp", wt[:, :, :Kc], x) + (b.double().cpu().view(1, Kc, 1) if bias else 0)
    dx64 = torch.einsum("bck,bkp->bcp", wt[:, :, :Kc], dy)
    dw64 = torch.einsum("bcp,bkp->bck", x, dy)
    assert bool((ybuf[B * Kc * P:] == -7.0).all()), "the forward wrote behind y"
    y = ybuf[:B * Kc * P].view(B, Kc, P).double()
    # an fp32 chain of n terms against fp64: n * 2^-24 * sum |a b| is the worst case; random signs give ~ sqrt(n). Bound: 4e-6 of the
    # largest magnitude, the floor of the module test (2^-24 = 6e-8: 64 ulp)
    for name, a, r in (("y", y, y64), ("dx", dx.double(), dx64), ("dwt", dwt[:, :, :Kc].double(), dw64)):
        err, scale = float((a - r).abs().max()), float(r.abs().max())
        print("%s %s: err %.3e scale %.3e" % (case, name, err, scale))
        assert err <= 4e-6 * scale, (name, err, scale)
    assert bool((dwt[:, :, Kc:] == 0).all()), "pad columns of dwt must be exactly zero"


def test_wide_entry_points_are_deterministic():
    dev = _dev()
    for case in RAW[:2]:
        a, b = _raw_run(case, dev), _raw_run(case, dev)
        for s, t in zip(a, b):
            assert torch.equal(s, t)


def test_wide_entry_points_refuse_other_shapes():
    from contrastiveseg_amd import _hip
    dev = _dev()
    lib = _hip.lib()
    t = torch.zeros(1 << 16, device=dev)
    for Kc, KP in ((32, 32), (257, 288), (171, 176), (171, 256), (40, 32)):
        B, C, P = 1, 8, 16
        assert lib.cseg_cls1x1_wide_fwd(_ptr(t), _ptr(t), None, B, C, Kc, KP, ctypes.c_long(P), _ptr(t), None) == 0
        assert b"cls1x1_wide_fwd" in lib.cseg_last_error()
        assert lib.cseg_cls1x1_wide_bwd(_ptr(t), _ptr(t), B, C, Kc, KP, ctypes.c_long(P), _ptr(t), None) == 0
        assert b"cls1x1_wide_bwd" in lib.cseg_last_error()
        assert lib.cseg_cls1x1_wide_wrw(_ptr(t), _ptr(t), B, C, Kc, KP, ctypes.c_long(P), _ptr(t), _ptr(t), None) == 0
        assert b"cls1x1_wide_wrw" in lib.cseg_last_error()
    assert lib.cseg_cls1x1_wide_wrw_ws_floats(1, 8, 32, ctypes.c_long(16)) == 0
    assert lib.cseg_cls1x1_wide_wrw_ws_floats(1, 8, 288, ctypes.c_long(16)) == 0
    assert lib.cseg_cls1x1_wide_wrw_ws_floats(1, 8, 176, ctypes.c_long(16)) == 0


def test_wide_routing(monkeypatch):
    """257 classes / the switch off: the reference's modules; 19 classes: the streaming kernels, as before."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.models.tools.module_helper import ClassifierConv1x1, FoldedDropout2d
    dev = _dev()
    calls = []
    _count(monkeypatch, K.Cls1x1, calls)
    _count(monkeypatch, K.Cls1x1Wide, calls)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 24, 4, 16, generator=g).to(dev)
    assert K.cls1x1_wide_kp(33) == K.cls1x1_wide_kp(64) and K.cls1x1_wide_kp(171) >= 171 and K.cls1x1_wide_kp(256) == 256

    def both(Kc):
        conv = ClassifierConv1x1(24, Kc, kernel_size=1, bias=True).to(dev)
        net = nn.Sequential(FoldedDropout2d(0.5, conv), conv).to(dev).train()
        ref = nn.Sequential(nn.Dropout2d(0.5), nn.Conv2d(24, Kc, kernel_size=1, bias=True)).to(dev).train()
        ref[1].load_state_dict(conv.state_dict())
        torch.manual_seed(3)
        mid = net[0](x)
        a = net[1](mid)
        torch.manual_seed(3)
        b = ref(x)
        return conv, mid, a, b

    monkeypatch.setattr(K, "CLS1X1_WIDE", True)
    conv, mid, a, b = both(257)
    assert calls == [] and not K.cls1x1_wide_eligible(x, conv.weight) and not K.cls1x1_eligible(x, conv.weight)
    assert getattr(mid, "_cseg_drop_mask", None) is None and torch.equal(a, b)        # nn.Dropout2d multiplied; the same convolution
    monkeypatch.setattr(K, "CLS1X1_WIDE", False)
    conv, mid, a, b = both(171)
    assert calls == [] and not K.cls1x1_wide_eligible(x, conv.weight)
    assert getattr(mid, "_cseg_drop_mask", None) is None and torch.equal(a, b)
    monkeypatch.setattr(K, "CLS1X1_WIDE", True)
    conv, mid, a, b = both(171)
    assert calls == ["Cls1x1Wide"] and K.cls1x1_wide_eligible(x, conv.weight) and not K.cls1x1_eligible(x, conv.weight)
    assert getattr(mid, "_cseg_drop_mask", None) is not None and float((a - b).detach().abs().max()) <= 1e-5
    del calls[:]
    conv, mid, a, b = both(19)
    assert calls == ["Cls1x1"] and K.cls1x1_eligible(x, conv.weight) and not K.cls1x1_wide_eligible(x, conv.weight)
    assert float((a - b).detach().abs().max()) <= 1e-5


@pytest.mark.parametrize("name", list(WIDE_MODEL_CASES))
def test_wide_model_forward_gpu_matches_reference(name, golden_dir, monkeypatch):
    """The whole model with a 171-class head on the product path against the reference's logits: absolute 1e-3 (the north_star bar)."""
    from test_models_golden import _build, _check, _forward
    from contrastiveseg_amd import kernels as K
    c = WIDE_MODEL_CASES[name]
    g = load(golden_dir, name)
    assert os.environ.get("MIOPEN_USER_DB_PATH"), "the shipped MIOpen solver records must be active (as in bench.py)"
    torch.backends.cudnn.benchmark = False
    calls = []
    monkeypatch.setattr(K, "CLS1X1_WIDE", True)
    _count(monkeypatch, K.Cls1x1Wide, calls)
    out = _forward(_build(name, c).cuda(), c, "cuda")
    assert len(calls) == WIDE_CALLS[name], calls
    _check(out, g, 1e-3)
