"""The fused object-context kernels (csrc/ocr.hip, kernels.OcrGather / kernels.OcrAttention, CSEG_OCR_FUSED=1) against the torch
composition lib/models/modules/spatial_ocr_block.py runs with the switch off: outputs and all gradients within fp32 summation-order
noise with fp64 as the yardstick (the rule of tests/test_gpu_cls1x1_wide.py: err <= max(8 x the library's own fp32 error, 4e-6 x
max|truth|) per tensor), the raw C-ABI against fp64 einsum + softmax with guard regions behind every output, determinism, refusals, what
autograd keeps between forward and backward, the routing of the two modules, the whole OCR model against logits of the reference, one
SGD step against the reference's step golden, and capture into a graph.
Replayed on the CPU emulation by tests/test_emu_ocr_fused.py (all but the large shapes, the model legs and the capture)."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _ref_attention(q, key, value, scale):
    """ObjectAttentionBlock2D.forward between f_pixel / f_object / f_down and f_up, as it stands with the switch off."""
    b, c, h, w = q.shape
    query = q.reshape(b, c, -1).permute(0, 2, 1)
    sim = F.softmax(scale * torch.matmul(query, key), dim=-1)
    return torch.matmul(sim, value.permute(0, 2, 1)).permute(0, 2, 1).contiguous().reshape(b, c, h, w)


def _ref_gather(feats, probs, scale):
    """SpatialGather_Module.forward as it stands with the switch off."""
    b, k = probs.shape[:2]
    probs = F.softmax(scale * probs.reshape(b, k, -1), dim=2)
    feats = feats.reshape(b, feats.shape[1], -1).permute(0, 2, 1)
    return torch.matmul(probs, feats).permute(0, 2, 1).unsqueeze(3)


def _count(monkeypatch, fn_class, calls, backward=False):
    orig = fn_class.apply
    monkeypatch.setattr(fn_class, "apply", staticmethod(lambda *a: (calls.append(fn_class.__name__), orig(*a))[1]))
    if backward:
        orig_b = fn_class.backward
        monkeypatch.setattr(fn_class, "backward", staticmethod(lambda *a: (calls.append(fn_class.__name__ + ".backward"), orig_b(*a))[1]))


def _grads(fn, inputs, dout, dev, dtype):
    xs = [t.to(dev).to(dtype).clone().requires_grad_(True) for t in inputs]
    y = fn(*xs)
    gs = torch.autograd.grad(y, xs, dout.to(dev).to(dtype).reshape(y.shape))
    return [t.detach().double().cpu() for t in (y,) + tuple(gs)]


def _parity(tag, names, fused, ref, inputs, dout, dev):
    """The rule of tests/test_gpu_cls1x1_wide.py:90 per tensor; err / library fp32 / scale printed for every tensor."""
    truth = _grads(ref, inputs, dout, dev, torch.float64)
    base = _grads(ref, inputs, dout, dev, torch.float32)
    got = _grads(fused, inputs, dout, dev, torch.float32)
    for name, a, r32, r64 in zip(names, got, base, truth):
        assert a.shape == r64.shape, (name, a.shape, r64.shape)
        assert bool(torch.isfinite(a).all()), (tag, name, "not finite")
        scale = float(r64.abs().max())
        err, b = float((a - r64).abs().max()), float((r32 - r64).abs().max())
        print("%s %s: err %.3e, library fp32 %.3e, scale %.3e, err / bound %.3f" % (tag, name, err, b, scale, err / max(8.0 * b, 4e-6 * scale)))
        assert err <= max(8.0 * b, 4e-6 * scale), (tag, name, err, b, scale)


ATTN = [  # B, C, K, H, W, sharp
    (2, 256, 171, 5, 13, False),           # 65 pixels: one ragged pixel tile; 21 masked pad classes
    (1, 256, 19, 4, 36, False),            # Cityscapes: KP = 64, 45 pad classes (masking dominates)
    (2, 40, 33, 8, 32, False),             # one channel chunk + 8 channels; first K above 32
    (1, 48, 256, 4, 16, False),            # no pad class
    (3, 50, 60, 7, 9, False),              # C, K and P all ragged
    (1, 256, 150, 9, 33, False),           # 297 pixels: two full pixel tiles and a ragged one
    (1, 64, 2, 3, 11, False),              # smallest K
    (2, 256, 171, 5, 13, True),            # q scaled so that the scaled logits reach +-60: near one-hot, needs the max subtraction
]
ATTN_FULL = (2, 256, 171, 130, 130, False)             # the benched feature size: 16 900 pixels, not a multiple of 128 (GPU only)

GATHER = [  # B, C, K, H, W, factor on probs
    (2, 64, 40, 5, 13, 1.0),
    (1, 512, 171, 4, 36, 1.0),
    (1, 96, 19, 6, 20, 1.0),
    (1, 48, 256, 4, 16, 1.0),
    (3, 50, 60, 7, 9, 1.0),
    (1, 130, 33, 10, 52, 1.0),             # two channels over a 128-channel tile; 520 pixels: several stages, an uneven pixel split
    (2, 64, 40, 5, 13, 30.0),              # scores x 30: a softmax over the pixels that is near one-hot
]
GATHER_FULL = (2, 512, 171, 130, 130, 1.0)


def _attn_inputs(case):
    B, C, Kc, H, W, sharp = case
    g = torch.Generator().manual_seed(300 + C + Kc + H * W)
    q = torch.randn(B, C, H, W, generator=g).relu_()              # f_pixel ends in a ReLU
    key = torch.randn(B, C, Kc, generator=g).relu_()
    value = torch.randn(B, C, Kc, generator=g).relu_()
    dout = torch.randn(B, C, H, W, generator=g)
    scale = C ** -0.5
    if sharp:
        q = q - 0.5                                                # both signs
        top = float((scale * torch.einsum("bcp,bck->bkp", q.reshape(B, C, -1).double(), key.double())).abs().max())
        q = q * (60.0 / top)
    return q, key, value, dout, scale


@pytest.mark.parametrize("case", ATTN + [ATTN_FULL])
def test_fused_attention_matches_the_torch_composition(case, monkeypatch):
    from contrastiveseg_amd import kernels as K
    monkeypatch.setattr(K, "OCR_FUSED", True)
    q, key, value, dout, scale = _attn_inputs(case)
    assert K.ocr_fused_eligible(q.to(_dev()), case[2], key.to(_dev()), value.to(_dev()))
    _parity(case, ("out", "dq", "dkey", "dvalue"), lambda a, b, c: K.ocr_attention(a, b, c, scale),
            lambda a, b, c: _ref_attention(a, b, c, scale), (q, key, value), dout, _dev())


def _gather_inputs(case):
    B, C, Kc, H, W, factor = case
    g = torch.Generator().manual_seed(500 + C + Kc + H * W)
    feats = torch.randn(B, C, H, W, generator=g).relu_()
    probs = torch.randn(B, Kc, H, W, generator=g) * factor
    dctx = torch.randn(B, C, Kc, 1, generator=g)
    return feats, probs, dctx


@pytest.mark.parametrize("case", GATHER + [GATHER_FULL])
def test_fused_gather_matches_the_torch_composition(case, monkeypatch):
    from contrastiveseg_amd import kernels as K
    monkeypatch.setattr(K, "OCR_FUSED", True)
    feats, probs, dctx = _gather_inputs(case)
    _parity(case, ("ctx", "dfeats", "dprobs"), lambda a, b: K.ocr_gather(a, b, 1.0), lambda a, b: _ref_gather(a, b, 1.0),
            (feats, probs), dctx, _dev())


# ---- the raw C-ABI ------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


RAW = [  # B, C, K, P, scale
    (2, 50, 60, 63, 0.5),                  # C, K and P ragged; the scalar loaders
    (1, 96, 171, 144, 0.25),
    (2, 33, 256, 40, 1.0),                 # no pad class; one channel over a chunk
    (1, 130, 33, 260, 0.3),                # two channels over a 128-channel tile; three pixel tiles
    (1, 40, 19, 70, 1.0),                  # KP = 64 for 19 classes
]
GUARD = 4096


def _raw_inputs(case, dev):
    B, C, Kc, P, scale = case
    g = torch.Generator().manual_seed(11 + C + Kc + P)
    t = {"q": torch.randn(B, C, P, generator=g), "key": torch.randn(B, C, Kc, generator=g), "value": torch.randn(B, C, Kc, generator=g),
         "dout": torch.randn(B, C, P, generator=g), "probs": torch.randn(B, Kc, P, generator=g) * 3, "feats": torch.randn(B, C, P, generator=g),
         "dctx": torch.randn(B, C, Kc, generator=g)}
    return {k: v.to(dev) for k, v in t.items()}


def _guarded(n, dev):
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    buf[n:] = -7.0
    return buf


def _raw_run(case, dev):
    """Every entry point once; each output NaN-filled beforehand with a guard region behind it. -> {name: whole buffer on the CPU}"""
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    B, C, Kc, P, scale = case
    KP = K.ocr_kp(Kc)
    t = _raw_inputs(case, dev)
    lib, lp, st = _hip.lib(), ctypes.c_long(P), _hip.stream_ptr()
    sizes = {"ctx": B * C * Kc, "rstats": 2 * B * Kc, "dprobs": B * Kc * P, "dfeats": B * C * P, "out": B * C * P, "stats": 2 * B * P,
             "dq": B * C * P, "dkey": B * C * Kc, "dvalue": B * C * Kc, "out_nostats": B * C * P, "ctx_nostats": B * C * Kc}
    o = {k: _guarded(n, dev) for k, n in sizes.items()}
    n = lib.cseg_ocr_gather_ws_floats(B, C, Kc, KP, lp)
    assert n > 0
    ws = torch.full((n,), float("nan"), device=dev)
    _hip.call("cseg_ocr_gather_fwd", _ptr(t["probs"]), _ptr(t["feats"]), scale, B, C, Kc, KP, lp, _ptr(ws), _ptr(o["rstats"]), _ptr(o["ctx"]), st)
    _hip.call("cseg_ocr_gather_fwd", _ptr(t["probs"]), _ptr(t["feats"]), scale, B, C, Kc, KP, lp, _ptr(ws), None, _ptr(o["ctx_nostats"]), st)
    _hip.call("cseg_ocr_gather_bwd", _ptr(t["probs"]), _ptr(t["feats"]), _ptr(o["rstats"]), _ptr(t["dctx"]), scale, B, C, Kc, KP, lp,
              _ptr(o["dprobs"]), _ptr(o["dfeats"]), st)
    _hip.call("cseg_ocr_attn_fwd", _ptr(t["q"]), _ptr(t["key"]), _ptr(t["value"]), scale, B, C, Kc, KP, lp, _ptr(o["out"]), _ptr(o["stats"]), st)
    _hip.call("cseg_ocr_attn_fwd", _ptr(t["q"]), _ptr(t["key"]), _ptr(t["value"]), scale, B, C, Kc, KP, lp, _ptr(o["out_nostats"]), None, st)
    n = lib.cseg_ocr_attn_bwd_ws_floats(B, C, Kc, KP, lp)
    assert n > 0
    ws2 = torch.full((n,), float("nan"), device=dev)
    _hip.call("cseg_ocr_attn_bwd", _ptr(t["q"]), _ptr(t["key"]), _ptr(t["value"]), _ptr(o["stats"]), _ptr(t["dout"]), scale, B, C, Kc, KP,
              lp, _ptr(ws2), _ptr(o["dq"]), _ptr(o["dkey"]), _ptr(o["dvalue"]), st)
    return {k: v.cpu() for k, v in o.items()}, sizes


@pytest.mark.parametrize("case", RAW)
def test_ocr_entry_points_match_fp64_einsums(case):
    B, C, Kc, P, scale = case
    dev = _dev()
    o, sizes = _raw_run(case, dev)
    t = {k: v.double().cpu() for k, v in _raw_inputs(case, dev).items()}
    for v in t.values():
        v.requires_grad_(True)
    s = torch.softmax(scale * t["probs"], dim=2)
    ctx = torch.einsum("bkp,bcp->bck", s, t["feats"])
    dfeats, dprobs = torch.autograd.grad(ctx, (t["feats"], t["probs"]), t["dctx"].detach())
    a = torch.softmax(scale * torch.einsum("bck,bcp->bkp", t["key"], t["q"]), dim=1)
    out = torch.einsum("bck,bkp->bcp", t["value"], a)
    dq, dkey, dvalue = torch.autograd.grad(out, (t["q"], t["key"], t["value"]), t["dout"].detach())
    want = {"ctx": ctx, "dfeats": dfeats, "dprobs": dprobs, "out": out, "dq": dq, "dkey": dkey, "dvalue": dvalue, "out_nostats": out,
            "ctx_nostats": ctx}
    for name, buf in o.items():
        assert bool((buf[sizes[name]:] == -7.0).all()), "%s: written behind the output" % name
        assert bool(torch.isfinite(buf[:sizes[name]]).all()), "%s: not every element was written" % name
    # Each result is one or two chained fp32 fmaf chains of at most a few hundred terms (1e-7 of sum |a b| each, section 14 of
    # DESIGN.md) around an exponential that is good to a few ulp for arguments in [-20, 0]: the 64 ulp floor of the module tests
    for name, r in want.items():
        got = o[name][:sizes[name]].double().view(r.shape)
        err, sc = float((got - r.detach()).abs().max()), float(r.detach().abs().max())
        print("%s %s: err %.3e scale %.3e" % (case, name, err, sc))
        assert err <= 4e-6 * sc, (name, err, sc)
    assert torch.equal(o["out"][:sizes["out"]], o["out_nostats"][:sizes["out"]])          # the statistics are a by-product only
    assert torch.equal(o["ctx"][:sizes["ctx"]], o["ctx_nostats"][:sizes["ctx"]])
    # the statistics themselves: max and sum of exp of the scaled scores
    rs = o["rstats"][:2 * B * Kc].double().view(2, B, Kc)
    m64 = (scale * t["probs"].detach()).amax(2)
    assert float((rs[0] - m64).abs().max()) <= 1e-6 * float(m64.abs().max())
    z64 = torch.exp(scale * t["probs"].detach() - m64.unsqueeze(2)).sum(2)
    assert float((rs[1] / z64 - 1).abs().max()) <= 4e-6


def test_ocr_entry_points_are_deterministic():
    dev = _dev()
    for case in (RAW[0], RAW[1], RAW[3]):                          # RAW[3]: two channel tiles, an uneven split of the pixel stages
        (a, _), (b, _) = _raw_run(case, dev), _raw_run(case, dev)
        for name in a:
            assert torch.equal(a[name], b[name]), name


def test_ocr_entry_points_refuse_other_shapes():
    from contrastiveseg_amd import _hip
    dev = _dev()
    lib = _hip.lib()
    t = torch.zeros(1 << 16, device=dev)
    p = _ptr(t)
    for Kc, KP in ((1, 64), (257, 288), (171, 176), (171, 256), (40, 32), (19, 32), (0, 64)):
        B, C, P = 1, 8, ctypes.c_long(16)
        assert lib.cseg_ocr_gather_fwd(p, p, 1.0, B, C, Kc, KP, P, p, p, p, None) == 0
        assert b"ocr_gather_fwd" in lib.cseg_last_error()
        assert lib.cseg_ocr_gather_bwd(p, p, p, p, 1.0, B, C, Kc, KP, P, p, p, None) == 0
        assert b"ocr_gather_bwd" in lib.cseg_last_error()
        assert lib.cseg_ocr_attn_fwd(p, p, p, 1.0, B, C, Kc, KP, P, p, p, None) == 0
        assert b"ocr_attn_fwd" in lib.cseg_last_error()
        assert lib.cseg_ocr_attn_bwd(p, p, p, p, p, 1.0, B, C, Kc, KP, P, p, p, p, p, None) == 0
        assert b"ocr_attn_bwd" in lib.cseg_last_error()
        assert lib.cseg_ocr_gather_ws_floats(B, C, Kc, KP, P) == 0
        assert lib.cseg_ocr_attn_bwd_ws_floats(B, C, Kc, KP, P) == 0
    assert bool((t == 0).all())
    assert lib.cseg_ocr_gather_ws_floats(1, 8, 171, 192, ctypes.c_long(16)) > 0


def test_nothing_of_the_size_of_the_map_is_saved_for_backward(monkeypatch):
    """No B x K x P tensor survives the forward pass: the inputs and the softmax statistics are all autograd holds."""
    from contrastiveseg_amd import kernels as K
    monkeypatch.setattr(K, "OCR_FUSED", True)
    dev = _dev()
    B, C, Kc, H, W = 2, 40, 171, 5, 13
    P = H * W
    g = torch.Generator().manual_seed(1)
    q, key, value = (torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in ((B, C, H, W), (B, C, Kc), (B, C, Kc)))
    out = K.ocr_attention(q, key, value, C ** -0.5)
    assert sum(t.numel() for t in out.grad_fn.saved_tensors) <= q.numel() + key.numel() + value.numel() + 2 * B * P
    feats, probs = (torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in ((B, C, H, W), (B, Kc, H, W)))
    ctx = K.ocr_gather(feats, probs, 1.0)
    assert sum(t.numel() for t in ctx.grad_fn.saved_tensors) <= feats.numel() + probs.numel() + 2 * B * Kc
    from contrastiveseg_amd import _hip
    seen, orig = {}, _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (seen.__setitem__(name, a), orig(name, *a))[1])
    with torch.no_grad():                                           # the validation pass: same numbers, no statistics, nothing kept
        out2, ctx2 = K.ocr_attention(q, key, value, C ** -0.5), K.ocr_gather(feats, probs, 1.0)
    monkeypatch.setattr(_hip, "call", orig)
    assert seen["cseg_ocr_attn_fwd"][10].value is None and seen["cseg_ocr_gather_fwd"][9].value is None
    assert out2.grad_fn is None and ctx2.grad_fn is None and torch.equal(out2, out.detach()) and torch.equal(ctx2, ctx.detach())


def _modules(dev, cin, ck):
    from contrastiveseg_amd.lib.models.modules.spatial_ocr_block import ObjectAttentionBlock2D, SpatialGather_Module
    torch.manual_seed(9)
    return SpatialGather_Module(0).to(dev), ObjectAttentionBlock2D(cin, ck, 1, bn_type="torchsyncbn").to(dev).train()


def test_ocr_routing(monkeypatch):
    """Switch off, 257 classes, CPU tensors: the torch lines, bit for bit. Switch on at 171 and at 19 classes: each module runs its
    Function exactly once, under torch.no_grad() too."""
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    calls = []
    _count(monkeypatch, K.OcrGather, calls)
    _count(monkeypatch, K.OcrAttention, calls)
    cin, ck, H, W, B = 64, 64, 4, 16, 2
    gather, attn = _modules(dev, cin, ck)
    g = torch.Generator().manual_seed(5)

    def present_lines(x, probs):
        proxy = _ref_gather(x, probs, 1)
        b = x.shape[0]
        key = attn.f_object(proxy).reshape(b, ck, -1)
        value = attn.f_down(proxy).reshape(b, ck, -1)
        return proxy, attn.f_up(_ref_attention(attn.f_pixel(x), key, value, ck ** -.5))

    def both(Kc, device):
        x = torch.randn(B, cin, H, W, generator=g).to(device)
        probs = torch.randn(B, Kc, H, W, generator=g).to(device)
        torch.manual_seed(3)
        proxy = gather(x, probs)
        y = attn(x, proxy)
        torch.manual_seed(3)
        rp, ry = present_lines(x, probs)
        return proxy, y, rp, ry

    monkeypatch.setattr(K, "OCR_FUSED", False)
    proxy, y, rp, ry = both(171, dev)
    assert calls == [] and torch.equal(proxy, rp) and torch.equal(y, ry)
    monkeypatch.setattr(K, "OCR_FUSED", True)
    proxy, y, rp, ry = both(257, dev)
    assert calls == [] and torch.equal(proxy, rp) and torch.equal(y, ry)
    if dev.type == "cuda":                                      # (on the emulated device the CPU is the device)
        # (the block's convolutions and BatchNorms have no CPU path in the product, so the attention runs between identities there)
        from contrastiveseg_amd.lib.models.modules.spatial_ocr_block import ObjectAttentionBlock2D
        xc, pc = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 171, H, W, generator=g)
        proxy = gather(xc, pc)
        bare = ObjectAttentionBlock2D(cin, cin, 1, bn_type="torchsyncbn")
        bare.f_pixel = bare.f_object = bare.f_down = bare.f_up = torch.nn.Identity()
        yc = bare(xc, proxy)
        assert calls == [] and torch.equal(proxy, _ref_gather(xc, pc, 1)) and not K.ocr_fused_eligible(xc, 171, proxy)
        assert torch.equal(yc, _ref_attention(xc, proxy.reshape(B, cin, -1), proxy.reshape(B, cin, -1), cin ** -.5))
    for Kc in (171, 19):
        del calls[:]
        proxy, y, rp, ry = both(Kc, dev)
        assert calls == ["OcrGather", "OcrAttention"], calls
        assert tuple(proxy.shape) == (B, cin, Kc, 1) and float((proxy - rp).abs().max()) <= 1e-5 * float(rp.abs().max())
        assert float((y - ry).detach().abs().max()) <= 1e-4 * max(1.0, float(ry.detach().abs().max()))
        del calls[:]
        with torch.no_grad():
            both(Kc, dev)
        assert calls == ["OcrGather", "OcrAttention"], calls


# ---- the whole model, one SGD step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hrnet_w48_ocr_contrast_k171", "hrnet_w48_ocr_contrast"])
def test_ocr_model_forward_gpu_matches_reference(name, golden_dir, monkeypatch):
    """The OCR model with the fused block against the reference's logits: absolute 1e-3, the bar these fixtures carry."""
    from test_models_golden import _build, _check, _forward
    from oracle.make_golden import MODEL_CASES
    from tests.golden_wide_cases import WIDE_MODEL_CASES, load
    from contrastiveseg_amd import kernels as K
    if name in WIDE_MODEL_CASES:
        c, g = WIDE_MODEL_CASES[name], load(golden_dir, name)
    else:
        c, g = MODEL_CASES[name], np.load(os.path.join(golden_dir, "model_%s.npz" % name))
    assert os.environ.get("MIOPEN_USER_DB_PATH"), "the shipped MIOpen solver records must be active (as in bench.py)"
    torch.backends.cudnn.benchmark = False
    calls = []
    monkeypatch.setattr(K, "OCR_FUSED", True)
    _count(monkeypatch, K.OcrGather, calls)
    _count(monkeypatch, K.OcrAttention, calls)
    out = _forward(_build(name, c).cuda(), c, "cuda")
    assert "OcrGather" in calls and "OcrAttention" in calls, calls
    _check(out, g, 1e-3)


def test_ocr_sgd_step_gpu_matches_reference(golden_dir, monkeypatch):
    """step_hrnet48_ocr with the fused block: the bars of tests/test_step_golden.py::test_sgd_step_gpu_matches_reference."""
    from test_step_golden import _compare, _run
    from oracle.make_golden import STEP_CASES
    from contrastiveseg_amd import kernels as K
    torch.backends.cudnn.benchmark = False
    calls = []
    monkeypatch.setattr(K, "OCR_FUSED", True)
    _count(monkeypatch, K.OcrGather, calls, backward=True)
    _count(monkeypatch, K.OcrAttention, calls, backward=True)
    c = STEP_CASES["step_hrnet48_ocr"]
    g = np.load(os.path.join(golden_dir, "step_hrnet48_ocr.npz"))
    worst = _compare(_run(c, torch.device("cuda:0")), g, c, 1e-3, 1e-3, 8e-2)
    print({k: "%.1e (bound %.1e)" % v for k, v in worst.items()})
    assert "OcrGather.backward" in calls and "OcrAttention.backward" in calls, calls


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_ocr_modules_capture_into_a_graph(monkeypatch):
    """Forward + backward of SpatialGather_Module and ObjectAttentionBlock2D on one stream, captured once, replayed twice: each replay
    equals the eager result bit for bit (no host synchronisation, no allocation outside torch's, no D2H in the entry points)."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.segmentor.tools import step_graph
    monkeypatch.setattr(K, "OCR_FUSED", True)
    dev = _dev()
    B, C, Kc, H, W = 2, 256, 171, 5, 13
    calls = []
    _count(monkeypatch, K.OcrGather, calls, backward=True)
    _count(monkeypatch, K.OcrAttention, calls, backward=True)
    gather, attn = _modules(dev, C, C)
    params = [p for p in attn.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, C, H, W, generator=g).to(dev).requires_grad_(True)
    probs = torch.randn(B, Kc, H, W, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(B, C, H, W, generator=g).to(dev)

    def step():
        y = attn(x, gather(x, probs))
        return (y,) + torch.autograd.grad(y, [x, probs] + params, dy)

    buffers = [(b, b.detach().clone()) for b in attn.buffers()]
    eager = [t.detach().clone() for t in step()]
    assert calls == ["OcrGather", "OcrAttention", "OcrAttention.backward", "OcrGather.backward"], calls
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    gc.collect()
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    step_graph._CAPTURING[0] = True
    try:
        with torch.cuda.stream(side):
            for _ in range(2):                                     # warm-up on the capture stream (step_graph.StepGraph._capture)
                step()
            torch.cuda.synchronize(dev)
            gc.collect()
            for t in (x, probs):
                t.__dict__.pop("_cseg_amax", None)                 # a record of the warm-up must not be baked into the graph
            K._AMAX_ARENAS.clear()
            with torch.cuda.graph(graph, stream=side):
                static = step()
    finally:
        step_graph._CAPTURING[0] = False
        K._AMAX_ARENAS.clear()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    for _ in range(2):
        for t in static:
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        for a, b in zip(static[:3], eager[:3]):                    # the output and the gradients of both inputs
            assert torch.equal(a.detach(), b)
    with torch.no_grad():
        for b, saved in buffers:
            b.copy_(saved)
