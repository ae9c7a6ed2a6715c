"""Dilated 3x3 convolutions at any rate (csrc/conv3x3_dilany.hip, kernels.conv3x3_dilany_*) on the CPU emulation of the execution
model: nine tap-shifted 1x1 GEMMs whose source pixels are validated per row and column. Forward (bias, BatchNorm statistics from the
epilogue), backward-data with an addend, the deterministic weight gradient and the autograd wrapper against torch in float64 --
every element, at the tolerances tests/test_emu_conv_stats.py / test_emu_sb_kernels.py use for the same arithmetic (3e-5 of
max|ref| for y and dx, 1e-4 for dw and db, statistics means within 2e-6 max(1, .)) -- on shapes where the rate exceeds the map,
rows are ragged and flat shifts wrap over row ends; independence of the wave schedule; the contract refusals; the routing."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.emu import inject

CASES = [  # B, Cin, Cout, H, W, d
    (1, 64, 64, 7, 33, 12),        # d > H: only the middle row of taps contributes
    (2, 128, 64, 30, 20, 24),      # d > W
    (1, 64, 128, 9, 10, 36),       # d exceeds both: the centre-tap 1x1
    (1, 256, 64, 13, 65, 12),      # ragged 65-wide rows whose flat shift wraps across row ends
    (1, 64, 48, 6, 17, 2),         # the rates conv3x3_sb16d_kernel owns, forced through the new kernel; a 48-multiple
    (1, 48, 64, 8, 36, 4),
    (1, 64, 64, 5, 16, 1),         # d = 1: plain 3x3
]


def _setup(monkeypatch):
    from contrastiveseg_amd import kernels as K
    inject.install(monkeypatch)
    monkeypatch.setattr(K, "SPLIT_ARITH", "f16x3")
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    monkeypatch.setattr(K, "CONV_EPILOGUE_STATS", True)
    return K


def _tensors(case):
    B, ci, co, H, W, d = case
    g = torch.Generator().manual_seed(17 + ci + W + d)
    x = torch.randn(B, ci, H, W, generator=g) + 0.3
    w = torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)
    b = torch.randn(co, generator=g) * 0.5
    dy = torch.randn(B, co, H, W, generator=g)
    add = torch.randn(B, ci, H, W, generator=g)
    return x, w, b, dy, add


def _close(got, ref, rel, what):
    err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
    assert err <= rel * scale, (what, err, rel * scale)


@pytest.mark.parametrize("case", CASES)
def test_all_directions_match_float64(case, monkeypatch):
    K = _setup(monkeypatch)
    B, ci, co, H, W, d = case
    x, w, b, dy, add = _tensors(case)
    assert K.conv3x3_dilany_eligible(x, w, (d, d))
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv2d(x64, w64, b64, 1, d, d)
    y64.backward(dy.double())
    y64, y64_nb = y64.detach(), F.conv2d(x.double(), w.double(), None, 1, d, d)

    # forward, with and without bias, statistics from the epilogue
    for bias, ref in ((b, y64), (None, y64_nb)):
        y = K.conv3x3_dilany_run(x, w, d, False, bias, want_stats=True)
        _close(y, ref, 3e-5, "y")
        st = K.known_tile_stats(y)
        assert st is not None and st.shape[0] == co and st.shape[2] == 4
        assert abs(float(st[:, :, 0].sum()) - co * B * H * W) < 0.5, "segment counts do not add up to the tensor"
        mi = K.bn_tiles_finalize(st, 1e-5, 0.1, torch.zeros(co), torch.ones(co), torch.tensor(0))
        yd = y.double().transpose(0, 1).reshape(co, -1)
        mean64, inv64 = yd.mean(1), 1.0 / torch.sqrt(yd.var(1, unbiased=False) + 1e-5)
        assert float((mi[:, 0].double() - mean64).abs().max()) <= 2e-6 * max(1.0, float(mean64.abs().max()))
        assert float((mi[:, 1].double() / inv64 - 1).abs().max()) <= 2e-6
    if d >= H and d >= W:                      # the result IS the centre-tap 1x1 convolution
        _close(K.conv3x3_dilany_run(x, w, d, False, b), F.conv2d(x.double(), w.double()[:, :, 1:2, 1:2], b.double()), 3e-5, "centre tap")

    # backward-data with an addend
    dx = K.conv3x3_dilany_run(dy, w, d, True, None, addend=add)
    dx_ref = x64.grad + add.double()
    err = float((dx.double() - dx_ref).abs().max())
    assert err <= 3e-5 * float(x64.grad.abs().max()), ("dx + addend", err)

    # weight gradient, twice
    dw1, dw2 = K.conv3x3_dilany_wrw(x, dy, d), K.conv3x3_dilany_wrw(x, dy, d)
    assert torch.equal(dw1, dw2), "the weight gradient is not deterministic"
    _close(dw1, w64.grad, 1e-4, "dw")

    # the autograd wrapper
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    ya = K.conv3x3_dilany_split(xa, wa, ba, d)
    ya.backward(dy)
    _close(ya.detach(), y64, 3e-5, "autograd y")
    _close(xa.grad, x64.grad, 3e-5, "autograd dx")
    _close(wa.grad, w64.grad, 1e-4, "autograd dw")
    _close(ba.grad, b64.grad, 1e-4, "autograd db")


def test_results_do_not_depend_on_the_wave_schedule(monkeypatch):
    K = _setup(monkeypatch)
    case = (1, 64, 64, 5, 21, 3)
    B, ci, co, H, W, d = case
    x, w, b, dy, add = _tensors(case)
    res = []
    for order in ("asc", "desc", "shuffle:9"):
        monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
        res.append((K.conv3x3_dilany_run(x, w, d, False, b, want_stats=True), K.conv3x3_dilany_run(dy, w, d, True, None, addend=add),
                    K.conv3x3_dilany_wrw(x, dy, d)))
    for other in res[1:]:
        for a, o in zip(res[0], other):
            assert torch.equal(a, o)
    _close(res[0][0], F.conv2d(x.double(), w.double(), b.double(), 1, d, d), 3e-5, "y")


def test_contract_refusals(monkeypatch):
    K = _setup(monkeypatch)
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd.lib.models.tools.module_helper import SplitConv2d
    lib = _hip.lib()
    monkeypatch.setattr(K, "CONV3X3_DIL_ANY", True)
    t = torch.zeros(1 << 14)
    rec = torch.zeros(K.AMAX_WORDS, dtype=torch.int32)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    # Cin % 16 != 0, an output channel count that is no multiple of 48 or 64, a rate of 0, addend together with statistics
    for (cin, cout, dil, addend, stats) in ((24, 64, 12, None, None), (64, 80, 12, None, None), (64, 64, 0, None, None), (64, 64, 12, p(t), p(t))):
        assert lib.cseg_conv3x3_split_dilany_fwd(p(t), p(t), None, addend, 1, cin, cout, 4, 8, dil, p(rec), p(rec), p(t), stats, None) == 0
        assert b"conv3x3_dilany" in lib.cseg_last_error()
    assert lib.cseg_conv3x3_split_dilany_packed_bytes(24, 64) == 0 and lib.cseg_conv3x3_split_dilany_packed_bytes(64, 80) == 0
    assert lib.cseg_conv3x3_split_dilany_packed_bytes(64, 64) == 2 * 4 * 9 * 2 * 64 * 16
    assert lib.cseg_conv3x3_split_dilany_pack(p(t), 64, 24, 0, p(rec), p(t), None) == 0 and b"conv3x3_dilany" in lib.cseg_last_error()
    assert lib.cseg_conv3x3_split_dilany_wrw_ws_floats(1, 24, 64, 4, 8, 12) == 0
    assert lib.cseg_conv3x3_split_dilany_wrw(p(t), p(t), 1, 24, 64, 4, 8, 12, p(rec), p(rec), p(t), p(t), None) == 0
    assert b"conv3x3_dilany_wrw" in lib.cseg_last_error()
    assert lib.cseg_conv3x3_split_dilany_wrw(p(t), p(t), 1, 64, 64, 4, 8, 12, None, p(rec), p(t), p(t), None) == 0
    x = torch.randn(1, 24, 6, 8)
    assert not K.conv3x3_dilany_eligible(x, torch.randn(64, 24, 3, 3), (12, 12))
    with pytest.raises(RuntimeError, match="unsupported channel counts"):
        K.conv3x3_dilany_run(x, torch.randn(64, 24, 3, 3), 12)
    with pytest.raises(RuntimeError, match="groups 1 only"):
        K.conv3x3_dilany_run(torch.randn(1, 64, 6, 8), torch.randn(64, 32, 3, 3), 12)          # the weight of a groups = 2 convolution
    with pytest.raises(RuntimeError, match="conv3x3_dilany_wrw"):
        K.conv3x3_dilany_wrw(x, torch.randn(1, 64, 6, 8), 12)
    # through the module: stride 2, padding != dilation and groups 2 stay on the reference's convolution
    calls = []
    orig = K.Conv3x3DilAny.apply
    monkeypatch.setattr(K.Conv3x3DilAny, "apply", staticmethod(lambda *a: (calls.append("Conv3x3DilAny"), orig(*a))[1]))
    xin = torch.randn(1, 64, 26, 28)
    for kw in (dict(stride=2, padding=12, dilation=12), dict(padding=1, dilation=12), dict(padding=12, dilation=12, groups=2),
               dict(padding=(12, 6), dilation=(12, 6))):
        conv = SplitConv2d(64, 64, 3, bias=False, **kw)
        out = conv(xin)
        assert torch.equal(out, F.conv2d(xin, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups))
    assert calls == []


def test_routing(monkeypatch):
    K = _setup(monkeypatch)
    from contrastiveseg_amd.lib.models.tools.module_helper import SplitConv2d
    monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 1)
    calls = []
    for cls in (K.Conv3x3DilAny, K.Conv3x3DilSplit):
        orig = cls.apply
        monkeypatch.setattr(cls, "apply", staticmethod(lambda *a, _o=orig, _n=cls.__name__: (calls.append(_n), _o(*a))[1]))
    orig_wrw = K.conv3x3_dilany_wrw
    monkeypatch.setattr(K, "conv3x3_dilany_wrw", lambda *a, **k: (calls.append("conv3x3_dilany_wrw"), orig_wrw(*a, **k))[1])
    torch.manual_seed(3)
    aspp = SplitConv2d(64, 64, 3, padding=12, dilation=12, bias=False)
    layer3 = SplitConv2d(64, 64, 3, padding=2, dilation=2, bias=False)
    x = torch.randn(1, 64, 6, 20)
    dy = torch.randn(1, 64, 6, 20)

    def run(conv):
        del calls[:]
        conv.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = conv(xi)
        y.backward(dy)
        return list(calls), y.detach(), xi.grad, conv.weight.grad.clone()

    monkeypatch.setattr(K, "CONV3X3_DIL_ANY", False)
    off12, off2 = run(aspp), run(layer3)
    assert off12[0] == [] and off2[0] == ["Conv3x3DilSplit"]
    monkeypatch.setattr(K, "CONV3X3_DIL_ANY", True)
    on12, on2 = run(aspp), run(layer3)
    assert on12[0] == ["Conv3x3DilAny", "conv3x3_dilany_wrw"]
    assert on2[0] == ["Conv3x3DilSplit", "conv3x3_dilany_wrw"]
    for off, on in ((off12, on12), (off2, on2)):
        for a, o, rel in zip(off[1:], on[1:], (3e-5, 3e-5, 1e-4)):
            assert float((a - o).abs().max()) <= rel * float(a.abs().max())
    assert torch.equal(off2[1], on2[1]) and torch.equal(off2[2], on2[2])        # rate 2: forward / backward-data are the same kernels
