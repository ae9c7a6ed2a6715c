"""The sliding-crop test modes: csrc/crop_eval.hip (kernels.crop_fuse_argmax) and Tester.sscrop_test / mscrop_test.

Yardsticks, as in tests/test_gpu_ms_eval.py: the reference's composition (segmentor/tester.py:351-378 sscrop_test -- a logits canvas
and a count canvas filled tile by tile, divided, resized -- and :505-523 mscrop_test) restated below with torch ops in float64, and
the same composition in fp32 with torch ops on the same device. R = the largest deviation of torch's own fp32 composition from the
float64 one on a case. The kernel's largest deviation must be at most 2 R + 2^-19 n_maps max|logit|, n_maps = the number of coarse
passes, plain plus flipped: per pass at most 12 roundings of at most 2^-24 max|logit| (4 for the coarse blend, 3 for the tile sum, 0
for the exact division by 1, 2 or 4, 4 for the canvas blend, 1 for the flip add) and n_maps more from the accumulation, which for
n_maps <= 16 is under 2^-19 per pass. The prediction equals the float64 argmax wherever the float64 top-two margin exceeds twice that
bound, is one of the float64 top two elsewhere, and at most 1 % of a case's pixels may be in the second group. The kernel is never
compared with itself, except for determinism and for the mirrored tiling (one expression on mirrored columns). Replayed on the CPU
emulation by tests/test_emu_crop_eval.py (the kernel-level tests; not the Tester legs)."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _decide_intersection(total_length, crop_length):
    """segmentor/tester.py:525-533 of the reference, literally."""
    stride = crop_length
    times = (total_length - crop_length) // stride + 1
    cropped_starting = []
    for i in range(times):
        cropped_starting.append(stride * i)
    if total_length - cropped_starting[-1] > crop_length:
        cropped_starting.append(total_length - crop_length)
    return cropped_starting


def _sscrop(stack, canvas, crop, H, W, dtype):
    """:358-378 on coarse crop outputs that are given: stack [tiles,B,K,hc,wc] in the reference's tile order."""
    (hs, ws), (ch, cw) = canvas, crop
    B, K = stack.shape[1:3]
    full = torch.zeros(B, K, hs, ws, dtype=dtype, device=stack.device)
    count = torch.zeros(B, K, hs, ws, dtype=dtype, device=stack.device)
    t = 0
    for y0 in _decide_intersection(hs, ch):
        for x0 in _decide_intersection(ws, cw):
            prediction = F.interpolate(stack[t].to(dtype), size=(ch, cw), mode="bilinear", align_corners=True)
            count[:, :, y0:y0 + ch, x0:x0 + cw] += 1
            full[:, :, y0:y0 + ch, x0:x0 + cw] += prediction
            t += 1
    assert t == stack.shape[0]
    full /= count
    return F.interpolate(full, size=(H, W), mode="bilinear", align_corners=True)


def _compose(terms, H, W, dtype):
    """:505-523: per scale probs = P(x) + flip(P(flip(x))), full_probs += probs; P = ss_test (:310-327) for a plain term and sscrop_test
    for a tiled one. terms as kernels.crop_fuse_argmax takes them."""
    first = terms[0][0] if terms[0][0] is not None else terms[0][1]
    B, K = first.shape[-4:-2]
    full = torch.zeros(B, K, H, W, dtype=dtype, device=first.device)

    def one(t, term):
        if len(term) == 2:
            return F.interpolate(t.to(dtype), size=(H, W), mode="bilinear", align_corners=True)
        return _sscrop(t, term[2], term[3], H, W, dtype)

    for term in terms:
        a, b = term[0], term[1]
        probs = one(a, term) if a is not None else None
        if b is not None:
            flipped = torch.flip(one(b, term), dims=[3])
            probs = flipped if probs is None else probs + flipped
        full += probs
    return full


_MS7 = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
# name: (B, K, H, W), crop, coarse map of one crop, scales, flipped stacks present
CASES = {
    "single": ((1, 3, 16, 24), (16, 24), (4, 6), [1.0], False),
    "exact2x2": ((2, 19, 32, 48), (16, 24), (4, 6), [1.0], True),
    "ragged": ((2, 19, 37, 53), (16, 24), (4, 6), [1.0], True),
    "plus1": ((1, 5, 17, 25), (16, 24), (4, 6), [1.0], True),
    "fullw": ((1, 2, 40, 9), (16, 9), (4, 3), [1.0], True),
    "ms7": ((2, 19, 37, 53), (24, 32), (6, 8), _MS7, True),
    "k171": ((1, 171, 33, 41), (20, 20), (3, 3), [1.0, 1.5], True),
}


def _inputs(name, dev):
    """Logits 4 * randn, seed 304. The maps of the mirrored input are the mirrored maps of the plain input (tile (ty, tx) of the mirrored
    canvas shows what tile (ty, nx-1-tx) of the plain one shows) plus noise, as a network would give them."""
    (B, K, H, W), (ch, cw), (hc, wc), scales, paired = CASES[name]
    g = torch.Generator().manual_seed(304)
    terms = []
    for s in scales:
        hs, ws = int(H * s), int(W * s)
        if s < 1:
            a = torch.randn(B, K, math.ceil(hs / 4), math.ceil(ws / 4), generator=g) * 4
            b = torch.flip(a, dims=[3]) + 0.5 * torch.randn(a.shape, generator=g) if paired else None
            terms.append((a.to(dev), None if b is None else b.to(dev)))
            continue
        ny, nx = len(_decide_intersection(hs, ch)), len(_decide_intersection(ws, cw))
        a = torch.randn(ny * nx, B, K, hc, wc, generator=g) * 4
        b = None
        if paired:
            b = torch.flip(a.view(ny, nx, B, K, hc, wc), dims=[1, 5]).reshape(a.shape) + 0.5 * torch.randn(a.shape, generator=g)
        terms.append((a.to(dev), None if b is None else b.to(dev), (hs, ws), (ch, cw)))
    return terms, H, W


def _n_maps(terms):
    return sum(1 for term in terms for t in term[:2] if t is not None)


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Inputs and the two yardsticks of one case, computed once and shared (never modified)."""
    terms, H, W = _inputs(name, torch.device(dev_str))
    d64 = _compose(terms, H, W, torch.float64)
    d32 = _compose(terms, H, W, torch.float32)
    R = float((d32.double() - d64).abs().max())
    amax = max(float(t.abs().max()) for term in terms for t in term[:2] if t is not None)
    return terms, H, W, d64, R, amax, _n_maps(terms)


def _bound(R, amax, n_maps):
    return 2 * R + 2.0 ** -19 * n_maps * amax


def _check_fused(tag, fused, d64, R, amax, n_maps):
    err = float((fused.double() - d64).abs().max())
    bound = _bound(R, amax, n_maps)
    print("%s: R (torch fp32 vs float64) %.3e  kernel vs float64 %.3e  bound %.3e  max|logit| %.2f  maps %d" % (tag, R, err, bound, amax, n_maps))
    assert err <= bound, (tag, err, bound, R)


def _check_pred(tag, pred, d64, R, amax, n_maps):
    top = d64.topk(2, dim=1)
    margin = top.values[:, 0] - top.values[:, 1]
    clear = margin > 2 * _bound(R, amax, n_maps)
    pred = pred.long()
    first, second = top.indices[:, 0], top.indices[:, 1]
    share = 1.0 - float(clear.double().mean())
    print("%s: %.4f %% of the pixels within twice the bound of a tie" % (tag, 100 * share))
    assert bool((pred[clear] == first[clear]).all()), tag
    assert bool(((pred == first) | (pred == second))[~clear].all()), tag
    assert share <= 0.01, (tag, share)


@pytest.mark.parametrize("case", list(CASES))
def test_fused_map_matches_the_float64_composition(case):
    from contrastiveseg_amd import kernels as K
    terms, H, W, d64, R, amax, n_maps = _case(case, str(_dev()))
    pred, fused = K.crop_fuse_argmax(terms, H, W, want_fused=True)
    assert fused.shape == d64.shape and fused.dtype == torch.float32
    _check_fused(case, fused, d64, R, amax, n_maps)
    only_fused = K.crop_fuse_argmax(terms, H, W, want_fused=True, want_pred=False)
    assert only_fused[0] is None and torch.equal(only_fused[1], fused)
    if case == "single":            # one tile that is the whole image: ss_test, bit for bit
        p_ms, f_ms = K.ms_fuse_argmax([(terms[0][0][0], None, 1.0)], H, W, want_fused=True)
        assert torch.equal(f_ms, fused) and torch.equal(p_ms, pred)
        p_pl, f_pl = K.crop_fuse_argmax([(terms[0][0][0], None)], H, W, want_fused=True)
        assert torch.equal(f_pl, fused) and torch.equal(p_pl, pred)


@pytest.mark.parametrize("case", list(CASES))
def test_prediction_matches_the_float64_argmax(case):
    from contrastiveseg_amd import kernels as K
    terms, H, W, d64, R, amax, n_maps = _case(case, str(_dev()))
    pred = K.crop_fuse_argmax(terms, H, W)
    assert pred.shape == (d64.shape[0], H, W) and pred.dtype == torch.uint8
    _check_pred(case, pred, d64, R, amax, n_maps)


def test_the_flipped_pass_tiles_the_mirrored_canvas():
    """On `ragged` (starts 0,24,29 across: the overlap band of the mirrored canvas lies on the other side of the image): the fused map
    from the flipped stacks alone is the horizontal flip of the fused map with those stacks passed as the plain ones, bit for bit."""
    from contrastiveseg_amd import kernels as K
    terms, H, W = _inputs("ragged", _dev())
    (a, b, canvas, crop), = terms
    assert not torch.equal(b, a)
    _, as_flipped = K.crop_fuse_argmax([(None, b, canvas, crop)], H, W, want_fused=True)
    _, as_plain = K.crop_fuse_argmax([(b, None, canvas, crop)], H, W, want_fused=True)
    assert torch.equal(as_flipped, torch.flip(as_plain, dims=[3]))
    assert not torch.equal(as_flipped, as_plain)
    # and against the restatement, which flips a finished map
    d64 = torch.flip(_sscrop(b, canvas, crop, H, W, torch.float64), dims=[3])
    d32 = torch.flip(_sscrop(b, canvas, crop, H, W, torch.float32), dims=[3])
    _check_fused("ragged, flipped alone", as_flipped, d64, float((d32.double() - d64).abs().max()), float(b.abs().max()), 1)


def test_first_index_wins_among_equal_maxima():
    from contrastiveseg_amd import kernels as K
    terms, H, W = _inputs("ms7", _dev())
    tied = []
    for term in terms:
        a, b = term[0].clone(), term[1].clone()
        for t in (a, b):
            t[..., 2, :, :] += 100.0
            t[..., 5, :, :] = t[..., 2, :, :]
        tied.append((a, b) + tuple(term[2:]))
    pred, fused = K.crop_fuse_argmax(tied, H, W, want_fused=True)
    assert torch.equal(fused[:, 2], fused[:, 5])
    assert bool((pred == 2).all())


def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    terms, H, W = _inputs("ms7", _dev())
    p1, f1 = K.crop_fuse_argmax(terms, H, W, want_fused=True)
    p2, f2 = K.crop_fuse_argmax(terms, H, W, want_fused=True)
    assert torch.equal(p1, p2) and torch.equal(f1, f2)


def test_refusals():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    a = torch.randn(1, 4, 3, 5, device=dev)
    st = torch.randn(4, 1, 4, 2, 3, device=dev)                  # 2 x 2 tiles of a 12 x 20 canvas under an 8 x 12 crop
    ok = (st, None, (12, 20), (8, 12))
    assert K.crop_fuse_argmax([ok], 6, 10).shape == (1, 6, 10)
    with pytest.raises(RuntimeError, match="9 terms"):
        K.crop_fuse_argmax([(a, None)] * 9, 6, 10)
    with pytest.raises(RuntimeError, match="0 terms"):
        K.crop_fuse_argmax([], 6, 10)
    with pytest.raises(RuntimeError, match="257 classes"):
        K.crop_fuse_argmax([(torch.zeros(1, 257, 2, 2, device=dev), None)], 4, 4)
    with pytest.raises(RuntimeError, match="canvas 7 x 20 is smaller than the crop 8 x 12"):
        K.crop_fuse_argmax([(st, None, (7, 20), (8, 12))], 6, 10)
    with pytest.raises(RuntimeError, match="canvas 12 x 11 is smaller than the crop 8 x 12"):
        K.crop_fuse_argmax([(st, None, (12, 11), (8, 12))], 6, 10)
    with pytest.raises(RuntimeError, match="stack of 4 tiles for the 2 x 3 tiles"):
        K.crop_fuse_argmax([(st, None, (12, 25), (8, 12))], 6, 10)
    with pytest.raises(RuntimeError, match="flipped stack"):
        K.crop_fuse_argmax([(st, torch.randn(4, 1, 4, 2, 4, device=dev), (12, 20), (8, 12))], 6, 10)
    with pytest.raises(RuntimeError, match="flipped map"):
        K.crop_fuse_argmax([(a, torch.randn(1, 4, 3, 6, device=dev))], 6, 10)
    with pytest.raises(RuntimeError, match="neither"):
        K.crop_fuse_argmax([(None, None)], 6, 10)
    with pytest.raises(RuntimeError, match="both outputs"):
        K.crop_fuse_argmax([ok], 6, 10, want_fused=False, want_pred=False)
    with pytest.raises(RuntimeError, match="empty"):
        K.crop_fuse_argmax([ok], 0, 10)
    with pytest.raises(RuntimeError, match="empty"):
        K.crop_fuse_argmax([(torch.zeros(4, 1, 4, 0, 3, device=dev), None, (12, 20), (8, 12))], 6, 10)
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            K.crop_fuse_argmax([(st.cpu(), None, (12, 20), (8, 12))], 6, 10)


def test_the_library_refuses_what_the_wrapper_refuses():
    """The C entry point's own checks (another caller of the C-ABI has no wrapper in front of it)."""
    import ctypes
    from contrastiveseg_amd import _hip
    dev = _dev()
    st = torch.randn(4, 1, 4, 2, 3, device=dev)
    pred = torch.zeros(1, 6, 10, dtype=torch.uint8, device=dev)

    def call(dims, n=1, out=True, K_=4):
        pa = (ctypes.c_void_p * 8)(*([st.data_ptr()] * 8))
        d = (ctypes.c_int * (7 * 8))(*(list(dims) * 8))
        _hip.call("cseg_crop_fuse_argmax", n, pa, None, d, 1, K_, 6, 10, ctypes.c_void_p(pred.data_ptr() if out else None),
                  ctypes.c_void_p(None), _hip.stream_ptr())

    call([12, 20, 8, 12, 2, 3, 4])
    for dims, kw, msg in [([12, 20, 8, 12, 2, 3, 4], dict(n=9), "9 terms"), ([12, 20, 8, 12, 2, 3, 4], dict(n=0), "0 terms"),
                          ([12, 20, 8, 12, 2, 3, 4], dict(K_=257), "257 classes"), ([12, 20, 8, 12, 2, 3, 4], dict(out=False), "both outputs"),
                          ([7, 20, 8, 12, 2, 3, 4], {}, "smaller than the crop"), ([12, 20, 8, 12, 2, 3, 6], {}, "stack of 6 tiles"),
                          ([12, 20, 8, 12, 0, 3, 4], {}, "empty")]:
        with pytest.raises(RuntimeError, match=msg):
            call(dims, **kw)


def test_nothing_of_the_size_of_a_canvas_is_allocated():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W = _inputs("ms7", dev)
    B, K_ = CASES["ms7"][0][:2]
    if dev.type != "cuda":
        assert K.crop_fuse_argmax(terms, H, W).numel() == B * H * W
        return
    canvas = B * K_ * 74 * 106 * 4            # one scale-2 canvas
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    pred = K.crop_fuse_argmax(terms, H, W)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("peak growth %d bytes; one scale-2 canvas would be %d" % (growth, canvas))
    assert pred.numel() == B * H * W and growth < canvas


# ---- Tester orchestration, end to end ----------------------------------------------------------------------------------------------------
def _tiny_cfg(**test_keys):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    for k, v in test_keys.items():
        cfg.add(["test", k], v)
    return cfg


def _restate_mscrop(net, inputs, crop_size, scales, dtype):
    """Tester.mscrop_test of the reference (:505-523, with ss_test :310-327 and sscrop_test :351-378) driven with the same model
    object; the model runs in fp32, everything after it in `dtype`. -> (full_probs, max|logit|, number of coarse passes)."""
    n, c, h, w = inputs.shape
    seen = {"amax": 0.0}

    def ss_test(x, scale=1):
        hh, ww = x.shape[-2:]
        scaled = F.interpolate(x, size=(int(hh * scale), int(ww * scale)), mode="bilinear", align_corners=True)
        out = net(scaled, is_eval=True)["seg"]
        seen["amax"] = max(seen["amax"], float(out.abs().max()))
        return F.interpolate(out.to(dtype), size=(hh, ww), mode="bilinear", align_corners=True)

    def sscrop_test(x, scale):
        scaled = F.interpolate(x, size=(int(h * scale), int(w * scale)), mode="bilinear", align_corners=True)
        hs, ws = scaled.shape[-2:]
        full = count = None
        for y0 in _decide_intersection(hs, crop_size[0]):
            for x0 in _decide_intersection(ws, crop_size[1]):
                crop_inputs = scaled[:, :, y0:y0 + crop_size[0], x0:x0 + crop_size[1]].contiguous()
                prediction = ss_test(crop_inputs)
                if full is None:
                    full = torch.zeros(n, prediction.shape[1], hs, ws, dtype=dtype, device=x.device)
                    count = torch.zeros_like(full)
                count[:, :, y0:y0 + crop_size[0], x0:x0 + crop_size[1]] += 1
                full[:, :, y0:y0 + crop_size[0], x0:x0 + crop_size[1]] += prediction
        full /= count
        return F.interpolate(full, size=(h, w), mode="bilinear", align_corners=True)

    full_probs = None
    for scale in scales:
        one = (lambda x: ss_test(x, scale)) if scale < 1 else (lambda x: sscrop_test(x, scale))
        probs = one(inputs)
        probs = probs + torch.flip(one(torch.flip(inputs, dims=[3])), dims=[3])
        if full_probs is None:
            full_probs = torch.zeros_like(probs)
        full_probs += probs
    return full_probs, seen["amax"], 2 * len(scales)


class _Memo(torch.nn.Module):
    """The model with its evaluation outputs remembered per input, as in tests/test_gpu_ms_eval.py: two forward passes of this network
    on the same input differ in the last bits on the GPU, which says nothing about the Tester; where a test compares two routes, or
    counts pixels that may change class, both routes get the same coarse maps."""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x, **kw):
        for x0, out in self.seen:
            if x0.shape == x.shape and torch.equal(x0, x):
                return out
        out = self.net(x, **kw)
        self.seen.append((x.clone(), out))
        return out


def test_tester_mscrop_test_matches_the_restatement():
    """Inputs 2 x 3 x 64 x 96, crop 40 x 56, scales 0.75 (plain), 1.0 (2 x 2 tiles, starts 0,24 x 0,40) and 1.5 (3 x 3 tiles, starts
    0,40,56 x 0,56,88); test.scale_weights is set and must play no part."""
    from contrastiveseg_amd.segmentor.tester import Tester
    dev = _dev()
    scales, crop = [0.75, 1.0, 1.5], [40, 56]
    torch.manual_seed(304)
    tester = Tester(_tiny_cfg(mode="mscrop_test", scale_search=scales, crop_size=crop, scale_weights=[0.5, 1, 2]))
    tester.seg_net = _Memo(tester.seg_net)
    inputs = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(304)).to(dev)
    with torch.no_grad():
        pred, fused = tester.mscrop_test(inputs, crop, want_fused=True)
        calls = len(tester.seg_net.seen)
        d64, amax, n_maps = _restate_mscrop(tester.seg_net, inputs, crop, scales, torch.float64)
        assert len(tester.seg_net.seen) == calls == 2 * (1 + 4 + 9)      # the restatement ran the net on the very same inputs
        d32, _, _ = _restate_mscrop(tester.seg_net, inputs, crop, scales, torch.float32)
    R = float((d32.double() - d64).abs().max())
    _check_fused("tester mscrop_test", fused, d64, R, amax, n_maps)
    _check_pred("tester mscrop_test", pred, d64, R, amax, n_maps)
    assert torch.equal(tester.mscrop_test(inputs, crop), pred)


def test_tester_sscrop_test_with_one_crop_is_ss_test():
    from contrastiveseg_amd.segmentor.tester import Tester
    dev = _dev()
    torch.manual_seed(304)
    tester = Tester(_tiny_cfg(mode="sscrop_test", crop_size=[64, 96]))
    tester.seg_net = _Memo(tester.seg_net)
    inputs = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(304)).to(dev)
    with torch.no_grad():
        p_crop, f_crop = tester.sscrop_test(inputs, [64, 96], want_fused=True)
        p_ss, f_ss = tester.ss_test(inputs, want_fused=True)
    assert len(tester.seg_net.seen) == 1
    assert torch.equal(p_crop, p_ss) and torch.equal(f_crop, f_ss)
    with pytest.raises(ValueError, match="scale 1.*64 x 96.*65 x 96"):
        tester.sscrop_test(inputs, [65, 96])


def test_phase_test_end_to_end_with_mscrop_test(tmp_path):
    from PIL import Image
    from contrastiveseg_amd import main_contrastive
    from contrastiveseg_amd.lib.metrics.running_score import RunningScore
    ids = [3, 7, 9, 11, 20]
    rs = np.random.RandomState(304)
    img_dir, lab_dir, out_dir = tmp_path / "val" / "image", tmp_path / "val" / "label", tmp_path / "out"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir()
    labels = {}
    for stem in ("frankfurt_000000", "munster_000001"):
        Image.fromarray(rs.randint(0, 256, size=(64, 96, 3)).astype(np.uint8)).save(str(img_dir / (stem + ".png")))
        lab = np.full((64, 96), 255, np.uint8)
        for _ in range(10):
            y0, x0 = rs.randint(0, 64), rs.randint(0, 96)
            lab[y0:y0 + 24, x0:x0 + 32] = ids[rs.randint(0, len(ids))]
        Image.fromarray(lab).save(str(lab_dir / (stem + ".png")))
        labels[stem] = lab
    log = str(tmp_path / "test.log")
    miou = main_contrastive.main(
        ["--configs", os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"), "--phase", "test", "--test_dir", str(img_dir),
         "--out_dir", str(out_dir), "--log_file", log, "--stdout_level", "error", "network.pretrained", "None", "network.resume", "None",
         "data.label_list", str(ids), "test.mode", "mscrop_test", "test.crop_size", "[40, 56]", "test.scale_search", "[0.75, 1.0]",
         "test.batch_size", "2", "test.data_transformer", "{'size_mode': 'fix_size', 'input_size': [96, 64], 'align_method': 'only_pad'}"])
    score = RunningScore(num_classes=5, ignore_index=-1)
    lut = np.full(256, -1, np.int64)
    lut[ids] = np.arange(5)
    for stem, lab in labels.items():
        png = np.asarray(Image.open(str(out_dir / "label" / (stem + ".png"))))
        assert png.shape == (64, 96) and png.dtype == np.uint8 and set(np.unique(png)) <= set(ids)
        score.update(torch.from_numpy(lut[png]), torch.from_numpy(lut[lab]))
    assert sorted(os.listdir(str(out_dir / "label"))) == ["frankfurt_000000.png", "munster_000001.png"]
    want = float(score.get_mean_iou())
    assert int(score.confusion_matrix.sum()) == sum(int((lab != 255).sum()) for lab in labels.values())
    assert miou == want, (miou, want)
    assert "Test mIoU {:.6f}".format(want) in open(log).read()
