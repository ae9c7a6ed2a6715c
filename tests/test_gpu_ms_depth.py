"""The depth-aware multi-scale fusion of the test phase (ms_test_depth): kernels.lut_u16_u8, kernels.ms_fuse_argmax(pixel_weights=...)
(csrc/ms_eval.hip, csrc/cseg_ms_fuse.h: cseg_lut_u16_u8, cseg_ms_fuse_argmax_weighted) and Tester.ms_test_depth.

Yardsticks, those of tests/test_gpu_ms_eval.py: the reference's composition (segmentor/tester.py:426-475: per scale
probs = U(a) + flip(U(b)), full += weight_map * probs with one fp32 weight MAP per scale) restated below with torch ops in float64 and in
fp32 on the same device. R = the largest deviation of torch's fp32 composition from the float64 one on a case; the kernel's largest
deviation must be at most 2 R + 2^-20 sum_i max_p w_i(p) max|logit|. The prediction equals the float64 argmax wherever the float64
top-two margin exceeds 4 R, is one of the float64 top two elsewhere, and at most 1 % of a case's pixels may be in the second group
(a condition on the case, checked with torch on the CPU as well before the shape of the 8-term case was fixed: 0 % there). Weight
maps come from the tables of segmentor/tester.py::depth_fusion_tables, which tests/test_tester_depth_host.py pins against the
reference's float64 statements over all 65 536 disparities. Exact tests compare the weighted call bit for bit with the call that
existed before it. Replayed on the CPU emulation by tests/test_emu_ms_depth.py (the kernel-level tests; not the memory assertion, not
the Tester legs)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ms_eval import _Memo, _check_fused, _check_pred, _tiny_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


_S4 = [(8, 16), (12, 24), (16, 32), (20, 40), (24, 48), (28, 56), (32, 64)]       # scale_search 0.5 ... 2.0 of 64 x 128 at stride 4
_S8 = [(3, 5), (5, 8), (6, 10), (8, 13), (9, 15), (11, 18), (12, 20), (14, 23)]
# name: (B, K, H, W), term sizes, paired
CASES = {
    "odd5": ((2, 19, 37, 53), [(5, 7), (9, 13), (19, 27), (37, 53), (48, 70)], True),
    "city7": ((1, 19, 64, 128), _S4, True),                  # eight bins
    "wide300": ((1, 3, 17, 300), [(5, 75), (9, 150)], False),
    "k171": ((1, 171, 33, 41), [(9, 11), (17, 21)], True),
    "row1": ((1, 2, 1, 9), [(1, 1)], True),
    "bins10": ((1, 19, 24, 40), _S8, True),                  # eight terms: ten bins
}


def _disparity(B, H, W, seed=304):
    """uniform uint16; the upper half of the rows modulo 12 000, so that the far bins (disparity <= 9142) occur as well; one pixel
    with disparity 0 (infinitely far) per image."""
    rs = np.random.RandomState(seed)
    disp = rs.randint(0, 65536, size=(B, H, W)).astype(np.uint16)
    disp[:, :(H + 1) // 2] %= 12000
    disp[:, 0, 0] = 0
    return disp


def _inputs(name, dev):
    from contrastiveseg_amd.segmentor.tester import depth_fusion_tables
    (B, K_, H, W), sizes, paired = CASES[name]
    g = torch.Generator().manual_seed(304)
    terms = []
    for h, w in sizes:
        a = torch.randn(B, K_, h, w, generator=g) * 4
        b = (torch.flip(a, dims=[3]) + 0.5 * torch.randn(B, K_, h, w, generator=g)) if paired else None
        terms.append((a.to(dev), None if b is None else b.to(dev), 1.0))
    lut, table = depth_fusion_tables([0.5 + 0.25 * i for i in range(len(sizes))])
    return terms, H, W, _disparity(B, H, W), lut, table


def _weight_maps(disp, lut, table, dev):
    """The reference's weight maps (:467-473) as fp32 tensors [B,1,H,W], one per scale."""
    bins = lut[disp].astype(np.int64)
    return [torch.from_numpy(np.ascontiguousarray(table[i][bins]))[:, None].to(dev) for i in range(table.shape[0])]


def _compose(terms, H, W, wmaps, dtype):
    """segmentor/tester.py:434-441 and :467-473 on coarse maps that are given: probs = U(a) + flip(U(b)) per scale, then
    full += weight_map * probs in scale order."""
    B, K_ = terms[0][0].shape[:2]
    full = torch.zeros(B, K_, H, W, dtype=dtype, device=terms[0][0].device)
    for (a, b, _), wm in zip(terms, wmaps):
        probs = F.interpolate(a.to(dtype), size=(H, W), mode="bilinear", align_corners=True)
        if b is not None:
            flip_probs = F.interpolate(b.to(dtype), size=(H, W), mode="bilinear", align_corners=True)
            probs = probs + torch.flip(flip_probs, dims=[3])
        full += wm.to(dtype) * probs
    return full


def _yardsticks(terms, H, W, wmaps):
    d64 = _compose(terms, H, W, wmaps, torch.float64)
    d32 = _compose(terms, H, W, wmaps, torch.float32)
    R = float((d32.double() - d64).abs().max())
    amax = max(float(t.abs().max()) for a, b, _ in terms for t in (a, b) if t is not None)
    wsum = sum(float(wm.max()) for wm in wmaps)
    return d64, R, amax, wsum


@functools.lru_cache(maxsize=None)
def _case(name, dev_str):
    """Inputs and the yardsticks of one case, computed once and shared (never modified)."""
    dev = torch.device(dev_str)
    terms, H, W, disp, lut, table = _inputs(name, dev)
    d64, R, amax, wsum = _yardsticks(terms, H, W, _weight_maps(disp, lut, table, dev))
    return terms, H, W, disp, lut, table, d64, R, amax, wsum


def _device_weights(disp, lut, table, dev):
    """The kernel route to the per-pixel weights: one upload, the look-up kernel, the table on the device."""
    from contrastiveseg_amd import kernels as K
    bins = K.lut_u16_u8(torch.from_numpy(disp).to(dev), torch.from_numpy(lut).to(dev))
    return bins, torch.from_numpy(table).to(dev)


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_fused_map_and_prediction_match_the_float64_composition(case):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W, disp, lut, table, d64, R, amax, wsum = _case(case, str(dev))
    if case in ("city7", "bins10"):                        # every bin occurs, the far end through disparity 0
        assert sorted(np.unique(lut[disp])) == list(range(table.shape[1])) and table.shape[1] == (8 if case == "city7" else 10)
    bins, table_d = _device_weights(disp, lut, table, dev)
    assert bins.dtype == torch.uint8 and np.array_equal(bins.cpu().numpy(), lut[disp])
    pred, fused = K.ms_fuse_argmax(terms, H, W, want_fused=True, pixel_weights=(bins, table_d))
    assert fused.shape == d64.shape and fused.dtype == torch.float32
    assert pred.shape == (d64.shape[0], H, W) and pred.dtype == torch.uint8
    _check_fused(case, fused, d64, R, amax, wsum)
    _check_pred(case, pred, d64, R)


# ---- 2. bit for bit against the call without pixel weights --------------------------------------------------------------------------------
_SIZES8 = [(5, 7), (9, 13), (19, 27), (37, 53), (48, 70), (3, 4), (12, 20), (7, 9)]
_C8 = [0.5, 0.75, 1.0, 1.25, 1.5, 0.8, 0.64, 2.0]


def _dense(n, dev, B=2, K_=19, flip_from=0):
    g = torch.Generator().manual_seed(304)
    terms = []
    for i, (h, w) in enumerate(_SIZES8[:n]):
        a = torch.randn(B, K_, h, w, generator=g) * 4
        b = torch.flip(a, dims=[3]) + 0.5 * torch.randn(B, K_, h, w, generator=g)
        terms.append((a.to(dev), b.to(dev) if i >= flip_from else None, 1.0))
    return terms


# one, two, four and eight terms are the kernel's four instances; 3 and 5 leave slots of an instance unused
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_a_table_constant_per_term_equals_scalar_weights(n):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms = _dense(n, dev, flip_from=1 if n == 3 else 0)           # n = 3: a term without a flipped map among terms with one
    H, W = 37, 53
    nbins = 3
    table = torch.tensor(_C8[:n], dtype=torch.float32)[:, None].repeat(1, nbins).contiguous().to(dev)
    # any bins: also bytes >= nbins, which read the last column
    bins = torch.randint(0, 256, (2, H, W), generator=torch.Generator().manual_seed(n), dtype=torch.uint8).to(dev)
    want_pred, want_fused = K.ms_fuse_argmax([(a, b, c) for (a, b, _), c in zip(terms, _C8)], H, W, want_fused=True)
    pred, fused = K.ms_fuse_argmax(terms, H, W, want_fused=True, pixel_weights=(bins, table))
    assert torch.equal(fused, want_fused) and torch.equal(pred, want_pred)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_a_one_bin_table_of_ones_equals_the_unweighted_call(n):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms = _dense(n, dev)
    H, W = 37, 53
    bins = torch.randint(0, 256, (2, H, W), generator=torch.Generator().manual_seed(n), dtype=torch.uint8).to(dev)
    want_pred, want_fused = K.ms_fuse_argmax(terms, H, W, want_fused=True)
    pred, fused = K.ms_fuse_argmax(terms, H, W, want_fused=True, pixel_weights=(bins, torch.ones(n, 1, device=dev)))
    assert torch.equal(fused, want_fused) and torch.equal(pred, want_pred)


def test_one_scale_without_flip_equals_ss_test():
    """What Tester.ss_test hands to the kernel: one term, no mirrored pass, weight 1."""
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    a = (torch.randn(2, 19, 16, 24, generator=torch.Generator().manual_seed(304)) * 4).to(dev)
    want_pred, want_fused = K.ms_fuse_argmax([(a, None, 1.0)], 64, 96, want_fused=True)
    bins = torch.zeros(2, 64, 96, dtype=torch.uint8, device=dev)
    pred, fused = K.ms_fuse_argmax([(a, None, 1.0)], 64, 96, want_fused=True, pixel_weights=(bins, torch.ones(1, 1, device=dev)))
    assert torch.equal(fused, want_fused) and torch.equal(pred, want_pred)
    # and the weights act per pixel: bin 1 of a two-bin table scales exactly those pixels
    bins[:, 32:] = 1
    table = torch.tensor([[1.0, 0.5]], device=dev)
    _, half = K.ms_fuse_argmax([(a, None, 1.0)], 64, 96, want_fused=True, pixel_weights=(bins, table))
    assert torch.equal(half[:, :, :32], want_fused[:, :, :32]) and torch.equal(half[:, :, 32:], want_fused[:, :, 32:] * 0.5)


# ---- 3. tie rule, determinism, either output alone --------------------------------------------------------------------------------------
def test_first_index_wins_among_equal_maxima():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W, disp, lut, table = _inputs("odd5", dev)
    tied = []
    for a, b, w in terms:
        a, b = a.clone(), b.clone()
        a[:, 2] += 100.0
        b[:, 2] += 100.0
        a[:, 5] = a[:, 2]
        b[:, 5] = b[:, 2]
        tied.append((a, b, w))
    pred, fused = K.ms_fuse_argmax(tied, H, W, want_fused=True, pixel_weights=_device_weights(disp, lut, table, dev))
    assert torch.equal(fused[:, 2], fused[:, 5])
    assert bool((pred == 2).all())


def test_two_calls_are_bit_identical():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W, disp, lut, table = _inputs("city7", dev)
    b1, t1 = _device_weights(disp, lut, table, dev)
    b2, _ = _device_weights(disp, lut, table, dev)
    assert torch.equal(b1, b2)
    p1, f1 = K.ms_fuse_argmax(terms, H, W, want_fused=True, pixel_weights=(b1, t1))
    p2, f2 = K.ms_fuse_argmax(terms, H, W, want_fused=True, pixel_weights=(b1, t1))
    assert torch.equal(p1, p2) and torch.equal(f1, f2)


def test_pred_alone_and_fused_alone():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W, disp, lut, table = _inputs("odd5", dev)
    pw = _device_weights(disp, lut, table, dev)
    pred, fused = K.ms_fuse_argmax(terms, H, W, want_fused=True, pixel_weights=pw)
    only_pred = K.ms_fuse_argmax(terms, H, W, pixel_weights=pw)
    none, only_fused = K.ms_fuse_argmax(terms, H, W, want_fused=True, want_pred=False, pixel_weights=pw)
    assert torch.equal(only_pred, pred) and none is None and torch.equal(only_fused, fused)


# ---- 4. the look-up kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 257, 4097])
def test_lut_u16_u8_equals_numpy_indexing(n):
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    rs = np.random.RandomState(304 + n)
    lut = rs.randint(0, 256, size=65536).astype(np.uint8)
    src = rs.randint(0, 65536, size=n).astype(np.uint16)
    src[:2] = [65535, 0][:min(n, 2)]
    got = K.lut_u16_u8(torch.from_numpy(src).to(dev), torch.from_numpy(lut).to(dev))
    assert got.dtype == torch.uint8 and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), lut[src])
    # int16 carrying the same bits; a shape of more than one axis
    if n == 4097:
        src2 = np.ascontiguousarray(src[:4096].reshape(2, 32, 64))
        got2 = K.lut_u16_u8(torch.from_numpy(src2.view(np.int16)).to(dev), torch.from_numpy(lut).to(dev))
        assert got2.shape == (2, 32, 64) and np.array_equal(got2.cpu().numpy(), lut[src2])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def _raw(dev, n_terms=1, K_=4, nbins=2, bins=True, table=True, pred=True, weights=None):
    """cseg_ms_fuse_argmax_weighted itself, past the wrapper, on a prediction buffer filled with 7: a refusal launches nothing."""
    from contrastiveseg_amd import _hip
    m = max(n_terms, 1)
    a = torch.zeros(1, max(K_, 1), 3, 5, device=dev)
    out = torch.full((60,), 7, dtype=torch.uint8, device=dev)
    b = torch.zeros(60, dtype=torch.uint8, device=dev)
    t = torch.ones(m, max(nbins, 1), device=dev)
    wt = None if weights is None else (ctypes.c_float * m)(*weights)
    try:
        _hip.call("cseg_ms_fuse_argmax_weighted", n_terms, (ctypes.c_void_p * m)(*[a.data_ptr()] * m), None, (ctypes.c_int * m)(*[3] * m),
                  (ctypes.c_int * m)(*[5] * m), wt, ctypes.c_void_p(b.data_ptr() if bins else None),
                  ctypes.c_void_p(t.data_ptr() if table else None), nbins, 1, K_, 6, 10,
                  ctypes.c_void_p(out.data_ptr() if pred else None), ctypes.c_void_p(None), _hip.stream_ptr())
    finally:
        if dev.type == "cuda":
            torch.cuda.synchronize()
    return out


def test_refusals():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    a, b = torch.randn(1, 4, 3, 5, device=dev), torch.randn(1, 4, 3, 5, device=dev)
    bins, table = torch.zeros(1, 6, 10, dtype=torch.uint8, device=dev), torch.ones(1, 2, device=dev)
    # the wrapper
    with pytest.raises(RuntimeError, match=r"terms\[0\] has weight 0.5 together with pixel_weights"):
        K.ms_fuse_argmax([(a, b, 0.5)], 6, 10, pixel_weights=(bins, table))
    with pytest.raises(RuntimeError, match="perm together with pixel_weights"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, perm=[0, 1, 3, 2], pixel_weights=(bins, table))
    with pytest.raises(RuntimeError, match=r"pixel_weights bins is \(1, 6, 9\)"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins[:, :, :9].contiguous(), table))
    with pytest.raises(RuntimeError, match=r"pixel_weights table is \(2, 2\)"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins, torch.ones(2, 2, device=dev)))
    with pytest.raises(RuntimeError, match="pixel_weights bins must be torch.uint8"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins.to(torch.int32), table))
    with pytest.raises(RuntimeError, match="pixel_weights table must be torch.float32"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins, table.double()))
    with pytest.raises(RuntimeError, match="src must be torch.uint16"):
        K.lut_u16_u8(torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(65536, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="lut has 256 entries"):
        K.lut_u16_u8(torch.zeros(4, dtype=torch.int16, device=dev), torch.zeros(256, dtype=torch.uint8, device=dev))
    # the library, through the wrapper
    with pytest.raises(RuntimeError, match="nbins = 17"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins, torch.ones(1, 17, device=dev)))
    with pytest.raises(RuntimeError, match="nbins = 0"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins, torch.ones(1, 0, device=dev)))
    with pytest.raises(RuntimeError, match="both outputs"):
        K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, want_pred=False, pixel_weights=(bins, table))
    with pytest.raises(RuntimeError, match="K = 257"):
        K.ms_fuse_argmax([(torch.zeros(1, 257, 2, 2, device=dev), None, 1.0)], 6, 10, pixel_weights=(bins, table))
    assert K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins, torch.ones(1, 16, device=dev))).shape == (1, 6, 10)
    # the library alone: accepted as it stands, then refused with the buffer untouched
    assert bool((_raw(dev) == 0).all())
    assert bool((_raw(dev, weights=[1.0]) == 0).all())
    for kw, what in ((dict(n_terms=0), "n_terms = 0"), (dict(n_terms=9), "n_terms = 9"), (dict(K_=0), "K = 0"), (dict(K_=257), "K = 257"),
                     (dict(nbins=0), "nbins = 0"), (dict(nbins=17), "nbins = 17"), (dict(bins=False), "bins is null"),
                     (dict(table=False), "table is null"), (dict(pred=False), "both outputs"),
                     (dict(weights=[0.5]), r"weights\[0\] = 0.5")):
        with pytest.raises(RuntimeError, match=what):
            _raw(dev, **kw)
    if dev.type == "cuda":          # on the emulated device host tensors ARE the device's tensors
        with pytest.raises(RuntimeError, match="GPU"):
            K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins.cpu(), table))
        with pytest.raises(RuntimeError, match="GPU"):
            K.ms_fuse_argmax([(a, b, 1.0)], 6, 10, pixel_weights=(bins, table.cpu()))
        with pytest.raises(RuntimeError, match="GPU"):
            K.lut_u16_u8(torch.zeros(4, dtype=torch.int16), torch.zeros(65536, dtype=torch.uint8, device=dev))


# ---- 6. memory -----------------------------------------------------------------------------------------------------------------------------
def test_nothing_of_the_size_of_the_fused_map_is_allocated():
    from contrastiveseg_amd import kernels as K
    dev = _dev()
    terms, H, W, disp, lut, table = _inputs("city7", dev)
    B, K_ = terms[0][0].shape[:2]
    src, lut_d, table_d = torch.from_numpy(disp).to(dev), torch.from_numpy(lut).to(dev), torch.from_numpy(table).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    pred = K.ms_fuse_argmax(terms, H, W, pixel_weights=(K.lut_u16_u8(src, lut_d), table_d))
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("peak growth %d bytes; the fused map would be %d" % (growth, B * K_ * H * W * 4))
    assert pred.numel() == B * H * W and growth < B * K_ * H * W * 4


# ---- 7. the Tester --------------------------------------------------------------------------------------------------------------------------
def _restate(net, inputs, scales, wmaps, dtype):
    """ms_test_depth / fuse_with_depth of the reference (:426-475) driven with the same model object; the model runs in fp32,
    everything after it in `dtype`."""
    n, c, h, w = inputs.shape

    def ss_test(x, scale):
        scaled = F.interpolate(x, size=(int(h * scale), int(w * scale)), mode="bilinear", align_corners=True)
        out = net(scaled, is_eval=True)["seg"]
        return F.interpolate(out.to(dtype), size=(h, w), mode="bilinear", align_corners=True), float(out.abs().max())

    full, amax = None, 0.0
    for scale, wm in zip(scales, wmaps):
        probs, m = ss_test(inputs, scale)
        flip_probs, m2 = ss_test(torch.flip(inputs, dims=[3]), scale)
        amax = max(amax, m, m2)
        probs = probs + torch.flip(flip_probs, dims=[3])
        if full is None:
            full = torch.zeros_like(probs)
        full += wm.to(dtype) * probs
    return full, amax


def test_phase_test_end_to_end_with_disparity_pngs(tmp_path, monkeypatch):
    from PIL import Image
    from contrastiveseg_amd import main_contrastive
    from contrastiveseg_amd.lib.metrics.running_score import RunningScore
    from contrastiveseg_amd.segmentor import tester as T
    ids = [3, 7, 9, 11, 20]
    scales = [0.5, 1.0, 1.5]
    rs = np.random.RandomState(304)
    img_dir, lab_dir, depth_dir, out_dir = tmp_path / "val" / "image", tmp_path / "val" / "label", tmp_path / "stereo", tmp_path / "out"
    img_dir.mkdir(parents=True)
    lab_dir.mkdir()
    depth_dir.mkdir()
    stems = ("frankfurt_000000", "munster_000001")
    labels, disps = {}, {}
    for k, stem in enumerate(stems):
        Image.fromarray(rs.randint(0, 256, size=(64, 96, 3)).astype(np.uint8)).save(str(img_dir / (stem + ".png")))
        lab = np.full((64, 96), 255, np.uint8)
        for _ in range(10):
            y0, x0 = rs.randint(0, 64), rs.randint(0, 96)
            lab[y0:y0 + 24, x0:x0 + 32] = ids[rs.randint(0, len(ids))]
        Image.fromarray(lab).save(str(lab_dir / (stem + ".png")))
        labels[stem] = lab
        disps[stem] = _disparity(1, 64, 96, seed=304 + k)[0]
        Image.fromarray(disps[stem]).save(str(depth_dir / (stem + ".png")))
    made = []
    init = T.Tester.__init__

    def remembering(self, *args, **kw):                    # the Tester of main() with its model's outputs remembered per input
        init(self, *args, **kw)
        self.seg_net = _Memo(self.seg_net)
        made.append(self)

    monkeypatch.setattr(T.Tester, "__init__", remembering)
    log = str(tmp_path / "test.log")
    miou = main_contrastive.main(
        ["--configs", os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"), "--phase", "test", "--test_dir", str(img_dir),
         "--out_dir", str(out_dir), "--log_file", log, "--stdout_level", "error", "network.pretrained", "None", "network.resume", "None",
         "data.label_list", str(ids), "test.mode", "ms_test_depth", "test.scale_search", str(scales), "test.batch_size", "2",
         "test.depth_dir", str(depth_dir),
         "test.data_transformer", "{'size_mode': 'fix_size', 'input_size': [96, 64], 'align_method': 'only_pad'}"])
    tester, = made
    assert tester.mode == "ms_test_depth" and tester.depth_table.shape == (3, 4)
    # the written PNGs against the float64 composition on the remembered coarse maps
    lut, table = tester.depth_tables
    inv = np.full(256, -1, np.int64)
    inv[ids] = np.arange(5)
    batches = list(tester.test_loader)
    assert [n for b in batches for n in b["name"]] == list(stems)
    inputs = torch.cat([b["img"] for b in batches])
    wmaps = _weight_maps(np.stack([disps[s] for s in stems]), lut, table, inputs.device)
    n_seen = len(tester.seg_net.seen)
    with torch.no_grad():
        d64, amax = _restate(tester.seg_net, inputs, scales, wmaps, torch.float64)
        d32, _ = _restate(tester.seg_net, inputs, scales, wmaps, torch.float32)
    assert len(tester.seg_net.seen) == n_seen == 2 * len(scales)       # the restatement ran on the coarse maps of the test run
    R = float((d32.double() - d64).abs().max())
    score = RunningScore(num_classes=5, ignore_index=-1)
    pngs = []
    for stem in stems:
        png = np.asarray(Image.open(str(out_dir / "label" / (stem + ".png"))))
        assert png.shape == (64, 96) and png.dtype == np.uint8 and set(np.unique(png)) <= set(ids)
        pngs.append(inv[png])
        score.update(torch.from_numpy(inv[png]), torch.from_numpy(inv[labels[stem]]))
    _check_pred("phase test ms_test_depth", torch.from_numpy(np.stack(pngs)).to(inputs.device), d64, R)
    assert sorted(os.listdir(str(out_dir / "label"))) == [s + ".png" for s in stems]
    want = float(score.get_mean_iou())
    assert int(score.confusion_matrix.sum()) == sum(int((lab != 255).sum()) for lab in labels.values())
    assert miou == want, (miou, want)
    assert "Test mIoU {:.6f}".format(want) in open(log).read()
    # the fused map of the same Tester, same coarse maps
    with torch.no_grad():
        pred, fused = tester.ms_test_depth(inputs, list(stems), want_fused=True)
    _check_fused("tester ms_test_depth", fused, d64, R, amax, sum(float(wm.max()) for wm in wmaps))
    assert np.array_equal(pred.cpu().numpy(), np.stack(pngs))


@pytest.mark.parametrize("value", [0, 1500, 40000])
def test_constant_disparity_is_ms_test_with_that_column_as_scale_weights(value, tmp_path):
    from PIL import Image
    from contrastiveseg_amd.segmentor.tester import Tester
    dev = _dev()
    scales = [0.5, 1.0, 1.5]
    names = ["a", "b"]
    for name in names:
        Image.fromarray(np.full((64, 96), value, np.uint16)).save(str(tmp_path / (name + ".png")))
    torch.manual_seed(304)
    depth = Tester(_tiny_cfg(mode="ms_test_depth", scale_search=scales, depth_dir=str(tmp_path)))
    depth.seg_net = _Memo(depth.seg_net)
    lut, table = depth.depth_tables
    column = [float(v) for v in table[:, lut[value]]]
    assert lut[value] == {0: 3, 1500: 2, 40000: 0}[value]
    plain = Tester(_tiny_cfg(mode="ms_test", scale_search=scales, scale_weights=column), seg_net=depth.seg_net)
    inputs = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(304)).to(dev)
    with torch.no_grad():
        p_depth, f_depth = depth.ms_test_depth(inputs, names, want_fused=True)
        p_plain, f_plain = plain.ms_test(inputs, want_fused=True)
    assert torch.equal(f_depth, f_plain) and torch.equal(p_depth, p_plain)
