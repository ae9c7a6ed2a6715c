"""SegFix refinement (kernels.segfix_shift, csrc/segfix.hip): the numpy fp32 restatement of the rule, the table of golden cases that
tools/make_segfix_golden.py turns into tests/golden/segfix/*.npz, and helpers shared by tests/test_segfix_host.py,
tests/test_gpu_segfix.py and tests/test_emu_segfix.py. Not a test module.

The rule (scripts/cityscapes/segfix.py:64-79 through torch's CPU grid_sample, bilinear, border padding, align_corners=False), in the
one fp32 order that has grid_sample's bits:

    sx = fp32(ow * scale) + j                    sy likewise with oh, i
    gx = sx / fp32((w - 1) / 2) - 1
    ix = fma(gx + 1, fp32(w / 2), -0.5);         ix = min(max(ix, 0), w - 1)
    x0 = floor(ix); wx = ix - x0; ex = 1 - wx;   y0, ny, s_y likewise (s_y = 1 - ny)
    nw = s_y * ex; ne = s_y * wx; sw = ny * ex; se = ny * wx
    v  = fma(d, se, fma(c, sw, fma(b, ne, a * nw)))
    out = u8(round_half_even(v))
"""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "segfix")
LABEL_LIST = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
NEAR_TIE = 1e-3              # |v - (n + 0.5)| below this in float64: the fp32 order of operations may decide the label
NEAR_TIE_SHARE = 0.03        # cap on the share of such pixels per golden case: a condition on the fixtures
f32, f64 = np.float32, np.float64

# name: (h, w), seed, kind, scales. kind 'unit': offsets in {-2, 0, 2} / scale, about half of them zero; 'border': additionally +-50 on
# every border row and column (clamping on all four sides); 'real': non-integer fp32 offsets. The seeds are those under which the
# near-tie share of the case stays within NEAR_TIE_SHARE (tools/make_segfix_golden.py asserts it).
GOLDEN_CASES = {
    "a": ((5, 7), 15, "unit", (2.0,)),
    "b": ((19, 31), 1, "unit", (2.0,)),
    "c": ((37, 53), 7, "unit", (2.0,)),
    "d": ((2, 33), 10, "unit", (2.0,)),
    "e": ((33, 2), 1, "unit", (2.0,)),
    "f": ((64, 128), 2, "unit", (2.0,)),
    "g": ((19, 31), 1, "border", (2.0,)),
    "h": ((19, 31), 8, "real", (0.5, 1.0, 2.0)),
}


def golden_names():
    """One fixture per case and scale: 'a' .. 'g', 'h_s0.5', 'h_s1', 'h_s2'."""
    out = []
    for name, (_, _, _, scales) in GOLDEN_CASES.items():
        out += [name if len(scales) == 1 else "%s_s%g" % (name, s) for s in scales]
    return out


def blocky_map(rs, h, w, classes=19):
    """A map of random blocks of about 1/6 of each side: class boundaries are frequent."""
    bh, bw = max(1, h // 6), max(1, w // 6)
    coarse = rs.randint(0, classes, size=((h + bh - 1) // bh, (w + bw - 1) // bw))
    return np.kron(coarse, np.ones((bh, bw), dtype=np.int64))[:h, :w].astype(np.uint8)


def make_case(name):
    """-> [(fixture name, x u8 [h,w] train ids, offsets fp32 [h,w,2] (row, column), scale)] of one row of GOLDEN_CASES."""
    (h, w), seed, kind, scales = GOLDEN_CASES[name]
    out = []
    for s in scales:
        rs = np.random.RandomState(1000 * seed + sum(map(ord, name)))
        x = blocky_map(rs, h, w)
        if kind == "real":
            off = rs.uniform(-3.0, 3.0, size=(h, w, 2)).astype(f32)
        else:
            off = rs.randint(-1, 2, size=(h, w, 2)).astype(f32) * f32(2.0 / s)
            off[rs.random_sample((h, w)) < 0.5] = 0
            if kind == "border":
                off[0, :, 0], off[-1, :, 0] = -50, 50
                off[:, 0, 1], off[:, -1, 1] = -50, 50
        out.append((name if len(scales) == 1 else "%s_s%g" % (name, s), x, off, float(s)))
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fused multiply-add, correctly rounded. The product of two fp32 values is exact in float64; the sum with c is rounded to
    float64 first, so where that sum is exactly half way between two fp32 values and was itself rounded, the error of the float64
    addition (TwoSum) decides the direction."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p = a.astype(f64) * b.astype(f64)
    c = c.astype(f64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    r = s.astype(f32)
    nb = np.nextafter(r, np.where(s > r, np.inf, -np.inf).astype(f32))
    mid = (err != 0) & (s != r.astype(f64)) & ((r.astype(f64) + nb.astype(f64)) / 2 == s)
    away = np.sign(err) != np.sign(r.astype(f64) - s)
    return np.where(mid & away, nb, r).astype(f32)


def _taps(x, x0, y0):
    h, w = x.shape
    xf = x.astype(f32)

    def tap(yy, xx):
        inside = (yy < h) & (xx < w)
        return np.where(inside, xf[np.minimum(yy, h - 1), np.minimum(xx, w - 1)], f32(0))
    return tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)


def restate_value(x, offsets, scale):
    """x [h,w] integer class indices, offsets [h,w,2] (row, column), scale -> the interpolated fp32 value of every pixel."""
    h, w = x.shape
    if h < 2 or w < 2:
        raise ValueError("the rule divides by (side - 1) / 2: %d x %d" % (h, w))
    off = np.asarray(offsets).astype(f32)
    scale = f32(scale)
    i = np.arange(h, dtype=f32)[:, None]
    j = np.arange(w, dtype=f32)[None, :]
    sx, sy = off[..., 1] * scale + j, off[..., 0] * scale + i
    gx, gy = sx / f32((w - 1) / 2) - f32(1), sy / f32((h - 1) / 2) - f32(1)
    ix = fma32(gx + f32(1), f32(w / 2), f32(-0.5))
    iy = fma32(gy + f32(1), f32(h / 2), f32(-0.5))
    ix = np.minimum(np.maximum(ix, f32(0)), f32(w - 1))
    iy = np.minimum(np.maximum(iy, f32(0)), f32(h - 1))
    x0, y0 = np.floor(ix), np.floor(iy)
    wx, ny = ix - x0, iy - y0
    ex, s_y = f32(1) - wx, f32(1) - ny
    nw, ne, sw, se = s_y * ex, s_y * wx, ny * ex, ny * wx
    a, b, c, d = _taps(x, x0.astype(np.int64), y0.astype(np.int64))
    v = fma32(d, se, fma32(c, sw, fma32(b, ne, a * nw)))
    assert v.dtype == f32
    return v


def restate(x, offsets, scale):
    """-> the refined class indices u8 [h,w]."""
    return np.round(restate_value(x, offsets, scale)).astype(np.uint8)


def value_f64(x, offsets, scale):
    """The same quantity evaluated in float64 throughout (the exact-arithmetic yardstick; ties are decided by fp32 roundings, so the
    labels may differ from the rule's on near-tie pixels only)."""
    h, w = x.shape
    off = np.asarray(offsets).astype(f64)
    i = np.arange(h, dtype=f64)[:, None]
    j = np.arange(w, dtype=f64)[None, :]
    sx, sy = off[..., 1] * f64(scale) + j, off[..., 0] * f64(scale) + i
    ix = np.clip((sx / ((w - 1) / 2) - 1 + 1) * (w / 2) - 0.5, 0, w - 1)
    iy = np.clip((sy / ((h - 1) / 2) - 1 + 1) * (h / 2) - 0.5, 0, h - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    wx, ny = ix - x0, iy - y0
    a, b, c, d = (t.astype(f64) for t in _taps(x, x0.astype(np.int64), y0.astype(np.int64)))
    return a * (1 - ny) * (1 - wx) + b * (1 - ny) * wx + c * ny * (1 - wx) + d * ny * wx


def near_tie(v64):
    """Pixels whose float64 value lies within NEAR_TIE of a half-integer."""
    return np.abs(v64 - np.floor(v64) - 0.5) < NEAR_TIE


def id_lut(label_list=LABEL_LIST):
    """u8 [256]: train id -> dataset id, 255 for a train id outside the list (LabelTransformer.decode's fill value)."""
    lut = np.full(256, 255, np.uint8)
    lut[:len(label_list)] = label_list
    return lut


def restate_batch(pred, offsets, records, scale):
    """pred [B,H,W] u8, offsets [B,H,W,2], records (x0, y0, bw, bh) -> refined [B,H,W]: the rule on every region, pred elsewhere."""
    out = pred.copy()
    for b, (x0, y0, bw, bh) in enumerate(records):
        out[b, y0:y0 + bh, x0:x0 + bw] = restate(pred[b, y0:y0 + bh, x0:x0 + bw], offsets[b, y0:y0 + bh, x0:x0 + bw], scale)
    return out


@functools.lru_cache(maxsize=None)
def golden(name):
    """-> dict(x u8 [h,w], offsets fp32 [h,w,2], scale float, out u8 [h,w] train ids, out_ids u8 [h,w], near_tie_share float) as the
    REFERENCE's shift / LabelTransformer produced it; loaded once, shared, never modified."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["scale"], g["near_tie_share"] = float(g["scale"]), float(g["near_tie_share"])
    for k in ("x", "offsets", "out", "out_ids"):
        g[k].setflags(write=False)
    return g
