"""Edge cases for the bilinear exchange kernels: upsample + concat (csrc/upcat.hip), the fused sum with ReLU and the plain n-ary sum
(csrc/fuse.hip) and their shared adjoint (csrc/cseg_bilinear.h) on each of its five routes -- band kernels with 8, 12, 24 and 40 taps
and the gather kernel. A plain module (like tests/loss_edge_cases.py): seeded cases, references and runners `run_*(K, dev, ...)` that
take the kernels module and a device; tests/test_gpu_exchange_edges.py (MI355X) and tests/test_emu_exchange_edges.py (the emulated
device, ascending and descending wave order) are thin users of it. Every case states the route of each of its coarse maps and asserts
it with the library's own plan query (cseg_bilinear_adjoint_plan, the predicate the launcher asks).

Reference. The tap weight of output index o is l1 = f - trunc(f) with f = fp32(s * o), and the compiler decides per instance whether
the subtraction sees the rounded product (`A_r`: the host build, torch on the CPU) or the exact one through an fma (`A_f`: what hipcc
emits for gfx950 under its default contraction). Both are legal, they differ by up to half an ulp of f, and the exchange kernels leave
the choice to the compiler. So per axis axis_ops() builds BOTH dense float64 operators from the kernel's own
index arithmetic; the expected value is always A_r,y . x . A_r,x^T in float64 and the allowed deviation is pointwise, from the
reference alone:
  rounding  forward 6 u Abar_y|x|Abar_x^T;  adjoint (t_x + t_y + 4) u Abar_y^T|g|Abar_x, t = most fine indices on one coarse index;
            fused sum (n_same + n_low + 6) u (sum|same| + sum Abar|low|Abar^T)                   (u = 2^-24, Abar = max(|A_r|, |A_f|))
  choice    |dA_y||x|Abar_x^T + Abar_y|x||dA_x|^T (transposed for the adjoint), dA = A_f - A_r -- added on the GPU only: on the
            emulator nothing is fused and the strict bound must hold.
The constants count roundings: the blend has the two rounded lower weights, two products and one sum per row pair, one product and
one sum across rows (<= 6 on any path to an output); an adjoint sum of t terms rounds once per term and per weight (t_x + t_y) plus
the weight, the product and the two accumulations across the axes (4); the fused sum adds one rounding per term.

Measured, worst error as a share of the bound over all cases at input scales 1 and 1e4 (the tests print every figure, `-s` shows them):
  emulator (strict bound):   forward 0.52, adjoint 0.25, fused forward 0.32, fused adjoint 0.24
  MI355X (strict + choice):  forward 0.999, adjoint 0.961, fused forward 0.984, fused adjoint 0.999
By these figures the MI355X takes A_f throughout (the compiler contracts the product), so there the choice term is nearly all of
the bound and is nearly used up: what is left over is the rounding term. The figure that says how the arithmetic itself does is the
distance to the NEARER of A_r x A_r^T and A_f x A_f^T as a share of the strict bound (printed as EXCHANGE-NEARER, never asserted):
  MI355X:   forward 0.52, adjoint 0.25, fused forward 0.33, fused adjoint 0.23          emulator: the shares above (it takes A_r)

Sensitivity (each change made to csrc/cseg_bilinear.h in a scratch copy, emulated library rebuilt): tap budget + 3 -> + 0 fails b12_4x,
b12_tall, b40_12x, m_pow2, m_odd, two_low (routes; by value b12_4x, m_pow2, m_odd); row budget + 3 -> + 0 fails b8_row_margin by value;
ws <= 256 -> <= 512 fails g_ws260 by route and by value; `>= 0` in the masked band load fails every fused-sum case on a band with a
width that is a multiple of 4, stripe_one_low among them.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

U = 2.0 ** -24               # unit roundoff of float32
SCALES = (1.0, 1e4)
B = 2
MEASURED = {}                # (quantity, device type) -> worst error / bound seen in this process


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # (a copy: the cached case arrays are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _seed(kind, name):
    """A case's seed hangs on its name alone: adding a case leaves the others as they are."""
    return zlib.crc32(("%s/%s" % (kind, name)).encode()) & 0x7FFFFFFF


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# =================================================================================================================================
# reference operators
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def axis_ops(n_in, n_out):
    """The two dense float64 operators [n_out, n_in] of one axis, their difference, their envelope, the tap structure and t."""
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    o = np.arange(n_out)
    f = s * o.astype(np.float32)
    assert f.dtype == np.float32
    i0 = f.astype(np.int64)
    assert i0.min() >= 0 and i0.max() <= n_in - 1
    i1 = i0 + (i0 < n_in - 1)
    l1_r = f - i0.astype(np.float32)
    l1_f = (np.float64(s) * o - i0).astype(np.float32)           # the product is exact in float64: one rounding, as an fma makes

    def dense(l1):
        l0 = np.float32(1) - l1
        assert l0.dtype == np.float32
        A = np.zeros((n_out, n_in))
        np.add.at(A, (o, i0), l0.astype(np.float64))
        np.add.at(A, (o, i1), l1.astype(np.float64))
        return A
    Ar, Af = dense(l1_r), dense(l1_f)
    S = np.zeros((n_out, n_in))
    S[o, i0] = 1
    S[o, i1] = 1
    ops = dict(Ar=Ar, Af=Af, dA=np.abs(Af - Ar), Abar=np.maximum(np.abs(Ar), np.abs(Af)), S=S, t=int(S.sum(0).max()))
    for v in ops.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ops


def up_ref(x, h0, w0):
    """x float32 [B,C,h,w] (NaNs allowed) -> float64 expected upsampling to (h0, w0), magnitude term Abar|x|Abar^T, choice term, and
    the mask of outputs one of whose taps (zero-weight taps included: 0 * NaN is NaN on the device too) reads a NaN, and the value under
    the other rounding, A_f x A_f^T (reported, never asserted)."""
    y, xo = axis_ops(x.shape[2], h0), axis_ops(x.shape[3], w0)
    nan = np.isnan(x)
    x64 = np.where(nan, 0.0, x.astype(np.float64))
    ax = np.abs(x64)
    exp = y["Ar"] @ x64 @ xo["Ar"].T
    mag = y["Abar"] @ ax @ xo["Abar"].T
    choice = y["dA"] @ ax @ xo["Abar"].T + y["Abar"] @ ax @ xo["dA"].T
    alt = y["Af"] @ x64 @ xo["Af"].T
    return exp, mag, choice, (y["S"] @ nan.astype(np.float64) @ xo["S"].T) > 0, alt


def adj_ref(g, hs, ws):
    """g float32 [B,C,h0,w0] -> float64 expected adjoint on (hs, ws), magnitude term, choice term, t_x + t_y + 4, value under A_f."""
    y, xo = axis_ops(hs, g.shape[2]), axis_ops(ws, g.shape[3])
    g64 = g.astype(np.float64)
    ag = np.abs(g64)
    exp = y["Ar"].T @ g64 @ xo["Ar"]
    mag = y["Abar"].T @ ag @ xo["Abar"]
    choice = y["dA"].T @ ag @ xo["Abar"] + y["Abar"].T @ ag @ xo["dA"]
    return exp, mag, choice, xo["t"] + y["t"] + 4, y["Af"].T @ g64 @ xo["Af"]


def _bound(k, mag, choice, dev):
    return k * U * mag + (choice if dev.type == "cuda" else 0.0)


def check(quantity, dev, got, exp, bound, nan=None, strict=None, alt=None):
    """|got - exp| <= bound pointwise; NaN exactly where `nan` says (nowhere by default). Prints and records the worst share. With
    `strict` and `alt` it also prints (and only prints) the distance to the nearer of the two roundings as a share of the strict bound:
    on the GPU, where the choice term is most of the bound, that is the figure that says how the arithmetic itself does."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == exp.shape, (quantity, got.dtype, got.shape, exp.shape)
    nan = np.zeros(exp.shape, bool) if nan is None else nan
    assert np.array_equal(np.isnan(got), nan), "%s: %d NaN where %d are due" % (quantity, np.isnan(got).sum(), nan.sum())
    ok = ~nan
    assert np.isfinite(got[ok]).all(), quantity
    err = np.abs(got.astype(np.float64) - exp)[ok]
    bnd = np.broadcast_to(bound, exp.shape)[ok]
    share = float((err / np.where(bnd > 0, bnd, 1.0))[bnd > 0].max()) if (bnd > 0).any() else 0.0
    print("EXCHANGE-SHARE %s %s %.3f" % (quantity, dev.type, share))
    key = (quantity, dev.type)
    MEASURED[key] = max(MEASURED.get(key, 0.0), share)
    if alt is not None:
        near = np.minimum(err, np.abs(got.astype(np.float64) - alt)[ok])
        sb = np.broadcast_to(strict, exp.shape)[ok]
        fig = float((near / np.where(sb > 0, sb, 1.0))[sb > 0].max()) if (sb > 0).any() else 0.0
        print("EXCHANGE-NEARER %s %s %.3f" % (quantity, dev.type, fig))
        MEASURED[key + ("nearer",)] = max(MEASURED.get(key + ("nearer",), 0.0), fig)
    assert (err[bnd == 0] == 0).all(), "%s: nonzero where every input is zero" % quantity
    assert share <= 1.0, "%s: worst error is %.3g of its bound (max error %.3g)" % (quantity, share, err.max())
    return share


def plan(K, hs, ws, h0, w0):
    taps, rows, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_long(-1)
    route = K._hip.lib().cseg_bilinear_adjoint_plan(hs, ws, h0, w0, ctypes.byref(taps), ctypes.byref(rows), ctypes.byref(lds))
    return route, taps.value, rows.value, lds.value


GATHER = 0
# name -> (fine (h0, w0), [coarse (hs, ws)], [route of each coarse map])
SHAPES = {
    # band kernel, 8 taps
    "b8_pow2": ((16, 32), [(8, 16)], [8]),
    "b8_odd": ((13, 21), [(7, 11)], [8]),                        # two bands, the last one partial; scalar loads (21 % 4 != 0)
    "b8_scale_near_1": ((17, 40), [(16, 39)], [8]),
    "b8_wide": ((9, 300), [(5, 255)], [8]),                      # 255 coarse columns: one idle lane in the horizontal pass
    "b8_ws256_55k": ((4, 512), [(2, 256)], [8]),                 # ws == 256 and 55 296 bytes of LDS: both limits from inside
    "b8_row_margin": ((13, 12), [(10, 6)], [8]),                 # the band of coarse rows 4..7 spans fine rows 4..10: (int)(5 / sy) + 1 rows
    # band kernel, 12 / 24 / 40 taps
    "b12_4x": ((16, 32), [(4, 8)], [12]),
    "b12_tall": ((64, 4), [(3, 2)], [12]),
    "b24_8x": ((16, 32), [(2, 4)], [24]),
    "b24_odd": ((24, 36), [(3, 5)], [24]),
    "b40_12x": ((36, 36), [(4, 4)], [40]),
    "b40_16x": ((48, 16), [(6, 2)], [40]),
    # gather kernel
    "g_lds": ((32, 192), [(2, 12)], [GATHER]),                   # 37 taps would do, but a band of 158 rows needs 126 KB
    "g_ws260": ((4, 520), [(2, 260)], [GATHER]),                 # ws > 256 (7 taps, 55 KB: nothing else refuses the band)
    "g_taps": ((40, 44), [(2, 3)], [GATHER]),                    # 46 taps
    "g_1x1": ((8, 48), [(1, 1)], [GATHER]),                      # scale 0 on both axes: every fine pixel on one coarse pixel
    "g_col": ((8, 48), [(8, 1)], [GATHER]),                      # scale 0 across, 1 down
    # degenerate
    "d_one_row": ((8, 48), [(1, 48)], [8]),
    "d_same_size": ((5, 7), [(5, 7)], [8]),                      # identity: bit for bit
    "d_fine_row": ((1, 8), [(1, 4)], [8]),
    "d_fine_col": ((6, 1), [(3, 1)], [8]),
    "d_1x1": ((1, 1), [(1, 1)], [8]),
    "d_70_rows": ((70, 8), [(4, 8)], [8]),                       # one band of all 70 fine rows
    # several coarse maps at once
    "m_pow2": ((16, 32), [(8, 16), (4, 8), (2, 4)], [8, 12, 24]),
    "m_odd": ((24, 36), [(12, 18), (6, 9), (3, 5)], [8, 12, 24]),
}
DOWN = ((4, 8), [(8, 16)], [8])                                  # downsampling: upcat takes it, fuse_sum refuses it
UPCAT_CASES = dict(SHAPES, down=DOWN)


def check_routes(K, fine, lows, routes):
    for (hs, ws), want in zip(lows, routes):
        route, taps, rows, lds = plan(K, hs, ws, fine[0], fine[1])
        assert route == want, "(%d,%d)<-(%d,%d): route %d (taps %d, rows %d, %d bytes), the case is built for %d" % (
            fine + (hs, ws, route, taps, rows, lds, want))
        assert route in (0, 8, 12, 24, 40) and (route == 0 or (taps <= route and ws <= 256 and lds <= 65536))
        assert lds == 4 * rows * (fine[1] + ws)


def check_route_reasons(K):
    """Each gather case leaves the band for the one reason it is named after, and the 55 KB case sits inside all three limits."""
    assert plan(K, 2, 256, 4, 512) == (8, 7, 18, 55296)
    route, taps, rows, lds = plan(K, 2, 12, 32, 192)
    assert route == 0 and taps <= 40 and lds > 65536
    route, taps, rows, lds = plan(K, 2, 260, 4, 520)
    assert route == 0 and taps <= 8 and lds <= 65536
    route, taps, rows, lds = plan(K, 2, 3, 40, 44)
    assert route == 0 and taps > 40 and lds <= 65536
    assert plan(K, 1, 1, 8, 48)[:2] == (0, 48) and plan(K, 8, 1, 8, 48)[:2] == (0, 48)
    assert {route for c in SHAPES.values() for route in c[2]} == {0, 8, 12, 24, 40}


# =================================================================================================================================
# upsample + concat
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def upcat_case(name, scale):
    fine, lows, routes = UPCAT_CASES[name]
    i = _seed("upcat", name)
    rs = np.random.RandomState(i)
    chans = [2 + (i + 2 * k) % 3 for k in range(len(lows) + 1)]
    xs = [(rs.standard_normal((B, c) + s) * scale).astype(np.float32) for c, s in zip(chans, [fine] + lows)]
    g = (rs.standard_normal((B, sum(chans)) + fine) * scale).astype(np.float32)
    fwd = [up_ref(x, *fine) for x in xs[1:]]
    offs = np.cumsum([0] + chans)
    adj = [adj_ref(g[:, offs[k + 1]:offs[k + 2]], *lows[k]) for k in range(len(lows))]
    for a in xs + [g]:
        a.setflags(write=False)
    return dict(fine=fine, lows=lows, routes=routes, chans=chans, offs=offs, xs=xs, g=g, fwd=fwd, adj=adj)


def run_upcat(K, dev, name):
    fine, lows, routes = UPCAT_CASES[name]
    check_routes(K, fine, lows, routes)
    for scale in SCALES:
        c = upcat_case(name, scale)
        offs = c["offs"]
        assert len(set(c["chans"])) > 1 and all(2 <= ch <= 4 for ch in c["chans"])
        xs = [_t(x, dev).requires_grad_(True) for x in c["xs"]]
        out = K.upsample_concat(xs)
        got = _np(out)
        assert got.shape == (B, offs[-1]) + fine
        assert np.array_equal(_bits(got[:, :offs[1]]), _bits(c["xs"][0])), "pass-through channels"
        for k, (exp, mag, choice, nan, alt) in enumerate(c["fwd"]):
            part = got[:, offs[k + 1]:offs[k + 2]]
            check("forward", dev, part, exp, _bound(6, mag, choice, dev), strict=6 * U * mag, alt=alt)
            if lows[k] == fine:
                assert np.array_equal(_bits(part), _bits(c["xs"][k + 1])), "same size: the upsampling is the identity"
        g = _t(c["g"], dev)
        grads = [_np(t) for t in torch.autograd.grad(out, xs, g)]
        assert np.array_equal(_bits(grads[0]), _bits(c["g"][:, :offs[1]])), "gradient of the pass-through channels"
        for k, (exp, mag, choice, kk, alt) in enumerate(c["adj"]):
            assert grads[k + 1].shape == (B, c["chans"][k + 1]) + lows[k]
            check("adjoint", dev, grads[k + 1], exp, _bound(kk, mag, choice, dev), strict=kk * U * mag, alt=alt)
            if lows[k] == fine:
                assert np.array_equal(_bits(grads[k + 1]), _bits(c["g"][:, offs[k + 1]:offs[k + 2]])), "same size: adjoint of the identity"
        # the needs_input_grad holes: the gradient of the last coarse map alone (no pass-through copy, no other adjoint) is the same bits
        xs2 = [_t(x, dev) for x in c["xs"]]
        xs2[-1].requires_grad_(True)
        (alone,) = torch.autograd.grad(K.upsample_concat(xs2), [xs2[-1]], g)
        assert np.array_equal(_bits(_np(alone)), _bits(grads[-1]))


# =================================================================================================================================
# fused sum + ReLU
# =================================================================================================================================
def _fuse_table():
    t = {}
    for i, (name, (fine, lows, routes)) in enumerate(SHAPES.items()):
        t[name] = dict(fine=fine, lows=lows, routes=routes, n_same=1 + i % 4, C=2 + i % 3)
    t["g_lds"]["C"] = 4                                          # the largest tensor of the file: 2 x 4 x 32 x 192
    t["two_low"] = dict(fine=(13, 21), lows=[(7, 11), (4, 6)], routes=[8, 12], n_same=3, C=3)
    t["no_low"] = dict(fine=(13, 21), lows=[], routes=[], n_same=4, C=2)
    # planted: same[1] = -same[0] on a stripe of rows; with a coarse term its rows under the stripe are zero, so the sum is exactly 0
    t["stripe_no_low"] = dict(fine=(16, 32), lows=[], routes=[], n_same=2, C=3, stripe=(3, 5))
    t["stripe_one_low"] = dict(fine=(16, 32), lows=[(8, 16)], routes=[8], n_same=2, C=2, stripe=(0, 2))
    # planted: one NaN in a same-resolution term and one in a coarse term (vector and scalar forward kernel)
    t["nan_vec"] = dict(fine=(16, 32), lows=[(8, 16), (2, 4)], routes=[8, 24], n_same=2, C=3, nan=True)
    t["nan_scalar"] = dict(fine=(13, 21), lows=[(7, 11)], routes=[8], n_same=3, C=2, nan=True)
    return t


FUSE_CASES = _fuse_table()


@functools.lru_cache(maxsize=None)
def fuse_case(name, scale):
    c = FUSE_CASES[name]
    fine, lows, n_same, C = c["fine"], c["lows"], c["n_same"], c["C"]
    rs = np.random.RandomState(_seed("fuse", name))
    same = [(rs.standard_normal((B, C) + fine) * scale).astype(np.float32) for _ in range(n_same)]
    low = [(rs.standard_normal((B, C) + s) * scale).astype(np.float32) for s in lows]
    g = (rs.standard_normal((B, C) + fine) * scale).astype(np.float32)
    planted = np.zeros((B, C) + fine, bool)
    if "stripe" in c:
        r0, r1 = c["stripe"]
        same[1][:, :, r0:r1] = -same[0][:, :, r0:r1]
        planted[:, :, r0:r1] = True
        for l in low:                                            # zero the coarse rows any tap of the stripe reads
            S = axis_ops(l.shape[2], fine[0])["S"]
            l[:, :, S[r0:r1].sum(0) > 0] = 0.0
    if c.get("nan"):
        same[-1][1, C - 1, 3, 5] = np.nan
        low[0][0, 1, 2, 3] = np.nan
    ups = [up_ref(l, *fine) for l in low]
    nan = np.zeros((B, C) + fine, bool)
    pre = np.zeros((B, C) + fine)
    mag = np.zeros((B, C) + fine)
    choice = np.zeros((B, C) + fine)
    pre_f = np.zeros((B, C) + fine)
    for s in same:
        nan |= np.isnan(s)
        s64 = np.where(np.isnan(s), 0.0, s.astype(np.float64))
        pre += s64
        pre_f += s64
        mag += np.abs(s64)
    for exp, m, ch, nn, alt in ups:
        pre += exp
        pre_f += alt
        mag += m
        choice += ch
        nan |= nn
    for a in same + low + [g]:
        a.setflags(write=False)
    return dict(c, same=same, low=low, g=g, pre=pre, mag=mag, choice=choice, nan=nan, planted=planted, pre_f=pre_f,
                k=n_same + len(lows) + 6)


def _lib_fuse_bwd_unmasked(K, g, lows, shape):
    """cseg_fuse_sum_bwd with out_act = NULL and g_same = NULL: the third route, the adjoint of d_out itself."""
    Bn, C, h, w = shape
    d_low = [torch.full((Bn, C) + s, 7.0, dtype=torch.float32, device=g.device) for s in lows]
    dl = (ctypes.c_void_p * len(d_low))(*[t.data_ptr() for t in d_low])
    K._hip.call("cseg_fuse_sum_bwd", K._p(g, torch.float32, "d_out"), None, K._int_arr([s[0] for s in lows]),
                K._int_arr([s[1] for s in lows]), len(lows), Bn, C, h, w, None, dl, K._hip.stream_ptr())
    return d_low


def run_fuse(K, dev, name, monkeypatch):
    cfg = FUSE_CASES[name]
    fine, lows = cfg["fine"], cfg["lows"]
    check_routes(K, fine, lows, cfg["routes"])
    monkeypatch.setattr(K, "FUSE_SUM_AMAX", bool(cfg.get("nan")))   # the NaN cases also look at the max|.| record the kernel can leave
    for scale in SCALES:
        c = fuse_case(name, scale)
        n_same, pre, nan, planted = c["n_same"], c["pre"], c["nan"], c["planted"]
        assert 1 <= n_same <= 4 and 0 <= len(lows) <= 3
        strict = c["k"] * U * c["mag"]
        bound = strict + (c["choice"] if dev.type == "cuda" else 0.0)
        # a property of the reference alone, under the wider (GPU) bound: next to no element sits so close to 0 that its mask is open
        near = (np.abs(pre) <= strict + c["choice"]) & ~planted & ~nan
        assert near.sum() <= 1e-3 * pre.size, "%d of %d pre-activations inside the bound: pick another seed" % (near.sum(), pre.size)
        assert (pre[planted] == 0).all() and (not planted.any() or (strict[planted] > 0).all())

        same = [_t(s, dev).requires_grad_(True) for s in c["same"]]
        low = [_t(l, dev).requires_grad_(True) for l in c["low"]]
        out_t = K.fuse_sum_relu(same, low)
        out = _np(out_t)
        check("fused forward", dev, out, np.maximum(pre, 0.0), bound, nan=nan, strict=strict, alt=np.maximum(c["pre_f"], 0.0))
        decided = (np.abs(pre) > bound) & ~nan
        assert np.array_equal((out > 0)[decided], (pre > 0)[decided]), "ReLU mask away from 0"
        assert (_bits(out[planted]) == 0).all(), "planted stripe: the sum is exactly +0"
        if cfg.get("nan"):
            assert nan.sum() > 1 and not nan.all()
            if K.split_arith_id():                                # the record skips NaN: it is the maximum of the finite outputs
                rec = K.known_amax(out_t)
                assert rec is not None and float(_np(rec.view(torch.float32)).max()) == float(np.nanmax(np.abs(out)))

        g = _t(c["g"], dev)
        mask = out > 0                                           # the kernel's own mask (NaN > 0 is false, as in the kernel)
        gm = np.where(mask, c["g"], np.float32(0))
        grads = [_np(t) for t in torch.autograd.grad(out_t, same + low, g)]
        for k in range(n_same):
            assert np.array_equal(_bits(grads[k]), _bits(gm)), "same-resolution gradient %d" % k
        assert (_bits(grads[0][planted]) == 0).all(), "planted stripe: the gradient is exactly +0"
        if not lows:
            continue
        refs = [adj_ref(gm, *s) for s in lows]
        for k, (exp, m, ch, kk, alt) in enumerate(refs):
            check("fused adjoint", dev, grads[n_same + k], exp, _bound(kk, m, ch, dev), strict=kk * U * m, alt=alt)
        # only coarse gradients wanted: the mask is fused into the adjoint -- the same bits as through the materialised masked gradient
        # (a forward of its own whose same-resolution terms ask for no gradient: needs_input_grad follows the inputs, not the query)
        low2 = [_t(l, dev).requires_grad_(True) for l in c["low"]]
        out2 = K.fuse_sum_relu([_t(s, dev) for s in c["same"]], low2)
        assert np.array_equal(_bits(_np(out2)), _bits(out))
        fused = [_np(t) for t in torch.autograd.grad(out2, low2, g)]
        for k in range(len(lows)):
            assert np.array_equal(_bits(fused[k]), _bits(grads[n_same + k])), "coarse gradient %d: fused mask vs materialised" % k
        # no activation at all: the adjoint of d_out itself
        plain = _lib_fuse_bwd_unmasked(K, g, lows, out.shape)
        for k, s in enumerate(lows):
            exp, m, ch, kk, alt = adj_ref(c["g"], *s)
            check("fused adjoint", dev, _np(plain[k]), exp, _bound(kk, m, ch, dev), strict=kk * U * m, alt=alt)


# =================================================================================================================================
# plain n-ary sum
# =================================================================================================================================
def _terms(n, w, seed):
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal((B, 3, 5, w)) * 10.0 ** rs.randint(-2, 3)).astype(np.float32) for _ in range(n)]


def _left_to_right(terms):
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    assert acc.dtype == np.float32
    return acc


def run_sum(K, dev, n, w):
    """sum_same and FanOutSum (2..4 gradients: the kernel) are the left-to-right fp32 sum, bit for bit."""
    terms = _terms(n, w, 3000 + 10 * n + w)
    want = _left_to_right(terms)
    got = _np(K.sum_same([_t(t, dev) for t in terms]))
    assert np.array_equal(_bits(got), _bits(want))
    x = _t(terms[0], dev).requires_grad_(True)
    outs = K.fan_out(x, n)
    assert len(outs) == n
    (gx,) = torch.autograd.grad(outs, [x], [_t(t, dev) for t in terms])
    assert np.array_equal(_bits(_np(gx)), _bits(want))


def run_fanout_fallback(K, dev):
    """Five gradients are more than the kernel takes: FanOutSum adds them with torch, within 4 roundings of the float64 sum."""
    terms = _terms(5, 7, 3333)
    x = _t(terms[0], dev).requires_grad_(True)
    (gx,) = torch.autograd.grad(K.fan_out(x, 5), [x], [_t(t, dev) for t in terms])
    exp = sum(t.astype(np.float64) for t in terms)
    mag = sum(np.abs(t.astype(np.float64)) for t in terms)
    err = np.abs(_np(gx).astype(np.float64) - exp)
    assert (err <= 4 * U * mag).all(), float((err / (4 * U * mag)).max())


# =================================================================================================================================
# refusals
# =================================================================================================================================
def _z(dev, *shape):
    return torch.zeros(*shape, dtype=torch.float32, device=dev)


def _lib_upcat_fwd(K, feats, out):
    ptrs = (ctypes.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
    ia = lambda k: K._int_arr([f.shape[k] for f in feats])
    K._hip.call("cseg_upcat_fwd", ptrs, ia(1), ia(2), ia(3), len(feats), feats[0].shape[0], K._pf(out), K._hip.stream_ptr())


def _lib_fuse_fwd(K, same, low, out):
    sp = (ctypes.c_void_p * max(1, len(same)))(*([t.data_ptr() for t in same] or [None]))
    lp = (ctypes.c_void_p * max(1, len(low)))(*([t.data_ptr() for t in low] or [None]))
    Bn, C, h, w = out.shape
    K._hip.call("cseg_fuse_sum_fwd", sp, len(same), lp, K._int_arr([t.shape[2] for t in low] or [1]),
                K._int_arr([t.shape[3] for t in low] or [1]), len(low), Bn, C, h, w, 1, K._pf(out), K._hip.stream_ptr())


# what -> (which wrapper, shapes of its operands, the message it must raise with)
REFUSALS = {
    "upcat_five_maps": ("upcat", [(1, 2, 4, 4)] * 5, r"upcat: n_maps=5 not in \[1,4\]"),
    "upcat_empty_map": ("upcat", [(2, 3, 4, 8), (2, 0, 2, 4)], "upcat: empty map 1"),
    "upcat_empty_rows": ("upcat", [(2, 3, 4, 8), (2, 2, 0, 4)], "upcat: empty map 1"),
    "upcat_65536_channels": ("upcat", [(1, 65536, 1, 4)], "upcat: grid too large"),
    "upcat_65536_channels_in_two_maps": ("upcat", [(1, 65535, 1, 4), (1, 1, 1, 2)], "upcat: grid too large"),
    "fuse_five_same": ("fuse", ([(2, 3, 4, 8)] * 5, []), "fuse_sum: n_same=5 n_low=0 out of range"),
    "fuse_four_low": ("fuse", ([(2, 3, 4, 8)], [(2, 3, 2, 4)] * 4), "fuse_sum: n_same=1 n_low=4 out of range"),
    "fuse_empty_map": ("fuse", ([(2, 3, 0, 8)], []), "fuse_sum: bad shape"),
    "fuse_65536_channels": ("fuse", ([(1, 65536, 1, 4)], []), "fuse_sum: bad shape"),
    "fuse_downsampling": ("fuse", ([(2, 3, 4, 8)], [(2, 3, 8, 16)]), "fuse_sum: coarse term 0 is 8x16 for a 4x8 output"),
    "fuse_coarse_wider": ("fuse", ([(2, 3, 4, 8)], [(2, 3, 2, 4), (2, 3, 2, 9)]), "fuse_sum: coarse term 1 is 2x9 for a 4x8 output"),
    "fuse_no_same": ("fuse", ([], [(2, 3, 2, 4)]), "fuse_sum_relu needs at least one same-resolution term"),
}


def run_refusal(K, dev, what):
    kind, shapes, msg = REFUSALS[what]
    if kind == "upcat":
        feats = [_z(dev, *s) for s in shapes]
        with pytest.raises(RuntimeError, match=msg):
            K.upsample_concat(feats)
        out = torch.full((shapes[0][0], sum(s[1] for s in shapes)) + tuple(shapes[0][2:]), 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match=msg):
            _lib_upcat_fwd(K, feats, out)
    else:
        same, low = [_z(dev, *s) for s in shapes[0]], [_z(dev, *s) for s in shapes[1]]
        with pytest.raises(RuntimeError, match=msg):
            K.fuse_sum_relu(same, low)
        if not same:                                             # the wrapper's own check; the library takes coarse terms alone
            return
        out = torch.full(shapes[0][0], 7.0, dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match=msg):
            _lib_fuse_fwd(K, same, low, out)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to its output"
