"""Exact-operand cases for the convolution kernels: operands chosen so that NOTHING is rounded anywhere in the split arithmetic
(csrc/cseg_split.h) or in the fp32 accumulation, so every kernel must reproduce the float64 convolution BIT FOR BIT -- in all three
directions, at any shape, whatever the tile form, the split-K partition or the order of the sums. A plain module (like
tests/golden_wide_cases.py): generators, float64 references and per-family runners that take a device; the emulated-device file
(tests/test_emu_exact_operands.py) and the MI355X file (tests/test_gpu_exact_operands.py) are thin users of it.

Why exact
---------
* Dense small integers. Both operands are integers in [-7, 7]: exact in bf16, and in fp16 after any power-of-two scale, so every
  `lo` piece is zero and every piece product is exact in fp32. Every partial sum is an integer multiple of one unit with magnitude
  below 2^24 units as long as  9 * Cin * 49 < 2^24  (forward, backward-data) and  B * H * W * 49 < 2^24  (weight gradient) -- asserted
  per case -- so fp32 accumulation is exact in ANY order: MFMA-internal order, split-K partial sums, the reduce kernels.
* Wide impulses. One operand is sparse -- at most one non-zero element per (image, channel), placed so that every output element
  receives at most ONE product (asserted: the float64 operator applied to the operands' non-zero indicators is <= 1 everywhere) -- the
  other is dense.
    wide_a:  the sparse operand holds integers that need BOTH pieces (odd, 20-21 bits, mixed signs), the dense one is drawn from
             {0, +-1, +-2, +-4}: the product fits 24 bits and the result is hi * w + lo * w exactly;
    wide_b:  the sparse operand holds {+-1, +-2, +-4}, the dense one odd integers of 13-21 bits in (-2^21, 2^21).
  Between them the two pin both cross terms (a0 b1, a1 b0) and the piece-to-term mapping (ta / tb) separately; the dropped a1 b1 is
  zero by construction. Generator rule: every non-zero element of a wide tensor lies within a factor 2^10 of that tensor's max|.|
  (asserted), so every lo piece is at least 2^-24 in scaled units and representable (the per-tensor scale puts max|s x| into
  [2^14, 2^15); an element 2^18 below the maximum loses its lo piece, as the header says). wide_a plants on purpose: one element equal
  to max|.| that is exactly a power of two (2^21); one element m * 2^-10 * (1 + 2^-23) with m = 2^21, whose lo piece (2^-19 in scaled
  units) is an fp16 SUBNORMAL; one element 2^21 - 2^-3 = 2^k - 2^(k-24), whose hi piece rounds up into the next binade (lo < 0).
  bf16x6 splits 24 bits into 8 + 8 + 8 exactly and keeps every product of a piece with a one-piece operand, so the same cases are
  exact there. Impulses sit at the four corners, on each edge, at ragged-tile boundaries in the interior (row 4, column 64 of a
  65-wide map) and closer than the dilation to each border.
* Power-of-two magnitudes. The dense-integer case with x * 2^40 and w * 2^-30, and the mirror image: scaling changes no mantissa bit,
  so the result is the dense reference times 2^10, exactly -- a wrong or missing per-tensor scale / un-scale shows.
* Degenerate operands. All-zero x, w or dy (split_amax_exp clamps the exponent of an empty max|.| record: "any finite scale"),
  constants (every element the same power of two: border outputs count taps, 4 / 6 / 9 times Cin * c * w).
* BEFORE any kernel runs, operands() asserts on the CPU that the float64 reference survives a round trip through fp32: the inputs,
  not the kernel, carry the exactness.
Hardware exactness is derived from the above (fp16 / bf16 products are exact in the matrix cores' fp32 accumulators, fp16 subnormal
inputs are kept), then observed: the split-operand arithmetic section of DESIGN.md has the date of the run."""
import functools
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F16X3, BF16X6 = "f16x3", "bf16x6"
EXACT_KINDS = ("dense", "wide_a", "wide_b", "pow2", "pow2_mirror")
DEGENERATE_KINDS = ("zero_a", "zero_b", "const")
WIDE_MAX = 2.0 ** 21
SPECIALS = (WIDE_MAX,                                  # max|.|, exactly a power of two
            WIDE_MAX * 2.0 ** -10 * (1.0 + 2.0 ** -23),  # lo piece = 2^-19 in scaled units: an fp16 subnormal
            -(WIDE_MAX - 2.0 ** -3))                    # 2^k - 2^(k-24): hi rounds up into the next binade, lo is negative


class Geo(object):
    """The operator: k x k kernel, stride, dilation, padding = dilation * (k // 2)."""

    def __init__(self, k=3, stride=1, dil=1):
        self.k, self.stride, self.dil = k, stride, dil
        self.pad = dil * (k // 2)

    def key(self):
        return (self.k, self.stride, self.dil)

    def shapes(self, case):
        """case = (B, Cin, Cout, Ho, Wo): the OUTPUT map, as in the stride-2 tables (stride 1: the same map)."""
        B, ci, co, Ho, Wo = case
        return (B, ci, Ho * self.stride, Wo * self.stride), (co, ci, self.k, self.k), (B, co, Ho, Wo)

    def ref(self, direction, a, b, case):
        xs, ws, ys = self.shapes(case)
        a, b = a.double(), b.double()
        s, p, d = self.stride, self.pad, self.dil
        if direction == "fwd":
            return F.conv2d(a, b, None, s, p, d)
        if direction == "bwd":
            return torch.nn.grad.conv2d_input(xs, b, a, s, p, d)
        return torch.nn.grad.conv2d_weight(a, ws, b, s, p, d)

    def operand_shapes(self, direction, case):
        xs, ws, ys = self.shapes(case)
        return {"fwd": (xs, ws), "bwd": (ys, ws), "wrw": (xs, ys)}[direction]


def _gen(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ints(shape, rng, lo=-7, hi=7):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float32))


def _narrow_dense(shape, rng):
    return torch.from_numpy(rng.choice(np.array([0, 1, -1, 2, -2, 4, -4], dtype=np.float32), size=shape))


def _narrow_nonzero(n, rng):
    return rng.choice(np.array([1, -1, 2, -2, 4, -4], dtype=np.float64), size=n)


def _wide_dense(shape, rng):
    bits = rng.integers(13, 22, size=shape)                              # 13 .. 21 significant bits
    mag = (1 << (bits - 1)) | rng.integers(0, 1 << 20, size=shape) % (1 << (bits - 1)) | 1
    return torch.from_numpy((mag * rng.choice([-1, 1], size=shape)).astype(np.float32))


def _wide_values(n, rng):
    """odd integers of 20-21 bits with mixed signs; the first three are the planted elements"""
    mag = rng.integers(1 << 19, 1 << 21, size=n) | 1
    v = (mag * rng.choice([-1, 1], size=n)).astype(np.float64)
    v[:len(SPECIALS)] = SPECIALS[:n]
    return v


def _sites(geo, direction, shape, rng, want=28):
    """[(b, c, r, col)]: at most one per (image, channel); within an image no two whose products could meet in one output element
    (the weight gradient sums over images and pixels instead: one site per CHANNEL there)."""
    B, C, H, W = shape
    d = geo.dil
    if geo.k == 1:
        off = {0}
    elif geo.stride == 2:
        off = set(range(-2, 3))
    else:
        off = {0, d, -d, 2 * d, -2 * d}
    rows = [r for r in (0, H - 1, H // 2, 3, 4, 7, 8, d - 1, H - d, 1) if 0 <= r < H]
    cols = [c for c in (0, W - 1, W // 2, 63, 64, 3, 4, 31, 32, d - 1, W - d, 1) if 0 <= c < W]
    cand = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    cand += [(r, c) for c in cols[3:] for r in rows[2:]] + list(itertools.product(rows, cols))
    cand += [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(40)]
    chans = [c for c in (0, C - 1, 15, 16, 31, 32, 47, 48, 63, 64, C // 2, 1) if 0 <= c < C]
    chans = list(dict.fromkeys(chans + list(range(C))))
    sites, used_bc, used_c, nxt = [], set(), set(), 0
    for pos in dict.fromkeys(cand):
        if len(sites) >= want:
            break
        placed = False
        for b in [(len(sites) + i) % B for i in range(B)]:
            if direction != "wrw" and any(sb == b and (pos[0] - r) in off and (pos[1] - c) in off for sb, _, r, c in sites):
                continue
            for j in range(len(chans)):
                ch = chans[(nxt + j) % len(chans)]
                if (b, ch) in used_bc or (direction == "wrw" and ch in used_c):
                    continue
                sites.append((b, ch, pos[0], pos[1]))
                used_bc.add((b, ch))
                used_c.add(ch)
                nxt = (nxt + j + 1) % len(chans)
                placed = True
                break
            if placed:
                break
    return sites


def _sparse(shape, sites, values):
    t = torch.zeros(shape, dtype=torch.float64)
    for (b, c, r, col), v in zip(sites, values):
        t[b, c, r, col] = v
    f = t.float()
    assert torch.equal(f.double(), t), "a planted value is not an fp32 number"
    return f


def _check_wide_rule(t):
    nz = t[t != 0].abs()
    assert float(nz.min()) * 2.0 ** 10 >= float(nz.max()), "generator rule: non-zero elements within 2^10 of the tensor's maximum"


@functools.lru_cache(maxsize=None)
def _operands(geo_key, direction, kind, case, with_bias, with_addend):
    geo = Geo(*geo_key)
    sa, sb = geo.operand_shapes(direction, case)
    dense_based = ("dense", "pow2", "pow2_mirror", "zero_a", "zero_b")          # (the same integers under every one of these)
    rng = _gen(geo_key, direction, "dense" if kind in dense_based else kind, case)
    B, ci, co, Ho, Wo = case
    if kind in dense_based:
        a, b = _ints(sa, rng), _ints(sb, rng)
        if direction == "wrw":
            assert sa[0] * sa[2] * sa[3] * 49 < 2 ** 24
        else:
            assert geo.k * geo.k * max(ci, co) * 49 < 2 ** 24
        if kind == "pow2":
            a, b = a * 2.0 ** 40, b * 2.0 ** -30
        elif kind == "pow2_mirror":
            a, b = a * 2.0 ** -30, b * 2.0 ** 40
        elif kind == "zero_a":
            a = torch.zeros_like(a)
        elif kind == "zero_b":
            b = torch.zeros_like(b)
    elif kind == "const":
        a, b = torch.full(sa, 8.0), torch.full(sb, 0.25)
    elif kind in ("wide_a", "wide_b"):
        sites = _sites(geo, direction, sa, rng)
        assert len(sites) >= 6, "too few impulses placed"
        if kind == "wide_a":
            a, b = _sparse(sa, sites, _wide_values(len(sites), rng)), _narrow_dense(sb, rng)
            _check_wide_rule(a)
            assert float(a.abs().max()) == WIDE_MAX and len(sites) >= len(SPECIALS)          # (all three planted elements are in)
        else:
            a, b = _sparse(sa, sites, _narrow_nonzero(len(sites), rng)), _wide_dense(sb, rng)
            _check_wide_rule(b)
        count = geo.ref(direction, (a != 0).float(), (b != 0).float(), case)
        assert float(count.max()) == 1.0, "every output element must receive at most one product (and some must receive one)"
    else:
        raise ValueError(kind)
    ref = core = geo.ref(direction, a, b, case)
    bias = addend = None
    if with_bias:
        bias = _ints((ref.shape[1],), rng)
        ref = ref + bias.double().view(1, -1, 1, 1)
    if with_addend:
        addend = _ints(tuple(ref.shape), rng)
        ref = ref + addend.double()
    assert kind not in ("wide_a", "wide_b") or (bias is None and addend is None)       # (24-bit products leave no room for an addend)
    assert torch.equal(ref.float().double(), ref), "the float64 reference is not an fp32 number: the case broke its own exactness rule"
    assert bool(torch.isfinite(ref).all())
    if kind == "pow2" or kind == "pow2_mirror":
        base = _operands(geo_key, direction, "dense", case, False, False)[2]
        assert torch.equal(core, base * 2.0 ** 10)
    if kind in ("zero_a", "zero_b"):
        want = torch.zeros_like(ref)
        if bias is not None:
            want = want + bias.double().view(1, -1, 1, 1)
        if addend is not None:
            want = want + addend.double()
        assert torch.equal(ref, want)
    if kind == "const" and direction == "fwd" and geo.k == 3 and geo.stride == 1 and geo.dil == 1 and Ho > 2 and Wo > 2 and not (with_bias or with_addend):
        unit = ci * 8.0 * 0.25
        assert float(ref[0, 0, 0, 0]) == 4 * unit and float(ref[0, 0, 0, 1]) == 6 * unit and float(ref[0, 0, 1, 1]) == 9 * unit
    return a, b, ref, bias, addend


def operands(geo, direction, kind, case, with_bias=False, with_addend=False):
    """-> (a, b, ref float64, bias, addend) on the CPU, computed once per case and shared (never modified by the callers).
    a / b: fwd (x, w), bwd (dy, w), wrw (x, dy)."""
    return _operands(geo.key(), direction, kind, tuple(case), bool(with_bias), bool(with_addend))


def check(out, ref, what):
    assert tuple(out.shape) == tuple(ref.shape), (what, tuple(out.shape), tuple(ref.shape))
    out = out.detach().cpu()
    assert bool(torch.isfinite(out).all()), (what, "non-finite output")
    if not torch.equal(out.double(), ref):
        bad = (out.double() != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ from float64; first at %s: got %r want %r"
                             % (what, bad.shape[0], ref.numel(), i, float(out[i]), float(ref[i])))


# ---- the kernel families: how each direction is called through contrastiveseg_amd/kernels.py ---------------------------------------
def setup(K, monkeypatch, arith=F16X3, env=None):
    """The monkeypatching of the existing kernel tests: arithmetic, a fresh pack cache, every shape on the project's kernels."""
    monkeypatch.setattr(K, "SPLIT_ARITH", arith)
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 1)
    monkeypatch.setattr(K, "CONV1X1_SB_MIN_TILES", 1)
    monkeypatch.setattr(K, "CONV3X3_MIN_FWD_TILES", 0)
    monkeypatch.setattr(K, "CONV3X3_DIL_ANY", True)
    monkeypatch.setattr(K, "CLS1X1_WIDE", True)
    monkeypatch.setattr(K, "_GROUP_SCHED", {})
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _dev(device, *ts):
    return [None if t is None else t.detach().clone().to(device).contiguous() for t in ts]          # (never the shared CPU operands themselves)


class Family(object):
    """geo(case) -> Geo; directions; run(K, direction, a, b, case, bias, addend, opts) -> tensor; eligible(K, direction, a, b, case)."""
    split = True              # uses the split arithmetic: the impulse kinds apply
    directions = ("fwd", "bwd", "wrw")

    def geo(self, case):
        return Geo(3, 1, 1)

    def case5(self, case):
        return tuple(case[:5])


class SB3(Family):
    name = "conv3x3_sb"

    def eligible(self, K, direction, a, b, case):
        if direction == "wrw":
            return K.conv3x3_sb_wrw_eligible(a, b)
        x = a if direction == "fwd" else torch.zeros(1, case[1], 1, 1, device=a.device)
        return K.conv3x3_sb_eligible(x, b)

    def run(self, K, direction, a, b, case, bias=None, addend=None, opts=None):
        opts = opts or {}
        if direction == "wrw":
            return K.conv3x3_sb_wrw(a, b)
        return K.conv3x3_sb_run(a, b, direction == "bwd", bias, opts.get("nt", 0), addend=addend, want_stats=opts.get("stats", False))


class Dil(Family):
    name = "conv3x3_dil"
    directions = ("fwd", "bwd")

    def geo(self, case):
        return Geo(3, 1, case[5])

    def eligible(self, K, direction, a, b, case):
        x = a if direction == "fwd" else torch.zeros(1, case[1], 1, 1, device=a.device)
        return K.conv3x3_dil_eligible(x, b, (case[5], case[5]))

    def run(self, K, direction, a, b, case, bias=None, addend=None, opts=None):
        return K.conv3x3_dil_run(a, b, case[5], direction == "bwd", bias, addend=addend, want_stats=(opts or {}).get("stats", False))


class DilAny(Family):
    name = "conv3x3_dilany"

    def geo(self, case):
        return Geo(3, 1, case[5])

    def eligible(self, K, direction, a, b, case):
        if direction == "wrw":
            return K.conv3x3_dilany_wrw_eligible(a, b)
        x = a if direction == "fwd" else torch.zeros(1, case[1], 1, 1, device=a.device)
        return K.conv3x3_dilany_eligible(x, b, (case[5], case[5]))

    def run(self, K, direction, a, b, case, bias=None, addend=None, opts=None):
        if direction == "wrw":
            return K.conv3x3_dilany_wrw(a, b, case[5])
        return K.conv3x3_dilany_run(a, b, case[5], direction == "bwd", bias, addend=addend, want_stats=(opts or {}).get("stats", False))


class S2(Family):
    name = "conv3x3_s2"

    def geo(self, case):
        return Geo(3, 2, 1)

    def eligible(self, K, direction, a, b, case):
        B, ci, co, Ho, Wo = case[:5]
        x = torch.zeros(1, ci, 2 * Ho, 2 * Wo, device=a.device)
        w = torch.zeros(co, ci, 3, 3, device=a.device)
        return {"fwd": K.conv3x3_s2_fwd_eligible, "bwd": K.conv3x3_s2_bwd_eligible, "wrw": K.conv3x3_s2_wrw_eligible}[direction](x, w)

    def run(self, K, direction, a, b, case, bias=None, addend=None, opts=None):
        if direction == "fwd":
            return K.conv3x3_s2_run(a, b, want_stats=(opts or {}).get("stats", False))
        return K.conv3x3_s2_bwd_run(a, b) if direction == "bwd" else K.conv3x3_s2_wrw(a, b)


class One(Family):
    name = "conv1x1_sb"

    def geo(self, case):
        return Geo(1, 1, 1)

    def eligible(self, K, direction, a, b, case):
        if direction == "wrw":
            return K.conv1x1_sb_wrw_eligible(a, b)
        x = a if direction == "fwd" else torch.zeros(1, case[1], 1, 1, device=a.device)
        return K.conv1x1_sb_eligible(x, b)

    def run(self, K, direction, a, b, case, bias=None, addend=None, opts=None):
        if direction == "wrw":
            return K.conv1x1_sb_wrw(a, b)
        return K.conv1x1_sb_run(a, b, direction == "bwd", bias, want_stats=(opts or {}).get("stats", False), addend=addend)


FAMILIES = {f.name: f for f in (SB3(), Dil(), DilAny(), S2(), One())}
NT_SB8 = 0x109

# (family, case, arith, opts, env, directions); case = (B, Cin, Cout, H, W[, d]) -- for the stride-2 family H, W are the OUTPUT map.
# `emu`: also replayed on the emulated device (the GPU file runs all).
CONFIGS = []


def _add(fam, case, arith=F16X3, opts=None, env=None, directions=None, emu=False):
    CONFIGS.append(dict(fam=fam, case=tuple(case), arith=arith, opts=opts or {}, env=env or {},
                        directions=tuple(directions or FAMILIES[fam].directions), emu=emu))


SB3_CASES = [(1, 48, 48, 5, 8), (2, 48, 48, 9, 65), (1, 192, 48, 7, 36), (1, 64, 64, 7, 65), (1, 144, 144, 4, 64)]
for _arith in (F16X3, BF16X6):
    for _i, _case in enumerate(SB3_CASES):
        if _arith == BF16X6 and _case[1] % 48:
            continue                                             # 64 channels: the 16-channel-chunk kernels are f16x3 only
        for _glds in ("1", "0"):
            _add("conv3x3_sb", _case, _arith, env={"CSEG_CONV3X3_SB_GLDS": _glds}, directions=("fwd", "bwd"),
                 emu=(_glds == "1" and _i in (0, 1, 3)) or (_glds == "0" and _i == 0))
    for _nt in (3, 6):                                           # explicit channel tiling
        _add("conv3x3_sb", (1, 48, 96, 5, 40), _arith, opts={"nt": _nt}, directions=("fwd",), emu=(_arith == F16X3))
        _add("conv3x3_sb", (1, 96, 96, 5, 40), _arith, opts={"nt": _nt}, directions=("bwd",))
    for _case, _versions in (((2, 16, 48, 9, 128), ("1", "2")), ((2, 96, 48, 3, 17), ("2",)), ((1, 64, 96, 9, 33), ("2",))):
        if _arith == BF16X6 and _case[4] % 32:
            continue                                             # ragged widths: f16x3 only (conv3x3_sb_wrw_eligible)
        for _v in _versions:                                     # version 1: no ragged loaders
            _add("conv3x3_sb", _case, _arith, env={"CSEG_CONV3X3_SB_WRW_V": _v}, directions=("wrw",), emu=(_v == "2" or _arith == F16X3))
_add("conv3x3_sb", (1, 48, 144, 9, 68), opts={"nt": NT_SB8}, directions=("fwd",), emu=True)
_add("conv3x3_sb", (1, 144, 144, 5, 36), opts={"nt": NT_SB8}, directions=("bwd",))
_add("conv3x3_dil", (1, 64, 64, 7, 65, 2), emu=True)
_add("conv3x3_dil", (2, 128, 64, 5, 36, 4))
_add("conv3x3_dilany", (1, 64, 64, 5, 16, 1), emu=True)
_add("conv3x3_dilany", (1, 64, 48, 6, 17, 3), emu=True)
_add("conv3x3_dilany", (1, 48, 64, 14, 36, 12))
_add("conv3x3_dilany", (1, 64, 128, 9, 10, 36), emu=True)      # a rate larger than the map: the centre-tap 1x1
_add("conv3x3_s2", (1, 48, 48, 5, 32), emu=True)               # odd x even output map, every direction
_add("conv3x3_s2", (2, 96, 48, 3, 66), directions=("fwd", "bwd"))
_add("conv3x3_s2", (1, 64, 64, 6, 33), directions=("fwd",))    # odd output width
_add("conv3x3_s2", (1, 64, 128, 6, 32), directions=("fwd", "bwd", "wrw"))
for _arith in (F16X3, BF16X6):
    _add("conv1x1_sb", (2, 48, 64, 8, 8), _arith, emu=True)
    _add("conv1x1_sb", (1, 48, 144, 13, 43), _arith, directions=("fwd", "bwd"))
    _add("conv1x1_sb", (1, 144, 160, 8, 12), _arith, directions=("wrw",), emu=(_arith == F16X3))


def config_id(c):
    parts = [c["fam"], "x".join(str(v) for v in c["case"]), c["arith"], "+".join(c["directions"])]
    parts += ["%s%s" % (k, v) for k, v in sorted(c["opts"].items())] + ["%s%s" % (k.replace("CSEG_CONV3X3_SB_", ""), v) for k, v in sorted(c["env"].items())]
    return "-".join(parts)


def run_config(K, device, c, kinds):
    """One configuration: every direction it offers x every kind, compared with torch.equal against float64."""
    fam = FAMILIES[c["fam"]]
    geo, case = fam.geo(c["case"]), fam.case5(c["case"])
    for direction in c["directions"]:
        for kind in kinds:
            a, b, ref, _, _ = operands(geo, direction, kind, case)
            ad, bd = _dev(device, a, b)
            assert fam.eligible(K, direction, ad, bd, c["case"]), (c, direction)
            out = fam.run(K, direction, ad, bd, c["case"], opts=c["opts"])
            check(out, ref, "%s %s %s" % (config_id(c), direction, kind))


# ---- epilogue variants (dense integers and the degenerate operands only: bias / addend / statistics) ----------------------------------
EPILOGUE_CONFIGS = [          # (family, case, arith, bias, addend, stats)
    ("conv3x3_sb", (2, 48, 48, 9, 65), F16X3, True, False, False), ("conv3x3_sb", (2, 48, 48, 9, 65), F16X3, True, True, False),
    ("conv3x3_sb", (2, 48, 48, 9, 65), F16X3, True, False, True), ("conv3x3_sb", (1, 48, 48, 5, 8), BF16X6, True, True, False),
    ("conv3x3_sb", (1, 48, 48, 5, 8), BF16X6, False, False, True), ("conv3x3_sb", (1, 64, 64, 7, 65), F16X3, True, True, False),
    ("conv3x3_dil", (1, 64, 64, 7, 65, 2), F16X3, True, True, False), ("conv3x3_dilany", (1, 64, 48, 6, 17, 3), F16X3, True, True, False),
    ("conv3x3_dilany", (1, 64, 48, 6, 17, 3), F16X3, True, False, True), ("conv3x3_s2", (1, 48, 48, 5, 32), F16X3, False, False, True),
    ("conv1x1_sb", (2, 48, 64, 8, 8), F16X3, True, True, False), ("conv1x1_sb", (2, 48, 64, 8, 8), BF16X6, True, False, True),
]
EPILOGUE_EMU = (0, 1, 2, 3, 7, 10)


def run_epilogue(K, device, cfg, kinds=("dense", "zero_a", "zero_b", "const")):
    name, case, arith, with_bias, with_addend, stats = cfg
    fam = FAMILIES[name]
    geo = fam.geo(case)
    for kind in kinds:
        a, b, ref, bias, addend = operands(geo, "fwd", kind, fam.case5(case), with_bias, with_addend)
        ad, bd, biasd, addd = _dev(device, a, b, bias, addend)
        assert fam.eligible(K, "fwd", ad, bd, case), cfg
        out = fam.run(K, "fwd", ad, bd, case, bias=biasd, addend=addd, opts={"stats": stats})
        if stats:
            assert K.known_tile_stats(out) is not None, "the statistics epilogue did not run"
        check(out, ref, "%s %s fwd %s bias=%s addend=%s stats=%s" % (name, case, kind, with_bias, with_addend, stats))


# ---- degenerate operands, one small shape per family, every direction ---------------------------------------------------------------
DEGENERATE_CONFIGS = [        # (family, case, arith, directions or None = all)
    ("conv3x3_sb", (1, 48, 48, 5, 8), F16X3, None), ("conv3x3_sb", (1, 48, 48, 5, 8), BF16X6, ("fwd", "bwd")),
    ("conv3x3_sb", (1, 64, 64, 7, 65), F16X3, None), ("conv3x3_dil", (1, 64, 64, 7, 65, 2), F16X3, None),
    ("conv3x3_dilany", (1, 64, 48, 6, 17, 3), F16X3, None), ("conv3x3_s2", (1, 48, 48, 5, 32), F16X3, None),
    ("conv1x1_sb", (2, 48, 64, 8, 8), F16X3, None), ("conv1x1_sb", (2, 48, 64, 8, 8), BF16X6, None),
    ("conv3x3_sb", (2, 16, 48, 9, 128), BF16X6, ("wrw",)),          # bf16x6 weight gradient: widths % 32 only
]
DEGENERATE_EMU = (0, 1, 4, 5, 6, 8)


def run_degenerate(K, device, cfg):
    """all-zero x / w / dy and constant operands: dx, dw, y exactly zero (or the exact tap counts), and finite"""
    name, case, arith, directions = cfg
    fam = FAMILIES[name]
    geo = fam.geo(case)
    for direction in directions or fam.directions:
        for kind in DEGENERATE_KINDS:
            a, b, ref, _, _ = operands(geo, direction, kind, fam.case5(case))
            ad, bd = _dev(device, a, b)
            assert fam.eligible(K, direction, ad, bd, case), (cfg, direction)
            out = fam.run(K, direction, ad, bd, case)
            check(out, ref, "%s %s %s %s" % (name, case, direction, kind))
        if direction != "fwd":                        # both operands zero (a zero-initialised layer behind a dead channel)
            a, b, ref, _, _ = operands(geo, direction, "zero_a", fam.case5(case))
            ad, bd = _dev(device, a, torch.zeros_like(b))
            check(fam.run(K, direction, ad, bd, case), torch.zeros_like(ref), "%s %s %s zero x zero" % (name, case, direction))


def run_autograd_zero_input(K, device):
    """All-zero x through the autograd nodes conv3x3_split_bf16 / conv1x1_split_bf16, forward and backward: the activation's max|.|
    goes through amax_of / known_amax with an EMPTY record (all words zero); then an all-zero dy (the contrast warm-up:
    loss + 0 * loss_contrast)."""
    for fn, k, case in ((K.conv3x3_split_bf16, 3, (2, 48, 48, 9, 65)), (K.conv1x1_split_bf16, 1, (2, 48, 64, 8, 8))):
        geo = Geo(k, 1, 1)
        _, w, _, _, _ = operands(geo, "fwd", "dense", case)
        _, dy, _, _, _ = operands(geo, "wrw", "dense", case)
        B, ci, co, H, W = case
        bias = torch.arange(co, dtype=torch.float32) - 3
        for x_zero, dy_zero in ((True, False), (False, True)):
            x = torch.zeros(B, ci, H, W) if x_zero else operands(geo, "fwd", "dense", case)[0]
            g = torch.zeros_like(dy) if dy_zero else dy
            xd, wd, bd, gd = _dev(device, x, w, bias, g)
            xd.requires_grad_(True), wd.requires_grad_(True), bd.requires_grad_(True)
            y = fn(xd, wd, bd)
            y.backward(gd)
            x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
            y64 = F.conv2d(x64, w64, b64, 1, k // 2)
            y64.backward(g.double())
            what = "%s zero %s" % (fn.__name__, "x" if x_zero else "dy")
            check(y, y64.detach(), what + " y")
            check(xd.grad, x64.grad, what + " dx")
            check(wd.grad, w64.grad, what + " dw")
            check(bd.grad, b64.grad, what + " db")
            if x_zero:
                assert torch.equal(y.detach().cpu(), bias.view(1, -1, 1, 1).expand_as(y)) and not bool(wd.grad.any())
            else:
                assert not bool(xd.grad.any()) and not bool(wd.grad.any()) and not bool(bd.grad.any())


# ---- grouped launches (csrc/conv3x3_group.hip) -----------------------------------------------------------------------------------------
GROUPS = [[(1, 48, 48, 9, 70), (1, 96, 96, 5, 36)], [(2, 48, 48, 4, 64), (2, 96, 96, 6, 33), (1, 192, 48, 3, 20)]]


def run_group(K, device, shapes, kinds):
    geo = Geo(3, 1, 1)
    for kind in kinds:
        for direction in ("fwd", "bwd"):
            items, refs = [], []
            for i, case in enumerate(shapes):
                with_addend = kind in ("dense", "zero_a", "zero_b") and i == 0
                a, b, ref, _, addend = operands(geo, direction, kind, case, False, with_addend)
                ad, bd, addd = _dev(device, a, b, addend)
                assert K.conv3x3_sb_eligible(ad if direction == "fwd" else torch.zeros(1, case[1], 1, 1, device=device), bd)
                items.append((ad, bd, direction == "bwd", K.tensor_amax(ad), addd))
                refs.append(ref)
            ys, _ = K.conv3x3_group_run(items, want_stats=(direction == "fwd"))
            for i, (y, ref) in enumerate(zip(ys, refs)):
                check(y, ref, "group %s member %d %s %s" % (shapes, i, direction, kind))
        items, refs = [], []
        for case in shapes:
            a, b, ref, _, _ = operands(geo, "wrw", kind, case)
            ad, bd = _dev(device, a, b)
            assert K.conv3x3_sb_wrw_eligible(ad, bd)
            items.append((ad, bd, K.tensor_amax(ad), K.tensor_amax(bd)))
            refs.append(ref)
        for i, (dw, ref) in enumerate(zip(K.conv3x3_group_wrw(items), refs)):
            check(dw, ref, "group %s member %d wrw %s" % (shapes, i, kind))


# ---- fp32 paths (no split: the dense-integer case and the degenerate operands) ------------------------------------------------------------
FP32_KINDS = ("dense", "pow2", "zero_a", "zero_b", "const")


def run_conv3x3_fp32(K, device, case, kinds=FP32_KINDS):
    """kernels.conv3x3 (csrc/conv3x3.hip) through its autograd node: forward, backward-data, weight gradient on the fp32-MFMA kernels"""
    from contrastiveseg_amd import _hip
    geo = Geo(3, 1, 1)
    B, ci, co, H, W = case
    for kind in kinds:
        x, w, y_ref, _, _ = operands(geo, "fwd", kind, case)
        dy, _, dx_ref, _, _ = operands(geo, "bwd", "dense", case)
        dx_ref = geo.ref("bwd", dy, w, case)
        dw_ref = geo.ref("wrw", x, dy, case)
        for r in (dx_ref, dw_ref):
            assert torch.equal(r.float().double(), r)
        xd, wd, dyd = _dev(device, x, w, dy)
        assert K.conv3x3_eligible(xd, wd)
        xd.requires_grad_(True), wd.requires_grad_(True)
        calls, orig = [], _hip.call
        _hip.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        try:
            y = K.conv3x3(xd, wd)
            y.backward(dyd)
        finally:
            _hip.call = orig
        want_calls = 2 + (1 if (co == ci and co in K.CONV3X3_WRW_CHANNELS) else 0)
        assert sum(c in ("cseg_conv3x3_fwd", "cseg_conv3x3_wrw") for c in calls) == want_calls, calls
        check(y, y_ref, "conv3x3 %s y %s" % (case, kind))
        check(xd.grad, dx_ref, "conv3x3 %s dx %s" % (case, kind))
        check(wd.grad, dw_ref, "conv3x3 %s dw %s" % (case, kind))


def run_rgb_stem(K, device, case, kinds=FP32_KINDS):
    B, H, W = case
    geo, c5 = Geo(3, 2, 1), (B, 3, 64, H // 2, W // 2)
    for kind in kinds:
        x, w, y_ref, _, _ = operands(geo, "fwd", kind, c5)
        dy = operands(geo, "bwd", "dense", c5)[0]
        dw_ref = geo.ref("wrw", x, dy, c5)
        assert torch.equal(dw_ref.float().double(), dw_ref) and B * H * W * 49 < 2 ** 24
        xd, wd, dyd = _dev(device, x, w, dy)
        assert K.conv3x3_s2_rgb_eligible(xd, wd)
        wd.requires_grad_(True)
        y = K.conv3x3_s2_rgb(xd, wd)
        y.backward(dyd)
        check(y, y_ref, "rgb stem %s y %s" % (case, kind))
        check(wd.grad, dw_ref, "rgb stem %s dw %s" % (case, kind))


CLS_CASES = [(2, 96, 19, 6, 20, False), (3, 64, 7, 5, 13, True)]               # B, C, K, H, W, bias
CLS_WIDE_CASES = [(2, 40, 33, 8, 32, True), (1, 96, 171, 6, 24, False), (2, 50, 60, 7, 9, True)]


def run_classifier(K, device, case, wide, kinds=FP32_KINDS):
    """cls1x1 / cls1x1_wide with mask=None: forward, backward-data, weight and bias gradient through the autograd nodes"""
    B, C, Kc, H, W, has_bias = case
    geo, c5 = Geo(1, 1, 1), (B, C, Kc, H, W)
    for kind in kinds:
        x, w, y_ref, bias, _ = operands(geo, "fwd", kind, c5, has_bias, False)
        dy = operands(geo, "bwd", "dense", c5)[0]
        dx_ref, dw_ref = geo.ref("bwd", dy, w, c5), geo.ref("wrw", x, dy, c5)
        for r in (dx_ref, dw_ref):
            assert torch.equal(r.float().double(), r)
        xd, wd, bd, dyd = _dev(device, x, w, bias, dy)
        assert (K.cls1x1_wide_eligible if wide else K.cls1x1_eligible)(xd, wd)
        xd.requires_grad_(True), wd.requires_grad_(True)
        if bd is not None:
            bd.requires_grad_(True)
        y = (K.cls1x1_wide if wide else K.cls1x1)(xd, wd, bd, None)
        y.backward(dyd)
        what = "%s %s %s " % ("cls1x1_wide" if wide else "cls1x1", case, kind)
        check(y, y_ref, what + "y")
        check(xd.grad, dx_ref, what + "dx")
        check(wd.grad, dw_ref, what + "dw")
        if bd is not None:
            check(bd.grad, dy.double().sum((0, 2, 3)), what + "db")
