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


# Operands are shared through this cache (the callers never modify them). Bounded: the lattice tables below hold a few thousand
# (shape, direction, kind) triples; the variants of one lattice chunk (arithmetic, tiling, environment) are adjacent in LATTICES and
# one chunk is at most 60 triples (LATTICE_EVALS), so a variant finds the operands of the one before it.
OPERAND_CACHE = 512


def _check_wide_rule(t):
    nz = t[t != 0].abs()
    assert float(nz.min()) * 2.0 ** 10 >= float(nz.max()), "generator rule: non-zero elements within 2^10 of the tensor's maximum"


@functools.lru_cache(maxsize=OPERAND_CACHE)
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


# ---- shape lattices ------------------------------------------------------------------------------------------------------------------------
# CONFIGS pins hand-picked shapes; the routing predicates admit ANY batch, height and width once the channels fit. The lattices below
# take their heights and widths from the tile geometry written in the kernels -- 4-row tiles (8 for NT_SB8), 64-pixel column segments
# (32 for version 2 of the weight gradient and the stride-2 weight gradient), rows that are / are not 16-byte aligned (W % 4 in
# {0, 1, 2, 3}) -- down to maps of one pixel: buffer-load bounds on maps smaller than a tile, the element-wise row store, weight /
# fragment staging when a block's tile is mostly padding, split-K reductions with fewer pixels than splits.
LAT_H = (1, 2, 3, 4, 5, 8, 9)
LAT_W = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129)
LAT_W32 = tuple(w for w in LAT_W if w % 32 == 0)
LAT_W64 = tuple(w for w in LAT_W if w % 64 == 0)
S2_BWD_W = (2, 4, 16, 32, 34, 64, 66)                  # stride 2, backward-data: even output widths
S2_WRW_W = (32, 64, 96)                                # stride 2, weight gradient: output widths % 32
DIL_H, DIL_W, DIL_D = (1, 2, 4, 6, 13), (1, 3, 16, 17, 33), (1, 2, 3, 5, 12, 36)     # rates below, equal to and above the map
LATTICE_EVALS = 60                                     # (shape, direction, kind) evaluations per table entry, at most
LATTICE_KINDS = ("dense", "const")                     # at every point; pow2 at the corners; the impulse kinds where they have room

# family, (B, Cin, Cout), arith, opts, env, directions, heights, widths, dilations (None: the family has none), emu
LATTICES = []


def impulse_room(geo, direction, shape):
    """Whether _sites() can place the impulses of wide_a / wide_b on the SPARSE operand `shape` (B, C, H, W): it needs six sites, each
    candidate position serves one site, and within an image two sites must not meet in one output element. The rule, from the shape
    alone: at least 12 positions, and (forward / backward-data of a k > 1 operator) at least 12 cells of a grid whose pitch is beyond
    the operator's reach, counted over the batch -- cells of such a grid never interact (the weight gradient and the 1x1 operator
    have no such constraint: one site per channel / any distinct positions). Conservative: _operands() still asserts the six."""
    B, C, H, W = shape
    if H * W < 12 or C < 6:
        return False
    if direction == "wrw" or geo.k == 1:
        return True
    if geo.stride == 2:
        pitch = 3
    elif geo.dil >= max(H, W):
        pitch = 1                                      # no two different positions are a multiple of the rate apart
    else:
        pitch = 2 * geo.dil + 1
    return B * ((H + pitch - 1) // pitch) * ((W + pitch - 1) // pitch) >= 12


def lattice_points(c):
    """[(case, direction, kind)] of one table entry, in running order."""
    fam = FAMILIES[c["fam"]]
    B, ci, co = c["pair"]
    hs, ws = c["heights"], c["widths"]
    out = []
    for d in c["dilations"] or (None,):
        for H in hs:
            for W in ws:
                case = (B, ci, co, H, W) + (() if d is None else (d,))
                geo = fam.geo(case)
                corner = H in (hs[0], hs[-1]) and W in (ws[0], ws[-1])
                for direction in c["directions"]:
                    kinds = list(LATTICE_KINDS) + (["pow2"] if corner else [])
                    if fam.split and impulse_room(geo, direction, geo.operand_shapes(direction, fam.case5(case))[0]):
                        kinds += ["wide_a", "wide_b"]
                    out += [(case, direction, k) for k in kinds]
    return out


def _lat(fam, pair, arith=F16X3, opts=None, env=None, directions=None, heights=LAT_H, widths=LAT_W, dilations=None, emu=()):
    """One lattice = heights x widths (x dilations) of a channel pair under one variant, cut along the widths (and dilations) into
    table entries of at most LATTICE_EVALS evaluations. emu: indices of the entries that the emulated device replays too, or
    {index: n} to replay every n-th evaluation of that entry (wide layers cost the emulator seconds per evaluation; the MI355X file
    runs every evaluation of every entry). An entry's `emu` is that n, 0 for the entries the emulated device leaves out."""
    emu = emu if isinstance(emu, dict) else {i: 1 for i in emu}
    base = dict(fam=fam, pair=tuple(pair), arith=arith, opts=opts or {}, env=env or {}, heights=tuple(heights),
                directions=tuple(directions or FAMILIES[fam].directions))
    n = 0
    for d in dilations or (None,):
        chunk = []
        for w in tuple(widths) + (None,):
            trial = dict(base, widths=tuple(chunk + [w]), dilations=None if d is None else (d,))
            if w is None or (chunk and len(lattice_points(trial)) > LATTICE_EVALS):
                entry = dict(base, widths=tuple(chunk), dilations=None if d is None else (d,), emu=emu.get(n, 0))
                assert chunk and len(lattice_points(entry)) <= LATTICE_EVALS, (entry, len(lattice_points(entry)))
                LATTICES.append(entry)
                n += 1
                chunk = []
            chunk.append(w)


def _lat_variants(fam, pair, variants, **kw):
    """The variants of one lattice entry by entry, so that the operands of a chunk are still cached when its next variant runs."""
    first = len(LATTICES)
    for v in variants:
        _lat(fam, pair, **dict(kw, **v))
    block = LATTICES[first:]
    per = len(block) // len(variants)
    # (variants differ in arithmetic, tiling and environment only, so they cut alike; OPERAND_CACHE relies on the interleaving)
    assert per * len(variants) == len(block) and all(block[v * per + i]["widths"] == block[i]["widths"] for v in range(len(variants)) for i in range(per))
    LATTICES[first:] = [block[v * per + i] for i in range(per) for v in range(len(variants))]


_GLDS = [{"env": {"CSEG_CONV3X3_SB_GLDS": g}} for g in ("1", "0")]
_FB = ("fwd", "bwd")
# conv3x3_sb forward / backward-data: every tile form a routing rule selects -- 48 / 192 / 384 output channels on the 16-channel-chunk
# kernel, 64 / 128 on its four-tile form, 96 / 144 on the 32-channel-chunk kernel (6 / 9 tiles), the 8-row kernel, explicit tilings.
# CSEG_CONV3X3_SB_GLDS is read by the bf16x6 form of the 32-channel-chunk kernel only (96 / 144 output channels, either direction):
# both values there, the variable left alone everywhere else (the f16x3 kernels and the 16-channel-chunk kernel never look at it).
for _pair in ((1, 48, 48), (1, 64, 64), (2, 48, 96), (1, 96, 48), (1, 64, 128), (3, 192, 48), (1, 144, 144)):
    _vs = [{"emu": {0: 2, 5: 1} if _pair == (1, 48, 48) else {2: 3} if _pair == (1, 64, 64) else ()}]
    if _pair[1] % 48 == 0 and _pair[2] % 48 == 0:
        if 96 in _pair[1:] or 144 in _pair[1:]:
            _vs += [dict(v, arith=BF16X6, emu=(4,) if (_pair == (2, 48, 96) and v is _GLDS[0]) else ()) for v in _GLDS]
        else:
            _vs += [{"arith": BF16X6}]
    _lat_variants("conv3x3_sb", _pair, _vs, directions=_FB)
_lat_variants("conv3x3_sb", (1, 144, 144), [{"opts": {"nt": NT_SB8}, "emu": {6: 16}}], directions=_FB)       # (nt = 0: the loop above)
for _c, _hs, _ws in ((192, (1, 5, 9), (3, 65, 128)), (384, (2, 4), (1, 33, 66))):
    _lat_variants("conv3x3_sb", (1, _c, _c), [{"opts": {"nt": nt}, "emu": {0: 11} if (_c, nt) == (192, "pick") else ()}
                                             for nt in ("pick", 3, 6, 9)], directions=_FB, heights=_hs, widths=_ws)
# conv3x3_sb weight gradient. f16x3 always runs version 2, whatever CSEG_CONV3X3_SB_WRW_V says: every width, the variable left alone.
# bf16x6 runs the version the variable selects: version 2 at widths % 32, version 1 at widths % 64 (output channels % 48 both).
for _pair in ((1, 48, 48), (1, 64, 64), (2, 16, 48), (3, 96, 48), (1, 64, 96)):
    _lat_variants("conv3x3_sb", _pair, [{"emu": (0,) if _pair == (1, 48, 48) else {3: 2} if _pair == (1, 64, 96) else ()}], directions=("wrw",))
    if _pair[2] % 48 == 0:
        _lat_variants("conv3x3_sb", _pair, [{"env": {"CSEG_CONV3X3_SB_WRW_V": "2"}, "arith": BF16X6, "emu": (0,) if _pair == (2, 16, 48) else ()}],
                      directions=("wrw",), widths=LAT_W32)
        _lat_variants("conv3x3_sb", _pair, [{"env": {"CSEG_CONV3X3_SB_WRW_V": "1"}, "arith": BF16X6, "emu": {0: 2} if _pair == (3, 96, 48) else ()}],
                      directions=("wrw",), widths=LAT_W64)
# conv1x1_sb, both arithmetics
for _pair, _dirs in (((1, 48, 64), None), ((2, 64, 48), None), ((3, 48, 144), None), ((1, 256, 48), None), ((1, 144, 160), ("wrw",))):
    for _d in ((_FB, ("wrw",)) if _dirs is None else (_dirs,)):
        _lat_variants("conv1x1_sb", _pair, [{"arith": F16X3, "emu": (0,) if _pair == (1, 48, 64) else ()},
                                            {"arith": BF16X6, "emu": (1,) if _pair == (2, 64, 48) else ()}], directions=_d)
# conv3x3_s2: H, W are the OUTPUT map (the input is twice that: even by contract); the kernels tile it 4 rows x 64 columns like the
# stride-1 ones, so the same heights in every direction and the same widths forward; backward-data and the weight gradient on the
# widths they take
for _pair, _dirs in (((1, 48, 48), ("fwd", "bwd", "wrw")), ((2, 96, 48), ("fwd", "bwd", "wrw")), ((3, 64, 64), ("fwd", "bwd", "wrw")),
                     ((1, 64, 128), ("fwd", "bwd", "wrw")), ((1, 48, 96), ("fwd",))):
    for _d in _dirs:
        _lat("conv3x3_s2", _pair, directions=(_d,), heights=LAT_H, widths={"fwd": LAT_W, "bwd": S2_BWD_W, "wrw": S2_WRW_W}[_d],
             emu={0: 2} if _pair == (1, 48, 48) else ())
# conv3x3_dilany: all three directions, rates below / equal to / above the map (the last: the centre-tap path)
for _pair in ((1, 64, 48), (2, 48, 64), (3, 64, 128)):
    for _d in (_FB, ("wrw",)):
        _lat("conv3x3_dilany", _pair, directions=_d, heights=DIL_H, widths=DIL_W, dilations=DIL_D, emu={0: 1, 3: 2, 5: 2} if _pair == (1, 64, 48) else ())


def lattice_id(c):
    parts = [c["fam"], "x".join(str(v) for v in c["pair"]), c["arith"], "+".join(c["directions"]),
             "h" + ".".join(str(h) for h in c["heights"]), "w" + ".".join(str(w) for w in c["widths"])]
    parts += ["d" + ".".join(str(d) for d in c["dilations"])] if c["dilations"] else []
    parts += ["%s%s" % (k, v) for k, v in sorted(c["opts"].items())] + ["%s%s" % (k.replace("CSEG_CONV3X3_SB_", ""), v) for k, v in sorted(c["env"].items())]
    return "-".join(parts)


def run_lattice(K, device, c, every=1):
    """One lattice entry: every point x every direction it offers x the kinds of lattice_points, torch.equal against float64. A point
    that its family's predicate rejects is an error of the table, not a skip. every: see _lat (the emulated device). -> the number of
    evaluations."""
    fam = FAMILIES[c["fam"]]
    n = 0
    for case, direction, kind in lattice_points(c)[::every]:
        geo = fam.geo(case)
        a, b, ref, _, _ = operands(geo, direction, kind, fam.case5(case))
        ad, bd = _dev(device, a, b)
        assert fam.eligible(K, direction, ad, bd, case), (lattice_id(c), case, direction)
        opts = dict(c["opts"])
        if opts.get("nt") == "pick":                   # the tiling the autograd nodes ask for at 192 / 384 channels
            opts["nt"] = K.conv3x3_sb_pick_nt(ad, ref.shape[1])
        out = fam.run(K, direction, ad, bd, case, opts=opts)
        check(out, ref, "%s %s %s %s" % (lattice_id(c), case, direction, kind))
        n += 1
    return n


# grouped launches: members of DIFFERENT lattice shapes (one row, one column, one pixel, just past a 64-pixel segment, unaligned rows)
LATTICE_GROUPS = [[(1, 48, 48, 1, 65), (2, 96, 96, 3, 1)],
                  [(3, 48, 48, 2, 33), (1, 96, 96, 1, 5), (1, 192, 192, 5, 2)],
                  [(1, 48, 96, 4, 129), (2, 96, 48, 9, 3), (1, 192, 48, 1, 1), (1, 384, 384, 2, 31)],
                  [(2, 384, 384, 1, 4), (1, 192, 192, 3, 65), (1, 48, 48, 8, 1)],
                  # every width a multiple of its row segment (64, and 32 for 96 = 32 mod 64): the grouped weight-gradient kernel and
                  # its grouped reduction -- one ragged member sends the whole group to one launch per member
                  [(1, 48, 48, 1, 32), (2, 96, 96, 3, 64), (1, 192, 192, 5, 128), (3, 48, 96, 2, 96)]]
LATTICE_GROUP_IDS = ["2-members", "3-members", "4-members", "3-members-b", "4-members-aligned"]
LATTICE_GROUP_KINDS = ("dense", "const", "pow2", "zero_a")          # (dense / zero_a: member 0 with an addend, run_group)

# fp32 families at lattice corners (kernels.conv3x3 takes widths % 4 only: its narrowest map is four pixels wide)
FP32_CONV3X3_CORNERS = [(1, 48, 48, 1, 4), (3, 96, 96, 2, 8), (1, 48, 48, 2, 68)]
RGB_STEM_CORNERS = [(1, 2, 2), (3, 4, 6), (1, 2, 130)]                           # B, H, W of the IMAGE: outputs 1x1, 2x3, 1x65
CLS_CORNERS = [(1, 96, 19, 1, 1, True), (3, 64, 7, 2, 3, False), (2, 96, 19, 1, 65, True)]
CLS_WIDE_CORNERS = [(1, 40, 33, 1, 2, True), (3, 96, 171, 2, 3, False), (1, 50, 60, 1, 65, True)]


# ---- refusals: what the documented contract rejects, the predicate rejects, and so does the entry point ------------------------------------
# One helper per predicate and per entry point, so that each argument list stands in ONE place (the calls are those of
# contrastiveseg_amd/kernels.py). A helper takes (K, where, B, Cin, Cout, H, W, **extra): `where` is the device for a predicate -- it
# gets zero tensors of the rejected shape -- and, for an entry point, a scratch pointer that stands in every pointer argument: every
# rule listed in REFUSALS is a CSEG_REQUIRE (or a zero workspace size, or the wrapper's own check) ahead of the first
# hipLaunchKernelGGL of its entry point, so a refusal launches nothing. For the stride-2 family H, W are the OUTPUT map; hin / win
# give an input map that is not twice that.
def _z(dev, *shape):
    return torch.zeros(*shape, device=dev)


def _s2_tensors(dev, B, ci, co, H, W, hin=None, win=None):
    return _z(dev, B, ci, 2 * H if hin is None else hin, 2 * W if win is None else win), _z(dev, co, ci, 3, 3)


def _blocks_ok(K, dev, channels):
    from contrastiveseg_amd.lib.models.backbones.hrnet_backbone import BasicBlock
    from contrastiveseg_amd.lib.models.tools.module_helper import mark_conv_bn_pairs
    blocks = [mark_conv_bn_pairs(BasicBlock(c, c, bn_type="torchbn").train()).to(dev) for c in channels]
    return K.basic_block_group_ok(blocks, [_z(dev, 1, c, 3, 5).requires_grad_(True) for c in channels])


REFUSAL_PREDICATES = {
    "c3": lambda K, dev, B, ci, co, H, W, **kw: K.conv3x3_sb_eligible(_z(dev, B, ci, H, W), _z(dev, co, ci, 3, 3)),
    "c3_head": lambda K, dev, B, ci, co, H, W, **kw: K.conv3x3_sb_head_nt(co) != 0,              # (does any rule pick the 8-row kernel?)
    "c3_wrw": lambda K, dev, B, ci, co, H, W, **kw: K.conv3x3_sb_wrw_eligible(_z(dev, B, ci, H, W), _z(dev, B, co, H, W)),
    "c1": lambda K, dev, B, ci, co, H, W, **kw: K.conv1x1_sb_eligible(_z(dev, B, ci, H, W), _z(dev, co, ci, 1, 1)),
    "c1_wrw": lambda K, dev, B, ci, co, H, W, **kw: K.conv1x1_sb_wrw_eligible(_z(dev, B, ci, H, W), _z(dev, B, co, H, W)),
    "s2_fwd": lambda K, dev, *c, **kw: K.conv3x3_s2_fwd_eligible(*_s2_tensors(dev, *c, **kw)),
    "s2_bwd": lambda K, dev, *c, **kw: K.conv3x3_s2_bwd_eligible(*_s2_tensors(dev, *c, **kw)),
    "s2_wrw": lambda K, dev, *c, **kw: K.conv3x3_s2_wrw_eligible(*_s2_tensors(dev, *c, **kw)),
    "any": lambda K, dev, B, ci, co, H, W, d=1, d2=None, **kw: K.conv3x3_dilany_eligible(_z(dev, B, ci, H, W), _z(dev, co, ci, 3, 3), (d, d if d2 is None else d2)),
    "any_wrw": lambda K, dev, B, ci, co, H, W, **kw: K.conv3x3_dilany_wrw_eligible(_z(dev, B, ci, H, W), _z(dev, B, co, H, W)),
    "blocks": lambda K, dev, *c, channels=(), **kw: _blocks_ok(K, dev, channels),
}


def _group_members(K, struct, fields, p, members):
    arr = (struct * len(members))()
    for e, (B, ci, co, H, W) in zip(arr, members):
        for f in fields:
            setattr(e, f, p.value)
        e.B, e.Cin, e.Cout, e.H, e.W = B, ci, co, H, W
    return arr


def _e_group_fwd(K, p, *c, members=(), **kw):
    import ctypes
    arr = _group_members(K, K._hip.ConvGroupMember, ("x", "wp", "y", "amax_x", "amax_w"), p, members)
    K._hip.call("cseg_conv3x3_split_group_fwd", ctypes.byref(arr), len(members), K.split_arith_id(), p, K._hip.stream_ptr())


def _e_group_wrw(K, p, *c, members=(), **kw):
    import ctypes
    arr = _group_members(K, K._hip.WrwGroupMember, ("x", "dy", "amax_x", "amax_dy", "ws", "dw"), p, members)
    K._hip.call("cseg_conv3x3_split_group_wrw", ctypes.byref(arr), len(members), K.split_arith_id(), K._hip.stream_ptr())


REFUSAL_ENTRIES = {
    "c3_fwd": lambda K, p, B, ci, co, H, W, nt=0, **kw: K._hip.call(
        "cseg_conv3x3_split_fwd", p, p, None, B, ci, co, H, W, nt, K.split_arith_id(), p, p, p, K._hip.stream_ptr()),
    "c3_fwd_add": lambda K, p, B, ci, co, H, W, nt=0, **kw: K._hip.call(
        "cseg_conv3x3_split_fwd_add", p, p, None, p, B, ci, co, H, W, nt, K.split_arith_id(), p, p, p, K._hip.stream_ptr()),
    "c3_wrw": lambda K, p, B, ci, co, H, W, **kw: K._hip.call(
        "cseg_conv3x3_split_wrw", p, p, B, ci, co, H, W, K.split_arith_id(), p, p, p, p, K._hip.stream_ptr()),
    "c3_wrw_wrapper": lambda K, p, B, ci, co, H, W, **kw: K.conv3x3_sb_wrw(torch.zeros(B, ci, H, W), torch.zeros(B, co, H, W)),       # (no workspace size)
    "c1_fwd": lambda K, p, B, ci, co, H, W, **kw: K._hip.call(
        "cseg_conv1x1_split_fwd", p, p, None, B, ci, co, H * W, K.split_arith_id(), p, p, p, K._hip.stream_ptr()),
    "c1_wrw": lambda K, p, B, ci, co, H, W, **kw: K._hip.call(
        "cseg_conv1x1_split_wrw", p, p, B, ci, co, H * W, K.split_arith_id(), p, p, p, p, K._hip.stream_ptr()),
    "s2_fwd": lambda K, p, B, ci, co, H, W, nt=3, **kw: K._hip.call(
        "cseg_conv3x3_s2_split_fwd", p, p, B, ci, co, H, W, nt, p, p, p, K._hip.stream_ptr()),
    "s2_bwd": lambda K, p, B, ci, co, H, W, nt=3, **kw: K._hip.call(
        "cseg_conv3x3_s2_split_bwd", p, p, B, ci, co, H, W, nt, p, p, p, K._hip.stream_ptr()),
    "s2_wrw": lambda K, p, B, ci, co, H, W, **kw: K._hip.call(
        "cseg_conv3x3_s2_split_wrw", p, p, B, ci, co, H, W, K.ARITH_IDS[F16X3], p, p, p, p, K._hip.stream_ptr()),
    "s2_wrw_wrapper": lambda K, p, B, ci, co, H, W, hin=None, win=None, **kw: K.conv3x3_s2_wrw(torch.zeros(B, ci, hin, win), torch.zeros(B, co, H, W)),
    "any_fwd": lambda K, p, B, ci, co, H, W, d=1, **kw: K._hip.call(
        "cseg_conv3x3_split_dilany_fwd", p, p, None, None, B, ci, co, H, W, d, p, p, p, None, K._hip.stream_ptr()),
    "any_wrw": lambda K, p, B, ci, co, H, W, d=1, **kw: K._hip.call(
        "cseg_conv3x3_split_dilany_wrw", p, p, B, ci, co, H, W, d, p, p, p, p, K._hip.stream_ptr()),
    "any_wrapper": lambda K, p, B, ci, co, H, W, d=1, **kw: K.conv3x3_dilany_run(torch.zeros(B, ci, H, W), torch.zeros(co, ci, 3, 3), d),
    "group_fwd": _e_group_fwd,
    "group_wrw": _e_group_wrw,
}

# (predicate or None, entry or None, (B, Cin, Cout, H, W), arith, env, extra). None: that side has no such rule -- the predicate is
# the stricter one, or the rule is about an argument the predicate never sees (a tiling, an input map the entry point is not told).
REFUSALS = []
_REFUSAL_MAPS = ((1, 1, 1), (3, 5, 33), (1, 9, 65))                 # (B, H, W)


def _refuse(pred, entry, case, arith=F16X3, env=None, **extra):
    REFUSALS.append((pred, entry, tuple(case), arith, env or {}, extra))


for _ci, _co in ((40, 48), (24, 96), (48, 80), (96, 40), (64, 100), (48, 16)):                  # conv3x3_sb forward / backward-data
    for _B, _H, _W in _REFUSAL_MAPS:
        _refuse("c3", "c3_fwd", (_B, _ci, _co, _H, _W))
_refuse("c3", None, (1, 16, 48, 5, 33))                              # 16 input channels: backward-data could not tile them
_refuse(None, "c3_fwd", (1, 48, 96, 5, 33), nt=9)                    # nine tiles of 96 channels
_refuse(None, "c3_fwd", (1, 48, 96, 5, 33), nt=5)
_refuse("c3_head", "c3_fwd", (1, 48, 96, 9, 65), nt=NT_SB8)          # the 8-row kernel: output channels % 144,
_refuse("c3_head", "c3_fwd", (1, 144, 144, 9, 65), BF16X6, nt=NT_SB8)          # f16x3 only,
_refuse(None, "c3_fwd_add", (1, 144, 144, 9, 65), nt=NT_SB8)         # and no addend
for _ci, _co in ((40, 48), (48, 40), (24, 24), (8, 96)):                                        # conv3x3_sb weight gradient
    for _B, _H, _W in _REFUSAL_MAPS:
        _refuse("c3_wrw", "c3_wrw", (_B, _ci, _co, _H, _W))
for _W in (1, 5, 31, 33, 65, 127):                                   # ragged widths: f16x3 only
    _refuse("c3_wrw", "c3_wrw", (2, 48, 48, 3, _W), BF16X6)
for _ci, _co in ((48, 64), (16, 32)):                                # a partly filled last channel block: f16x3 only
    _refuse("c3_wrw", "c3_wrw", (1, _ci, _co, 4, 64), BF16X6)
for _B, _H, _W in ((1, 4, 32), (8, 16, 32), (2, 3, 96)):             # version 1 has no 32-pixel segments (the 16 x 32 maps of the 384-channel branch)
    _refuse("c3_wrw", "c3_wrw", (_B, 48, 48, _H, _W), BF16X6, {"CSEG_CONV3X3_SB_WRW_V": "1"})
_refuse("c3_wrw", "c3_wrw", (1, 48, 48, 4, 32), BF16X6, {"CSEG_CONV3X3_SB_WRW_V": " 01"})          # (the library reads the switch with atoi)
_refuse(None, "c3_wrw_wrapper", (1, 40, 48, 3, 5))
for _arith in (F16X3, BF16X6):                                                                  # conv1x1_sb
    for _ci, _co in ((40, 48), (48, 80), (64, 40), (24, 144)):
        for _B, _H, _W in _REFUSAL_MAPS[:2]:
            _refuse("c1", "c1_fwd", (_B, _ci, _co, _H, _W), _arith)
    for _ci, _co in ((40, 48), (48, 40), (8, 8)):
        _refuse("c1_wrw", "c1_wrw", (2, _ci, _co, 3, 5), _arith)
# conv3x3_s2. Odd input maps: the entry points take the OUTPUT map, so only the predicates (and the weight-gradient wrapper) can refuse
for _hin, _win in ((5, 64), (4, 63), (1, 1), (3, 3), (9, 128), (64, 65)):
    for _p in ("s2_fwd", "s2_bwd", "s2_wrw"):
        _refuse(_p, None, (1, 48, 48, _hin // 2, _win // 2), hin=_hin, win=_win)
_refuse(None, "s2_wrw_wrapper", (1, 48, 48, 2, 32), hin=5, win=64)
for _ci, _co in ((40, 48), (48, 80), (48, 40)):
    _refuse("s2_fwd", "s2_fwd", (1, _ci, _co, 2, 32))
for _ci, _co, _W in ((48, 48, 1), (48, 48, 33), (96, 48, 65), (80, 48, 32), (48, 40, 32)):     # backward-data: even output widths
    _refuse("s2_bwd", "s2_bwd", (1, _ci, _co, 2, _W))
for _ci, _co, _W in ((48, 48, 1), (48, 48, 16), (48, 48, 33), (96, 48, 48), (40, 48, 32), (48, 40, 32)):       # weight gradient: output widths % 32
    _refuse("s2_wrw", "s2_wrw", (1, _ci, _co, 2, _W))
_refuse("s2_fwd", None, (1, 48, 48, 2, 32), BF16X6)
for _ci, _co in ((40, 48), (48, 80), (64, 40), (24, 64)):                                       # conv3x3_dilany
    for (_B, _H, _W), _d in zip(_REFUSAL_MAPS, (36, 2, 12)):
        _refuse("any", "any_fwd", (_B, _ci, _co, _H, _W), d=_d)
for _d in (0, -1):
    _refuse("any", "any_fwd", (1, 64, 48, 5, 33), d=_d)
_refuse("any", None, (1, 64, 48, 5, 33), d=2, d2=3)
_refuse("any", "any_wrapper", (1, 64, 48, 5, 33), BF16X6, d=2)
for _ci, _co in ((40, 48), (48, 40), (8, 64)):
    _refuse("any_wrw", "any_wrw", (1, _ci, _co, 5, 33), d=2)
_refuse(None, "any_wrw", (1, 64, 48, 5, 33), d=0)
# grouped launches: members need Cin >= 32 (and % 16) and Cout % 48; f16x3; at most eight members
_GOOD = (1, 48, 48, 3, 5)
for _bad in ((1, 16, 48, 3, 5), (1, 16, 16, 1, 1), (2, 16, 96, 9, 65), (1, 48, 64, 3, 5), (1, 48, 16, 3, 5), (1, 40, 48, 3, 5), (1, 48, 80, 1, 65)):
    for _members in ([_GOOD, _bad], [_bad, _GOOD, _GOOD]):
        _refuse(None, "group_fwd", _bad, members=_members)
for _bad in ((1, 48, 64, 3, 5), (1, 40, 48, 3, 5), (1, 48, 16, 1, 1)):
    _refuse(None, "group_wrw", _bad, members=[_GOOD, _bad])
_refuse(None, "group_fwd", _GOOD, BF16X6, members=[_GOOD, _GOOD])
_refuse(None, "group_wrw", _GOOD, BF16X6, members=[_GOOD, _GOOD])
_refuse(None, "group_fwd", _GOOD, members=[_GOOD] * 9)
for _channels in ((16, 48), (48, 16), (48, 64, 96), (40, 48)):       # 64: no grouped tile body; 16 / 40: below 32 / not a branch width
    _refuse("blocks", None, _GOOD, channels=_channels)
_refuse("blocks", None, _GOOD, BF16X6, channels=(48, 96))
_refuse("blocks", None, _GOOD, channels=(48,))


def run_refusals(K, device, monkeypatch, setup_fn):
    """Refusals only: nothing is launched (see above). -> the number of (predicate, entry) assertions made."""
    import ctypes
    import pytest
    n = 0
    for pred, entry, case, arith, env, extra in REFUSALS:
        what = (pred, entry, case, arith, env, extra)
        with monkeypatch.context() as m:
            setup_fn(K, m, arith, env)
            if pred is not None:
                assert not REFUSAL_PREDICATES[pred](K, device, *case, **extra), "the predicate accepts %s" % (what,)
                n += 1
            if entry is not None:
                buf = torch.zeros(1024, device=device)
                with pytest.raises(RuntimeError):
                    REFUSAL_ENTRIES[entry](K, ctypes.c_void_p(buf.data_ptr()), *case, **extra)
                n += 1
    return n


# ---- through the autograd nodes at lattice corners -------------------------------------------------------------------------------------------
# (wrapper, geometry, [case], bias). The channel pairs are ones whose THREE directions the nodes route to the project's kernels
# (equal channel counts from CONV3X3_SB_WRW_CHANNELS; stride 2: output widths % 32), so nothing here is a library call.
AUTOGRAD_LATTICE = [
    ("conv3x3_split_bf16", (3, 1), [(2, 48, 48, 1, 3), (1, 96, 96, 2, 65), (3, 64, 64, 3, 1)], True),
    ("conv1x1_split_bf16", (1, 1), [(1, 48, 64, 1, 1), (3, 64, 48, 2, 3), (2, 48, 144, 1, 65)], True),
    ("conv1x1_split_skip", (1, 1), [(1, 48, 48, 1, 2), (3, 64, 64, 2, 1), (1, 144, 144, 1, 65)], True),
    ("conv3x3_s2_split", (3, 2), [(1, 48, 48, 1, 32), (3, 64, 64, 2, 64), (2, 96, 48, 3, 96)], False),
    ("conv3x3_dilany_split", (3, 1), [(1, 64, 48, 1, 3, 2), (3, 48, 64, 2, 1, 36), (1, 64, 128, 2, 17, 5)], True),
    ("conv3x3_split_fork", (3, 1), [(1, 48, 48, 1, 2), (3, 96, 96, 2, 1), (1, 192, 192, 2, 65)], False),
]

# the library calls of one forward + backward through each wrapper: forward, backward-data (with the epilogue add for the two-output
# nodes), weight gradient
AUTOGRAD_ENTRY_POINTS = {
    "conv3x3_split_bf16": ("cseg_conv3x3_split_fwd", "cseg_conv3x3_split_fwd", "cseg_conv3x3_split_wrw"),
    "conv1x1_split_bf16": ("cseg_conv1x1_split_fwd", "cseg_conv1x1_split_fwd", "cseg_conv1x1_split_wrw"),
    "conv1x1_split_skip": ("cseg_conv1x1_split_fwd", "cseg_conv1x1_split_fwd_add", "cseg_conv1x1_split_wrw"),
    "conv3x3_s2_split": ("cseg_conv3x3_s2_split_fwd", "cseg_conv3x3_s2_split_bwd", "cseg_conv3x3_s2_split_wrw"),
    "conv3x3_dilany_split": ("cseg_conv3x3_split_dilany_fwd", "cseg_conv3x3_split_dilany_fwd", "cseg_conv3x3_split_dilany_wrw"),
    "conv3x3_split_fork": ("cseg_conv3x3_split_fwd", "cseg_conv3x3_split_fwd_add", "cseg_conv3x3_split_wrw"),
}


def run_autograd_lattice(K, device, entry):
    """One module-level wrapper on `dense` operands at three corner shapes: y, dx, dw (and db) torch.equal to float64 autograd. The
    two-output nodes (skip / fork) get a gradient on BOTH outputs, so the epilogue add of the backward-data kernel is in."""
    name, (k, stride), cases, with_bias = entry
    for case in cases:
        dil = case[5] if len(case) > 5 else 1
        geo, c5 = Geo(k, stride, dil), tuple(case[:5])
        x, w, _, bias, _ = operands(geo, "fwd", "dense", c5, with_bias, False)
        dy = operands(geo, "bwd", "dense", c5)[0]
        two = name in ("conv1x1_split_skip", "conv3x3_split_fork")
        g = _ints(tuple(x.shape), _gen("skip gradient", name, case)) if two else None
        xd, wd, bd, dyd, gd = _dev(device, x, w, bias, dy, g)
        for t in (xd, wd, bd):
            if t is not None:
                t.requires_grad_(True)
        fn = getattr(K, name)
        xin = xd * 1.0                                 # a non-leaf input, as inside the network
        calls, orig = [], K._hip.call
        K._hip.call = lambda nm, *a: (calls.append(nm), orig(nm, *a))[1]
        try:
            if name == "conv3x3_dilany_split":
                out = fn(xin, wd, bd, dil)
            elif name in ("conv3x3_s2_split", "conv3x3_split_fork"):
                out = fn(xin, wd)
            else:
                out = fn(xin, wd, bd)
            torch.autograd.backward(list(out) if two else [out], [dyd, gd] if two else [dyd])
        finally:
            K._hip.call = orig
        # forward, backward-data and the weight gradient each ran on the project's entry point, once (a fallback to the library
        # would be exact on these integers too, and go unnoticed otherwise)
        conv_calls = sorted(c for c in calls if c in sum(AUTOGRAD_ENTRY_POINTS.values(), ()))
        assert conv_calls == sorted(AUTOGRAD_ENTRY_POINTS[name]), (name, case, calls)
        x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
        b64 = None if bias is None else bias.double().requires_grad_(True)
        y64 = F.conv2d(x64, w64, b64, stride, geo.pad, dil)
        (y64 * dy.double()).sum().backward()
        dx64 = x64.grad + (g.double() if two else 0)
        for r in (y64, dx64, w64.grad):
            assert torch.equal(r.detach().float().double(), r.detach()), "the float64 reference is not an fp32 number"
        what = "%s %s " % (name, case)
        check(out[0] if two else out, y64.detach(), what + "y")
        if two:
            check(out[1], x.double(), what + "skip")
        check(xd.grad, dx64, what + "dx")
        check(wd.grad, w64.grad, what + "dw")
        if bias is not None:
            check(bd.grad, b64.grad, what + "db")


# The residual-block nodes (basic_block_split, basic_block_group) run their BatchNorms on BATCH statistics only -- there is no
# eval-mode path through them, and a normalisation by batch moments leaves no integers. What is compared is therefore the blocks'
# CONVOLUTION calls and the plumbing between them: the BatchNorm launches are replaced by their value at identity statistics and unit
# weight (y = relu(x [+ residual]), dx = dy * mask), computed with torch on the device, with the same hand-overs (the epilogue
# statistics must be there, the max|.| records are produced for the next convolution); every convolution, weight gradient and epilogue
# add is the node's own call. Operands: x, dy in [-1, 1], w1 in [-2, 2], w2 in [-1, 1], so that every partial sum of the chain stays
# below 162 C^2 + 1 < 2^24 (asserted) and the block is exact in any order.
BLOCK_CORNERS = [(2, 48, 1, 3), (1, 96, 2, 65), (3, 192, 3, 1)]                       # B, C, H, W
BLOCK_GROUPS = [[(1, 48, 1, 65), (2, 96, 3, 1)], [(3, 48, 2, 33), (1, 96, 1, 5), (1, 192, 5, 2)], [(1, 192, 1, 1), (2, 96, 2, 31), (1, 48, 8, 1), (1, 48, 4, 66)]]


def _identity_bn(K, monkeypatch):
    seen = {"fwd": 0, "bwd": 0}

    def amax_into(t, slot):
        return K.tensor_amax(t.contiguous(), slot) if slot is not None else None

    def fwd_one(x, residual):
        assert K.known_tile_stats(x) is not None, "the convolution epilogue left no statistics"
        y = torch.relu(x.detach() + (residual.detach() if residual is not None else 0))
        seen["fwd"] += 1
        return y, torch.zeros(x.shape[1], 2, device=x.device), amax_into(y, K.amax_request(x))

    def bwd_one(dy, x, out, mode, am):
        mask = ((out if mode == 2 else x).detach() > 0).to(dy.dtype)
        dx = dy.detach() * mask
        amax_into(dx, am)
        seen["bwd"] += 1
        zc = torch.zeros(x.shape[1], device=x.device)
        return dx, zc, zc.clone(), (dx.clone() if mode == 2 else None)

    monkeypatch.setattr(K, "_bn_train_fwd", lambda x, weight, bias, residual, bn: fwd_one(x, residual))
    monkeypatch.setattr(K, "bn_bwd", lambda dy, x, out, mi, weight, bias, mode, training, want_dx, amax=None: bwd_one(dy, x, out, mode, amax))

    def group_fwd(xs, bns, residuals, relu):
        r = [fwd_one(x, res) for x, res in zip(xs, residuals)]
        return [t[0] for t in r], [t[1] for t in r], [t[2] for t in r]

    def group_bwd(dys, xs, outs, mis, bns, mode):
        res = []
        for dy, x, out in zip(dys, xs, outs):
            am = K.amax_request(x)
            res.append(bwd_one(dy, x, out, mode, am) + (am,))
        return res

    monkeypatch.setattr(K, "bn_group_fwd", group_fwd)
    monkeypatch.setattr(K, "bn_group_bwd", group_bwd)
    return seen


def _block_operands(case):
    B, C, H, W = case
    assert 162 * C * C + 1 < 2 ** 24
    rng = _gen("block", case)
    x, dy = _ints((B, C, H, W), rng, -1, 1), _ints((B, C, H, W), rng, -1, 1)
    w1, w2 = _ints((C, C, 3, 3), rng, -2, 2), _ints((C, C, 3, 3), rng, -1, 1)
    x64, w164, w264 = (t.double().requires_grad_(True) for t in (x, w1, w2))
    y64 = torch.relu(F.conv2d(torch.relu(F.conv2d(x64, w164, None, 1, 1)), w264, None, 1, 1) + x64)
    (y64 * dy.double()).sum().backward()
    refs = (y64.detach(), x64.grad, w164.grad, w264.grad)
    for r in refs:
        assert torch.equal(r.float().double(), r) and float(r.abs().max()) < 2 ** 24
    return x, dy, w1, w2, refs


def run_block_lattice(K, device, monkeypatch, cases, grouped):
    """basic_block_split per case, or basic_block_group over all of them: out, dx, dw1, dw2 torch.equal to float64 autograd."""
    from contrastiveseg_amd.lib.models.backbones.hrnet_backbone import BasicBlock
    from contrastiveseg_amd.lib.models.tools.module_helper import mark_conv_bn_pairs
    monkeypatch.setattr(K, "CONV_EPILOGUE_STATS", True)
    seen = _identity_bn(K, monkeypatch)
    ops = [_block_operands(c) for c in cases]
    blocks, xs = [], []
    for (B, C, H, W), (x, dy, w1, w2, _) in zip(cases, ops):
        blk = mark_conv_bn_pairs(BasicBlock(C, C, bn_type="torchbn").train()).to(device)
        with torch.no_grad():
            blk.conv1.weight.copy_(w1)
            blk.conv2.weight.copy_(w2)
        blocks.append(blk)
        xs.append(_dev(device, x)[0].requires_grad_(True))
    ins = [x * 1.0 for x in xs]
    if grouped:
        assert K.basic_block_group_ok(blocks, ins), cases
        outs = K.basic_block_group(blocks, ins)
    else:
        for xi, blk in zip(ins, blocks):
            assert K.basic_block_split_ok(xi, blk.conv1.weight, blk.conv2.weight), tuple(xi.shape)
        outs = [K.basic_block_split(xi, blk) for xi, blk in zip(ins, blocks)]
    torch.autograd.backward(outs, [_dev(device, o[1])[0] for o in ops])
    assert seen["fwd"] == 2 * len(cases) and seen["bwd"] == 2 * len(cases), seen
    for case, blk, x, out, o in zip(cases, blocks, xs, outs, ops):
        what = "%s %s " % ("basic_block_group" if grouped else "basic_block_split", case)
        check(out, o[4][0], what + "out")
        check(x.grad, o[4][1], what + "dx")
        check(blk.conv1.weight.grad, o[4][2], what + "dw1")
        check(blk.conv2.weight.grad, o[4][3], what + "dw2")
