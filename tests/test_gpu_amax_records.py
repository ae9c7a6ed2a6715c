"""The max|.| records that the producers of a tensor leave for the split-operand convolutions that read it (kernels.amax_slot /
amax_request / amax_attach / known_amax / amax_of, csrc/cseg_split.h: amax_publish_block): the f16x3 kernels scale an operand by
2^(14 - floor(log2 max|x|)) read from that record, so a record that is too small overflows fp16 only when the largest element sits at
the top of its binade, one that is too large (or belongs to another tensor, or to an earlier graph replay) silently drops low bits --
neither moves an output beyond the fp64 bounds of the parity tests.

1. Every producer: the record's maximum word is BIT-equal to torch's max|.| of the tensor the kernel stored (what the consumer reads),
   every word outside the 32 slots is zero; the stored tensor itself against the fp64 module chain of tests/test_gpu_bn.py at that
   file's bounds. The extreme is planted at the first / the last element, through the residual or dy alone, under the ReLU (a large
   negative pre-activation the record must not see) and as a negative value of the largest magnitude.
2. A consumer gives the same bits with the producer's record as with a fresh cseg_amax_f32 pass; forwarded records (fan_out, the 1x1
   skip alias), the version guard, records across an arena switch.
3. The projection head's merged record (affine part + corrected rows): bounded from below by max|du| and from above by the affine map.
4. A hipGraph replay starts from zeroed records (GPU only).

tests/test_emu_amax_records.py replays these bodies on the emulated device in both wave orders.

Where the kernels set the terms: cseg_affine_channels reads 16 bytes at a time and refuses planes with P % 4 != 0 (asserted as a
refusal); a member of a grouped launch publishes into slot (block index of the LAUNCH) & 31, so its record equals the one-layer
call's in value (largest word), not word by word; batch statistics of one value have no fp64 module to compare with, so the
one-element shape runs the training-mode backward against the stored tensor only."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
# (B, C, H, W): the smallest shapes at which each path of csrc/bn.hip is taken (CHUNK = 4096 floats per block, the 16-byte path needs
# HW % 4 == 0, a block publishes into slot blockIdx.x & 31)
SHAPES = [
    (1, 1, 1, 1),        # one element, one block, scalar path (frozen statistics only: batch statistics of one value are degenerate)
    (2, 3, 1, 3),        # scalar path, fewer elements than a wave
    (3, 5, 7, 9),        # HW = 63: scalar path, ragged
    (2, 48, 5, 8),       # vector path, 96 blocks: every slot is written by three blocks
    (1, 2, 65, 64),      # HW = 4160: two chunks, the second of 64 floats, vector path
    (1, 3, 17, 241),     # HW = 4097: two chunks, the second of ONE float, scalar path
    (2, 40, 4, 4),       # 80 blocks of 16 floats: most lanes idle
]
TRAIN_SHAPES = SHAPES[1:]
COMBOS = [(False, False), (True, False), (True, True), (False, True)]          # (relu, residual)
BWD_COMBOS = [(False, False), (True, False), (True, True)]                     # modes 0, 1, 2
GROUPS = [
    [(1, 48, 9, 70), (1, 96, 5, 36)],
    [(2, 48, 4, 64), (2, 96, 6, 33), (1, 192, 3, 20)],        # the second member has HW % 4 != 0: per-member fallback of cseg_bn_group_apply
]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _k():
    from contrastiveseg_amd import kernels as K
    assert K.SPLIT_ARITH == "f16x3"
    return K


def _reference(*a):
    from test_gpu_bn import _reference as ref
    return ref(*a)


def _bits(t):
    """Bit pattern of max|t| as torch computes it over the stored values."""
    return int(t.detach().abs().max().view(torch.int32))


def check_record(rec, t):
    """The record describes the STORED tensor: its largest word is the bit pattern of torch's own max|t| (all zero for an all-zero t),
    only the 32 slot words are ever written, and it is an int32 record of K.AMAX_WORDS words on t's device."""
    K = _k()
    assert rec is not None
    assert rec.dtype == torch.int32 and rec.numel() == K.AMAX_WORDS and rec.device == t.device, (rec.dtype, rec.numel(), rec.device)
    words = rec.view(32, 32)                   # 32 slots, 32 words apart (include/cseg_hip.h; compare tests/emu/harness.amax)
    assert int(rec.max()) == _bits(t), (int(rec.max()), _bits(t))
    assert int(words[:, 0].min()) >= 0
    assert not bool(words[:, 1:].any()), "a word that is no slot was written"


def _close(got, ref, rel):
    err = float((got.detach().cpu().double() - ref).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    assert err <= rel * scale, (err, scale)


def _argmax(t):
    return int(t.detach().abs().reshape(-1).argmax())


# ---- operands --------------------------------------------------------------------------------------------------------------------
PLANTED = 64.0          # the planted extreme: a few times the ordinary values, so that the fp64 bounds still bind those
FWD_PLANTS = ("first", "last", "residual", "neg_relu", "neg")
BWD_PLANTS = ("first", "last", "dy", "masked", "neg")


def _fwd_plants(relu, res):
    """(a) first element, (b) last element, (c) largest only through the residual, (d) under the ReLU a large negative pre-activation,
    (e) without it a negative value of the largest magnitude."""
    return ["first", "last"] + (["residual"] if res else []) + ["neg_relu" if relu else "neg"]


def _bwd_plants(relu):
    """(a), (b), (c) largest only through dy, (d) a large dy where the ReLU was off, (e) a negative value of the largest magnitude."""
    return ["first", "last", "dy", "masked" if relu else "neg"]


def _random(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=gen) * 1.7 + torch.randn(1, C, 1, 1, generator=gen) * 3.0
    r = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    w = torch.randn(C, generator=gen).clamp(-2.0, 2.0)
    b = torch.randn(C, generator=gen)
    # running statistics near the batch's own (mean within a third of a standard deviation, variance within a factor 1.5): with frozen
    # statistics the outputs then stay of order ten, so that the planted extreme below need not be larger than a few tens and the
    # fp64 bounds (relative to max|reference|) stay meaningful for the ordinary elements
    rm = x.mean(dim=(0, 2, 3)) + 0.5 * torch.randn(C, generator=gen)
    rv = (torch.rand(C, generator=gen) + 0.5) * 2.9
    return x, r, g, w, b, rm, rv


@functools.lru_cache(maxsize=None)
def _fwd_case(shape, relu, res, train, plant):
    """Seeded operands with the extreme of y planted through the inputs, and the fp64 reference (computed once per case, read-only)."""
    B, C, H, W = shape
    n, HW = B * C * H * W, H * W
    x, r, g, w, b, rm, rv = _random(shape, 1000 * sum(shape) + 16 * FWD_PLANTS.index(plant) + 4 * relu + 2 * res + bool(train))
    p = {"first": 0, "last": n - 1, "residual": n // 2, "neg_relu": n // 3, "neg": n // 3}[plant]
    c = (p // HW) % C
    sign = -1.0 if plant.startswith("neg") else 1.0
    if res:
        r.view(-1)[p] = sign * PLANTED
    else:
        # through x and the channel's weight / bias: the channel's extreme value under a large positive weight
        ch = x[:, c]
        rm[c], rv[c] = float(ch.mean()), 1.0
        x.view(-1)[p] = float(ch.max()) + 10.0 if sign > 0 else float(ch.min()) - 10.0
        w[c], b[c] = 16.0, 0.5 * sign
    ref = None
    if train is not None:
        ref = _reference(x, r, g, w, b, rm, rv, relu, res, train)[:2]
    return dict(x=x, r=r, g=g, w=w, b=b, rm=rm, rv=rv, p=p, ref=ref)


@functools.lru_cache(maxsize=None)
def _bwd_case(shape, relu, res, train, plant):
    """Seeded operands with the extreme of dx planted through dy (x at the channel mean there, so that the batch-statistics terms do
    not move it), the ReLU held open (or, `masked`, shut) at that element through x / bias / residual."""
    B, C, H, W = shape
    n, HW = B * C * H * W, H * W
    x, r, g, w, b, rm, rv = _random(shape, 2000 * sum(shape) + 16 * BWD_PLANTS.index(plant) + 4 * relu + 2 * res + bool(train))
    p = {"first": 0, "last": n - 1, "dy": n // 2, "masked": n // 3, "neg": n // 3}[plant]
    c = (p // HW) % C
    ch = x[:, c]
    w[c], b[c] = 2.0, 1.0
    if plant == "masked":
        x.view(-1)[p] = float(ch.min()) - 10.0
        rm[c], rv[c] = float(ch.mean()), 1.0
        if res:
            r.view(-1)[p] = -PLANTED
        g.view(-1)[p] = PLANTED
    else:
        if ch.numel() > 1:
            x.view(-1)[p] = 0.0
            x.view(-1)[p] = float(ch.sum()) / (ch.numel() - 1)
        rm[c], rv[c] = float(ch.mean()), 1.0
        if res:
            r.view(-1)[p] = 5.0
        g.view(-1)[p] = -PLANTED if plant == "neg" else PLANTED
    ref = None
    if train is not None:
        ref = _reference(x, r, g, w, b, rm, rv, relu, res, train)[:2]
    return dict(x=x, r=r, g=g, w=w, b=b, rm=rm, rv=rv, p=p, ref=ref)


def _on(dev, c, *names):
    return [c[k].to(dev).clone() for k in names]            # (the cached operands stay as they are: bn_fwd updates running statistics in place)


def _mi_frozen(rm, rv):
    return torch.stack([rm, torch.rsqrt(rv + EPS)], dim=1).contiguous()        # fused_bn.bn_forward, eval branch


def _forward(K, dev, c, relu, res, route):
    """route: "fused" bn_fwd | "sync" bn_stats -> bn_finalize(count 0) -> bn_apply | "frozen" bn_apply with running statistics
    -> (y, mean_invstd, record)"""
    x, r, w, b, rm, rv = _on(dev, c, "x", "r", "w", "b", "rm", "rv")
    r = r if res else None
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    rec = K.amax_request(x)
    if route == "fused":
        y, mi = K.bn_fwd(x, w, b, r, relu, EPS, MOM, rm, rv, nbt, amax=rec)
    elif route == "sync":
        # one rank: the all-reduce is the identity, the count comes from row C of the moments
        mi = K.bn_finalize(K.bn_stats(x), 0.0, EPS, MOM, rm, rv, nbt)
        y = K.bn_apply(x, mi, w, b, r, relu, amax=rec)
    else:
        mi = _mi_frozen(rm, rv)
        y = K.bn_apply(x, mi, w, b, r, relu, amax=rec)
    return y, mi, rec


def _check_forward(c, y, rec, plant):
    check_record(rec, y)
    if c["ref"] is not None:
        _close(y, c["ref"][0], 1e-5)
    p = c["p"]
    if plant in ("first", "last"):
        assert _argmax(y) == p, (plant, _argmax(y), p)
    elif plant == "neg":
        assert _argmax(y) == p and float(y.detach().reshape(-1)[p]) < 0.0
    elif plant == "neg_relu":
        assert float(y.detach().reshape(-1)[p]) == 0.0


def _backward(K, dev, c, relu, res, train, route, want_dx=True):
    """route: "fused" bn_bwd | "sync" bn_bwd_reduce -> bn_bwd_apply(count 0) -> (dx, record)"""
    x, r, g, w, b, rm, rv = _on(dev, c, "x", "r", "g", "w", "b", "rm", "rv")
    r = r if res else None
    mode = 0 if not relu else (2 if res else 1)
    if train:
        out, mi = K.bn_fwd(x, w, b, r, relu, EPS, MOM, None, None, None)
    else:
        mi = _mi_frozen(rm, rv)
        out = K.bn_apply(x, mi, w, b, r, relu)
    out = out if mode == 2 else None
    rec = K.amax_request(x)
    if route == "fused":
        dx = K.bn_bwd(g, x, out, mi, w, b, mode, train, want_dx, amax=rec)[0]
    else:
        sums, _, _, gm = K.bn_bwd_reduce(g, x, out, mi, w, b, mode)
        dx = K.bn_bwd_apply(gm if mode == 2 else g, x, mi, w, b, sums, 0.0, mode == 1, amax=rec)
    return dx, rec


def _check_backward(c, dx, rec, plant):
    check_record(rec, dx)
    if c["ref"] is not None:
        _close(dx, c["ref"][1], 2e-5)
    p = c["p"]
    if plant in ("first", "last"):
        assert _argmax(dx) == p, (plant, _argmax(dx), p)
    elif plant == "neg":
        assert _argmax(dx) == p and float(dx.reshape(-1)[p]) < 0.0


# ---- 1. the record equals the stored tensor, for every producer ----------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "sync"])
@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_training_forward_leaves_the_record_of_the_stored_output(shape, route):
    """bn_fwd (cseg_bn_fwd_amax) and the SyncBN route on one rank bn_stats -> bn_finalize(count 0) -> bn_apply (cseg_bn_apply_amax)."""
    dev, K = _dev(), _k()
    for relu, res in COMBOS:
        for plant in _fwd_plants(relu, res):
            c = _fwd_case(shape, relu, res, True, plant)
            y, _, rec = _forward(K, dev, c, relu, res, route)
            _check_forward(c, y, rec, plant)


@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_forward_leaves_the_record_of_the_stored_output(shape):
    """bn_apply with mean / invstd built from the running statistics as fused_bn.bn_forward's eval branch builds them."""
    dev, K = _dev(), _k()
    for relu, res in COMBOS:
        for plant in _fwd_plants(relu, res):
            c = _fwd_case(shape, relu, res, False, plant)
            y, _, rec = _forward(K, dev, c, relu, res, "frozen")
            _check_forward(c, y, rec, plant)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_leaves_the_record_of_the_stored_input_gradient(shape, train):
    """bn_bwd (cseg_bn_bwd_amax), modes 0 / 1 / 2; without dx no record is written."""
    dev, K = _dev(), _k()
    for relu, res in BWD_COMBOS:
        if train and shape == (1, 1, 1, 1):
            # batch statistics of ONE value (torch refuses the module in training mode): dx is identically zero
            c = _bwd_case(shape, relu, res, None, "dy")
            dx, rec = _backward(K, dev, c, relu, res, True, "fused")
            check_record(rec, dx)
            assert _bits(dx) == 0
            continue
        for plant in _bwd_plants(relu):
            c = _bwd_case(shape, relu, res, train, plant)
            dx, rec = _backward(K, dev, c, relu, res, train, "fused")
            _check_backward(c, dx, rec, plant)
        dx, rec = _backward(K, dev, c, relu, res, train, "fused", want_dx=False)
        assert dx is None and int(rec.abs().max()) == 0, "a record was written although no dx was stored"


@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_sync_backward_leaves_the_record_of_the_stored_input_gradient(shape):
    """bn_bwd_reduce -> bn_bwd_apply(count 0) (cseg_bn_bwd_apply_amax): the SyncBN route on one rank, mask_from_x both ways."""
    dev, K = _dev(), _k()
    for relu, res in BWD_COMBOS:
        for plant in _bwd_plants(relu):
            c = _bwd_case(shape, relu, res, True, plant)
            dx, rec = _backward(K, dev, c, relu, res, True, "sync")
            _check_backward(c, dx, rec, plant)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_module_attaches_the_records_of_output_and_input_gradient(shape, train, monkeypatch):
    """FusedBatchNorm2d end to end: known_amax(y) after the forward; after the backward the record bn_backward handed to K.bn_bwd."""
    dev, K = _dev(), _k()
    from contrastiveseg_amd.lib.models.tools.fused_bn import FusedBatchNorm2d
    recs = []
    bn_bwd = K.bn_bwd

    def spy(*a, **k):
        res = bn_bwd(*a, **k)
        recs.append((k.get("amax"), res[0]))
        return res
    monkeypatch.setattr(K, "bn_bwd", spy)
    for relu, res in COMBOS:
        for kind, plants in (("bwd", _bwd_plants(relu)), ("fwd", _fwd_plants(relu, res))):
            for plant in plants:
                c = (_bwd_case if kind == "bwd" else _fwd_case)(shape, relu, res, train, plant)
                x, r, g, w, b, rm, rv = _on(dev, c, "x", "r", "g", "w", "b", "rm", "rv")
                m = FusedBatchNorm2d(shape[1]).to(dev)
                with torch.no_grad():
                    m.weight.copy_(w); m.bias.copy_(b); m.running_mean.copy_(rm); m.running_var.copy_(rv)
                m.train(train)
                x.requires_grad_(True)
                r.requires_grad_(True)
                xin = x * 1.0                       # a non-leaf input, as inside a network: its gradient is what the producer of x reads
                arrived = []
                xin.register_hook(lambda gr: arrived.append(gr))
                y = m(xin, residual=r if res else None, relu=relu)
                rec = K.known_amax(y)
                check_record(rec, y)
                _close(y, c["ref"][0], 1e-5)
                if kind == "fwd":
                    _check_forward(c, y, rec, plant)
                    continue
                del recs[:]
                y.backward(g)
                assert len(recs) == 1 and recs[0][0] is not None, "bn_backward did not ask for the record of dx"
                rec, dx = recs[0]
                _check_backward(c, dx, rec, plant)
                # ... and it travels with dx to the node in front
                assert K.known_amax(dx) is rec, "the record was not attached to dx"
                assert len(arrived) == 1 and K.known_amax(arrived[0]) is rec and torch.equal(arrived[0], x.grad)


def test_degenerate_operands_leave_all_zero_records(monkeypatch):
    """weight = bias = 0: y and its record are all zero and a split convolution that reads it returns exact zeros; dy = 0: the record
    of dx is all zero."""
    dev, K = _dev(), _k()
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    shape = (2, 48, 5, 8)
    c = dict(_fwd_case(shape, True, True, None, "first"))
    c["w"], c["b"] = torch.zeros(48), torch.zeros(48)
    for route in ("fused", "sync", "frozen"):
        for relu in (False, True):
            y, _, rec = _forward(K, dev, c, relu, False, route)
            check_record(rec, y)
            assert int(rec.abs().max()) == 0 and _bits(y) == 0
            wc = torch.randn(48, 48, 3, 3, generator=torch.Generator().manual_seed(1)).to(dev)
            z = K.conv3x3_sb_run(y, wc, False, ax=rec)
            assert bool(torch.isfinite(z).all()) and _bits(z) == 0
    for relu, res in BWD_COMBOS:
        for train in (True, False):
            c = dict(_bwd_case(shape, relu, res, None, "dy"))
            c["g"] = torch.zeros(shape)
            for route in (("fused", "sync") if train else ("fused",)):
                dx, rec = _backward(K, dev, c, relu, res, train, route)
                check_record(rec, dx)
                assert int(rec.abs().max()) == 0 and _bits(dx) == 0


def test_no_record_under_bf16x6(monkeypatch):
    """With the bf16x6 arithmetic nobody reads a record: amax_request returns None, a BatchNorm forward + backward leaves none, and no
    producer entry point is handed a non-null amax_out."""
    dev, K = _dev(), _k()
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd.lib.models.tools.fused_bn import FusedBatchNorm2d
    monkeypatch.setattr(K, "SPLIT_ARITH", "bf16x6")
    handed = []
    orig = _hip.call

    def spy(name, *a):
        if name.endswith("_amax") and name != "cseg_upcat_fwd_amax" or name == "cseg_affine_channels":
            handed.append((name, getattr(a[-2], "value", a[-2])))      # (.., amax_out, stream)
        elif name.startswith("cseg_bn_group_"):
            members = a[0]._obj                                          # (byref(member table), n, ..): amax_out travels in the table
            handed.extend((name, members[i].amax_out) for i in range(a[1]))
        return orig(name, *a)
    monkeypatch.setattr(_hip, "call", spy)
    c = _fwd_case((2, 48, 5, 8), True, True, True, "first")
    x, r, g, w, b = _on(dev, c, "x", "r", "g", "w", "b")
    assert K.amax_request(x) is None
    for train in (True, False):
        m = FusedBatchNorm2d(48).to(dev).train(train)
        x = x.detach().requires_grad_(True)
        y = m(x, residual=r, relu=True)
        assert K.known_amax(y) is None and not hasattr(y, "_cseg_amax")
        y.backward(g)
        _close(y, _reference(c["x"], c["r"], c["g"], torch.ones(48), torch.zeros(48), torch.zeros(48), torch.ones(48), True, True, train)[0], 1e-5)
    out, rec = K.affine_channels(x.detach(), w, b)
    assert rec is None
    # the grouped producers: their inputs carry epilogue statistics (one-layer convolutions here: the grouped one is f16x3 only)
    _fresh_split_state(monkeypatch, K)
    shapes = GROUPS[0]
    gen = torch.Generator().manual_seed(9)
    cs = [K.conv3x3_sb_run((torch.randn(s, generator=gen) * 0.7).to(dev), (torch.randn(s[1], s[1], 3, 3, generator=gen) / (3.0 * s[1] ** 0.5)).to(dev),
                           want_stats=True) for s in shapes]
    case = _group_case(shapes, "first", 9, bwd=True)
    bns = _bn_modules(dev, shapes, case)
    rs, gs = [m_["r"].to(dev) for m_ in case], [m_["g"].to(dev) for m_ in case]
    ys, mis, ams = K.bn_group_fwd(cs, bns, rs, True)
    ys2, _, ams2 = K.bn_group_sync_apply(cs, bns, rs, True, K.bn_group_sync_moments(cs))
    assert all(a is None for a in ams + ams2) and all(torch.equal(a, b_) for a, b_ in zip(ys, ys2))
    got = K.bn_group_bwd(gs, cs, ys, mis, bns, 2)
    packed, state = K.bn_group_sync_bwd_reduce(gs, cs, ys, mis, bns, 2)
    got2 = K.bn_group_sync_bwd_apply(state, packed)
    assert all(t[4] is None for t in got + got2) and all(torch.equal(t[0], t2[0]) for t, t2 in zip(got, got2))
    for s, cv, m_, y, t in zip(shapes, cs, case, ys, got):
        ref = _reference(cv.cpu(), m_["r"], m_["g"], m_["w"], m_["b"], torch.zeros(s[1]), torch.ones(s[1]), True, True, True)
        _close(y, ref[0], 1e-5)
        _close(t[0], ref[1], 2e-5)
    names = [n for n, _ in handed]
    for want in ("cseg_bn_fwd_amax", "cseg_bn_apply_amax", "cseg_bn_bwd_amax", "cseg_affine_channels", "cseg_bn_group_apply", "cseg_bn_group_bwd",
                 "cseg_bn_group_bwd_apply"):
        assert want in names, (want, sorted(set(names)))
    assert all(v is None for _, v in handed), handed


# (B, C, H, W) of u: one tiny plane, 96 blocks, a plane of two chunks (P / 4 = 2145 > 2048 float4 per chunk)
AFFINE_SHAPES = [(2, 3, 1, 4), (2, 48, 5, 8), (1, 2, 33, 260)]


@pytest.mark.parametrize("shape", AFFINE_SHAPES)
def test_affine_channels_leaves_the_record_of_the_stored_output(shape):
    """out = a_c + b_c * u (cseg_affine_channels): one fma per element, so the stored values lie within 2^-24 of the fp64 result,
    relative to that result; bound 2^-23 of the largest."""
    dev, K = _dev(), _k()
    B, C, H, W = shape
    n = B * C * H * W
    for plant in ("first", "last", "neg", "zero"):
        gen = torch.Generator().manual_seed(sum(shape) + len(plant))
        u = torch.randn(shape, generator=gen)
        a, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen).clamp(-2.0, 2.0)
        p = {"first": 0, "last": n - 1, "neg": n // 3, "zero": 0}[plant]
        c = (p // (H * W)) % C
        if plant == "zero":
            a, b = torch.zeros(C), torch.zeros(C)
        else:
            b[c] = 2.0
            u.view(-1)[p] = -PLANTED if plant == "neg" else PLANTED
        out, rec = K.affine_channels(u.to(dev), a.to(dev), b.to(dev))
        check_record(rec, out)
        ref = a.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1) * u.double()
        _close(out, ref, 2.0 ** -23)
        if plant == "zero":
            assert int(rec.abs().max()) == 0
        else:
            assert _argmax(out) == p and (float(out.reshape(-1)[p]) < 0.0) == (plant == "neg")
    out, rec = K.affine_channels(u.to(dev), a.to(dev), b.to(dev), want_amax=False)
    assert rec is None


def test_affine_channels_refuses_planes_that_are_no_multiple_of_four():
    """The kernel reads 16 bytes at a time (the projection head checks P % 4 == 0 before it calls): anything else is refused, not
    computed with a partial record."""
    dev, K = _dev(), _k()
    u = torch.randn(3, 5, 7, 9).to(dev)
    with pytest.raises(RuntimeError):
        K.affine_channels(u, torch.zeros(5).to(dev), torch.ones(5).to(dev))


# ---- grouped launches ------------------------------------------------------------------------------------------------------------------
def _fresh_split_state(monkeypatch, K):
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 1)
    monkeypatch.setattr(K, "CONV1X1_SB_MIN_TILES", 1)
    monkeypatch.setattr(K, "CONV_EPILOGUE_STATS", True)
    monkeypatch.setattr(K, "_GROUP_SCHED", {})


def _group_conv_outputs(K, dev, shapes, seed):
    """The members' BatchNorm inputs as the residual blocks produce them: ONE grouped convolution launch with the statistics epilogue."""
    gen = torch.Generator().manual_seed(seed)
    xs = [(torch.randn(s, generator=gen) * 0.7 + 0.1).to(dev) for s in shapes]
    ws = [(torch.randn(s[1], s[1], 3, 3, generator=gen) / (3.0 * s[1] ** 0.5)).to(dev) for s in shapes]
    cs, _ = K.conv3x3_group_run([(x, w, False, K.amax_of(x), None) for x, w in zip(xs, ws)], want_stats=True)
    assert all(K.known_tile_stats(c) is not None for c in cs)
    return cs, ws


def _group_case(shapes, plant, seed, bwd=False):
    """Per member: BatchNorm parameters, residual, dy with the extreme planted (forward: through the residual or the channel's weight;
    backward: through dy, the ReLU held open through bias / residual) -> list of dicts of CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for s in shapes:
        B, C, H, W = s
        n, HW = B * C * H * W, H * W
        r, g = torch.randn(s, generator=gen), torch.randn(s, generator=gen)
        w, b = torch.randn(C, generator=gen).clamp(-2.0, 2.0), torch.randn(C, generator=gen)
        p = {"first": 0, "last": n - 1, "neg": n // 3, "masked": n // 3, "weight": n - 1}[plant]
        c = (p // HW) % C
        if plant == "weight":
            w[c], b[c] = 16.0, 0.5
        else:
            sign = -1.0 if plant == "neg" else 1.0
            w[c] = 2.0
            b[c] = -20.0 if plant in ("masked", "neg") else 20.0          # mode 1: the ReLU of the whole channel shut / open
            r.view(-1)[p] = -PLANTED if plant == "masked" else (PLANTED if bwd else PLANTED * sign)       # mode 2: the ReLU at p shut / open
            g.view(-1)[p] = PLANTED * sign
        out.append(dict(r=r, g=g, w=w, b=b, p=p))
    return out


def _bn_modules(dev, shapes, case):
    bns = []
    for s, m in zip(shapes, case):
        bn = nn.BatchNorm2d(s[1]).to(dev)
        with torch.no_grad():
            bn.weight.copy_(m["w"]); bn.bias.copy_(m["b"])
        bns.append(bn)
    return bns


def _same_value(rec_a, rec_b):
    """The two records describe the same maximum. (Word by word they differ by design: a block publishes into slot blockIdx.x & 31, and
    a member's blocks of a grouped launch do not start at block 0.)"""
    assert int(rec_a.max()) == int(rec_b.max())


GROUP_FWD = [(True, False, "weight"), (False, False, "weight"), (True, True, "first"), (True, True, "last"), (True, True, "masked"),
             (False, True, "neg")]
GROUP_BWD = [(1, "first"), (1, "last"), (1, "masked"), (2, "first"), (2, "last"), (2, "masked"), (2, "neg")]


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("gi", range(len(GROUPS)))
def test_grouped_forward_leaves_every_members_record(gi, sync, monkeypatch):
    """bn_group_fwd (cseg_bn_group_tiles_finalize + cseg_bn_group_apply) and bn_group_sync_moments -> bn_group_sync_apply: every
    member's record against that member's stored output, and equal to the record (and the output to the output) of the one-layer calls
    on the same operands."""
    dev, K = _dev(), _k()
    _fresh_split_state(monkeypatch, K)
    shapes = GROUPS[gi]
    cs, _ = _group_conv_outputs(K, dev, shapes, 40 + gi)
    for relu, res, plant in GROUP_FWD:
        case = _group_case(shapes, plant, 50 + gi)
        rs = [m["r"].to(dev) if res else None for m in case]
        bns = _bn_modules(dev, shapes, case)
        if sync:
            ys, mis, ams = K.bn_group_sync_apply(cs, bns, rs, relu, K.bn_group_sync_moments(cs))
        else:
            ys, mis, ams = K.bn_group_fwd(cs, bns, rs, relu)
        for s, cv, m, r, bn, y, am in zip(shapes, cs, case, rs, bns, ys, ams):
            check_record(am, y)
            ref = _reference(cv.cpu(), m["r"], m["g"], m["w"], m["b"], torch.zeros(s[1]), torch.ones(s[1]), relu, res, True)[0]
            _close(y, ref, 1e-5)
            if plant in ("first", "last"):
                assert _argmax(y) == m["p"]
            elif plant == "neg":
                assert _argmax(y) == m["p"] and float(y.reshape(-1)[m["p"]]) < 0.0
            elif plant == "masked":
                assert float(y.reshape(-1)[m["p"]]) == 0.0
            # the one-layer calls
            one = nn.BatchNorm2d(s[1]).to(dev)
            st = K.known_tile_stats(cv)
            if sync:
                mi1 = K.bn_finalize(K.bn_tiles_moments(st), 0.0, EPS, MOM, one.running_mean, one.running_var, one.num_batches_tracked)
            else:
                mi1 = K.bn_tiles_finalize(st, EPS, MOM, one.running_mean, one.running_var, one.num_batches_tracked)
            rec1 = K.amax_request(cv)
            y1 = K.bn_apply(cv, mi1, bn.weight.detach(), bn.bias.detach(), r, relu, amax=rec1)
            check_record(rec1, y1)
            assert torch.equal(y, y1)
            _same_value(am, rec1)


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("gi", range(len(GROUPS)))
def test_grouped_backward_leaves_every_members_record(gi, sync, monkeypatch):
    """bn_group_bwd (modes 1 and 2) and bn_group_sync_bwd_reduce -> bn_group_sync_bwd_apply with `packed` passed straight through."""
    dev, K = _dev(), _k()
    _fresh_split_state(monkeypatch, K)
    shapes = GROUPS[gi]
    cs, _ = _group_conv_outputs(K, dev, shapes, 60 + gi)
    for mode, plant in GROUP_BWD:
        res = mode == 2
        case = _group_case(shapes, plant, 70 + gi, bwd=True)
        rs = [m["r"].to(dev) if res else None for m in case]
        gs = [m["g"].to(dev) for m in case]
        bns = _bn_modules(dev, shapes, case)
        ys, mis, _ = K.bn_group_fwd(cs, bns, rs, True)
        outs = ys if res else [None] * len(cs)
        if sync:
            packed, state = K.bn_group_sync_bwd_reduce(gs, cs, outs, mis, bns, mode)
            got = K.bn_group_sync_bwd_apply(state, packed)
        else:
            got = K.bn_group_bwd(gs, cs, outs, mis, bns, mode)
        for s, cv, m, g, bn, out, mi, (dx, _dw, _db, gm, am) in zip(shapes, cs, case, gs, bns, outs, mis, got):
            check_record(am, dx)
            ref = _reference(cv.cpu(), m["r"], m["g"], m["w"], m["b"], torch.zeros(s[1]), torch.ones(s[1]), True, res, True)[1]
            _close(dx, ref, 2e-5)
            if plant in ("first", "last"):
                assert _argmax(dx) == m["p"]
            elif plant == "neg":
                assert _argmax(dx) == m["p"] and float(dx.reshape(-1)[m["p"]]) < 0.0
            rec1 = K.amax_request(cv)
            w1, b1 = bn.weight.detach(), bn.bias.detach()
            if sync:
                sums, _, _, gm1 = K.bn_bwd_reduce(g, cv, out, mi, w1, b1, mode)
                dx1 = K.bn_bwd_apply(gm1 if mode == 2 else g, cv, mi, w1, b1, sums, 0.0, mode == 1, amax=rec1)
            else:
                dx1 = K.bn_bwd(g, cv, out, mi, w1, b1, mode, True, True, amax=rec1)[0]
            check_record(rec1, dx1)
            assert torch.equal(dx, dx1)
            _same_value(am, rec1)


# ---- 2. a consumer cannot tell the producer's record from a fresh one ---------------------------------------------------------------
TWO = 2.0
BELOW_TWO = float(torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)))


def _produce_by_bn_fwd(K, dev, shape, target, gen):
    """t = relu(bn(x) + r), max|t| == target exactly: everything else stays below 1.9 and the residual of one element is chosen so
    that the fp32 sum lands on the target."""
    C = shape[1]
    x = torch.randn(shape, generator=gen)
    w, b = (torch.randn(C, generator=gen) * 0.1).clamp(-0.2, 0.2), (torch.randn(C, generator=gen) * 0.05).clamp(-0.1, 0.1)
    r = (torch.randn(shape, generator=gen) * 0.3).clamp(-0.8, 0.8)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    plain = K.bn_fwd(xd, wd, bd, None, False, EPS, MOM, None, None, None)[0].cpu()           # the BatchNorm part, as the kernel rounds it
    assert float(plain.abs().max()) < 1.1
    cand = ((plain > 0.25) & (plain < 1.0)).reshape(-1).nonzero().reshape(-1)
    p = int(cand[len(cand) // 2])
    v = plain.reshape(-1)[p]
    r0 = torch.tensor(target, dtype=torch.float32) - v
    for k in range(-8, 9):
        rp = r0.clone()
        for _ in range(abs(k)):
            rp = torch.nextafter(rp, torch.tensor(4.0 if k > 0 else -4.0))
        if float(v + rp) == target:
            break
    else:
        raise AssertionError("no fp32 residual puts the sum on the target")
    r.view(-1)[p] = rp
    rec = K.amax_request(xd)
    t = K.bn_fwd(xd, wd, bd, r.to(dev), True, EPS, MOM, None, None, None, amax=rec)[0]
    return t, rec


def _produce_by_bn_bwd(K, dev, shape, target, gen):
    """t = dx of mode 2 with frozen statistics (dx = weight * invstd * masked dy: exact where both factors are 1)."""
    C = shape[1]
    n = shape[0] * C * shape[2] * shape[3]
    x, out = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    dy = (torch.randn(shape, generator=gen) * 0.25).clamp(-1.0, 1.0)
    w = torch.rand(C, generator=gen) * 2.0 - 1.0
    mi = torch.stack([torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5], dim=1).contiguous()
    p = n // 2 + 7
    c = (p // (shape[2] * shape[3])) % C
    w[c], mi[c, 1] = 1.0, 1.0
    out.view(-1)[p] = 1.0
    dy.view(-1)[p] = target
    xd = x.to(dev)
    rec = K.amax_request(xd)
    t = K.bn_bwd(dy.to(dev), xd, out.to(dev), mi.to(dev), w.to(dev), torch.zeros(C).to(dev), 2, False, True, amax=rec)[0]
    return t, rec


def _produce_by_affine(K, dev, shape, target, gen):
    C = shape[1]
    n = shape[0] * C * shape[2] * shape[3]
    u = (torch.randn(shape, generator=gen) * 0.4).clamp(-1.5, 1.5)
    a, b = (torch.rand(C, generator=gen) - 0.5) * 0.4, torch.rand(C, generator=gen) * 0.5 + 0.5
    p = n // 2 + 7
    c = (p // (shape[2] * shape[3])) % C
    a[c], b[c] = 0.0, 1.0
    u.view(-1)[p] = target
    return K.affine_channels(u.to(dev), a.to(dev), b.to(dev))


PRODUCERS = {"bn_fwd": _produce_by_bn_fwd, "bn_bwd": _produce_by_bn_bwd, "affine_channels": _produce_by_affine}


@pytest.mark.parametrize("target", [TWO, BELOW_TWO], ids=["2", "below2"])
@pytest.mark.parametrize("producer", sorted(PRODUCERS))
@pytest.mark.parametrize("shape", [(2, 48, 5, 64), (1, 64, 6, 33)])
def test_consumers_give_the_same_bits_with_the_producers_record(shape, producer, target, monkeypatch):
    """The split kernels depend on the record through its exponent only: forward, backward-data, weight gradient and the 1x1 kernel
    with the producer's record == with a separate cseg_amax_f32 pass, max|t| exactly at and one ulp below a power of two."""
    dev, K = _dev(), _k()
    _fresh_split_state(monkeypatch, K)
    C, P = shape[1], shape[2] * shape[3]
    if producer == "affine_channels" and P % 4:
        with pytest.raises(RuntimeError):              # (refused: see test_affine_channels_refuses_planes_that_are_no_multiple_of_four)
            _produce_by_affine(K, dev, shape, target, torch.Generator().manual_seed(1))
        return
    gen = torch.Generator().manual_seed(C + P)
    t, rec = PRODUCERS[producer](K, dev, shape, target, gen)
    assert float(t.abs().max()) == target
    check_record(rec, t)
    fresh = K.tensor_amax(t)
    check_record(fresh, t)
    w3 = (torch.randn(C, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)).to(dev)
    for flip in (False, True):
        assert torch.equal(K.conv3x3_sb_run(t, w3, flip, ax=rec), K.conv3x3_sb_run(t, w3, flip, ax=fresh)), flip
    xin = torch.randn(shape, generator=gen).to(dev)
    if K.conv3x3_sb_wrw_eligible(xin, t):
        ax = K.tensor_amax(xin)
        assert torch.equal(K.conv3x3_sb_wrw(xin, t, ax=ax, ady=rec), K.conv3x3_sb_wrw(xin, t, ax=ax, ady=fresh))
    if C == 64:
        w1 = (torch.randn(256, 64, 1, 1, generator=gen) / 8.0).to(dev)
        assert torch.equal(K.conv1x1_sb_run(t, w1, ax=rec), K.conv1x1_sb_run(t, w1, ax=fresh))


def _bn_output(K, dev, shape, seed, requires_grad=True):
    from contrastiveseg_amd.lib.models.tools.fused_bn import FusedBatchNorm2d
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=gen) * (1.0 + seed % 5)).to(dev).requires_grad_(requires_grad)
    m = FusedBatchNorm2d(shape[1]).to(dev).train()
    with torch.no_grad():
        m.weight.copy_(torch.randn(shape[1], generator=gen)); m.bias.copy_(torch.randn(shape[1], generator=gen))
    return m(x, relu=True)


def test_forwarded_records(monkeypatch):
    """fan_out hands every alias the SAME record object; conv1x1_split_skip hands the skip alias the record amax_of(x) left on x."""
    dev, K = _dev(), _k()
    _fresh_split_state(monkeypatch, K)
    y = _bn_output(K, dev, (2, 48, 5, 8), 3)
    rec = K.known_amax(y)
    check_record(rec, y)
    outs = K.fan_out(y, 3)
    assert len(outs) == 3 and all(o is not y for o in outs)
    for o in outs:
        assert K.known_amax(o) is rec
        check_record(K.known_amax(o), o)
    w = (torch.randn(256, 64, 1, 1, generator=torch.Generator().manual_seed(4)) / 8.0).to(dev)
    for x in (torch.randn(1, 64, 6, 33, generator=torch.Generator().manual_seed(5)).to(dev).requires_grad_(True),       # no record yet
              _bn_output(K, dev, (1, 64, 6, 33), 6)):                                                                   # a producer's record
        before = K.known_amax(x)
        y2, skip = K.conv1x1_split_skip(x, w)
        left = K.known_amax(x)
        assert left is not None and (before is None or left is before)
        assert skip is not x and K.known_amax(skip) is left
        check_record(K.known_amax(skip), skip)
        ref = F.conv2d(x.detach().double().cpu(), w.double().cpu())
        assert float((y2.detach().double().cpu() - ref).abs().max()) <= 4e-6 * float(ref.abs().max())


def test_an_in_place_edit_drops_the_record(monkeypatch):
    """The version guard: after y.mul_(4) the producer's record is gone, amax_of spends ONE pass and the next call none."""
    dev, K = _dev(), _k()
    from contrastiveseg_amd import _hip
    _fresh_split_state(monkeypatch, K)
    y = _bn_output(K, dev, (2, 48, 5, 64), 7, requires_grad=False)
    old = K.known_amax(y)
    check_record(old, y)
    with torch.no_grad():
        y.mul_(4.0)
    assert K.known_amax(y) is None
    passes = []
    orig = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (passes.append(name), orig(name, *a))[1])
    rec = K.amax_of(y)
    assert rec is not old
    check_record(rec, y)
    assert int(rec.max()) != int(old.max())
    assert K.amax_of(y) is rec and K.known_amax(y) is rec
    assert passes.count("cseg_amax_f32") == 1, passes
    w = (torch.randn(48, 48, 3, 3, generator=torch.Generator().manual_seed(8)) / 20.0).to(dev)
    assert torch.equal(K.conv3x3_sb_run(y, w), K.conv3x3_sb_run(y, w, ax=K.tensor_amax(y)))
    assert torch.equal(K.conv3x3_sb_run(y, w, ax=rec), K.conv3x3_sb_run(y, w))


def test_records_across_an_arena_switch(monkeypatch):
    """Arenas of four records: seven consecutive BatchNorm forwards take records from two arenas; every one describes its tensor, the
    earlier ones keep their values after the switch."""
    dev, K = _dev(), _k()
    monkeypatch.setattr(K, "AMAX_ARENA_RECORDS", 4)
    monkeypatch.setattr(K, "_AMAX_ARENAS", {})
    kept = []
    for i in range(7):
        y = _bn_output(K, dev, (2, 48, 5, 8) if i % 2 else (3, 5, 7, 9), 10 + i, requires_grad=False)
        rec = K.known_amax(y)
        check_record(rec, y)
        kept.append((y, rec, rec.clone()))
    assert len({r.data_ptr() for _, r, _ in kept}) == 7
    assert len({r.untyped_storage().data_ptr() for _, r, _ in kept}) >= 2, "the records all came from one arena"
    for y, rec, snap in kept:
        check_record(rec, y)
        assert torch.equal(rec, snap)


# ---- 3. the projection head's merged record ---------------------------------------------------------------------------------------
def test_projection_head_record_of_the_row_sparse_input_gradient(monkeypatch):
    """Row-sparse route of ProjectionHead (C = 48, P = 8 x 16, N = 24 anchor rows over B = 2): cseg_affine_channels sees du before
    _add_rows corrects N pixels, so the merged record may exceed max|du| but never fall below it, and it is bounded by the affine map:
    float(record) <= max(max|du|, M) * (1 + m). M = max |a_c + b_c u| in float64 over all pixels, with a_c and b_c the fp32 coefficients
    the kernel was GIVEN (the backward's fp64 coefficients are locals of the autograd node: any restatement from what the node returns
    -- d_gamma / d_beta, rounded to fp32 -- would bring a rounding of its own). With those the two conversion roundings are on both
    sides of the comparison and only the kernel's one fma rounding is left: m = 2^-24 = 6.0e-8 for every seed (< 2^-20)."""
    dev, K = _dev(), _k()
    from contrastiveseg_amd.lib.models.modules.projection import ProjectionHead
    _fresh_split_state(monkeypatch, K)
    monkeypatch.setattr(K, "SPARSE_EMBED_GRAD", True)
    B, C, H, W, D, N = 2, 48, 8, 16, 64, 24
    P = H * W
    torch.manual_seed(11)
    head = ProjectionHead(C, D, bn_type="torchbn").to(dev).train()
    gen = torch.Generator().manual_seed(3)
    feats = torch.randn(B, C, H, W, generator=gen).to(dev).requires_grad_(True)
    rows = torch.randn(N, D, generator=gen) * 0.1
    sel = torch.randperm(B * P, generator=gen)[:N].to(torch.int32)
    seen = {}
    affine = K.affine_channels

    def spy_affine(u, a, b, want_amax=True):
        seen["affine"] = (u, a, b)
        return affine(u, a, b, want_amax)
    monkeypatch.setattr(K, "affine_channels", spy_affine)
    run1, wrw1 = K.conv1x1_sb_run, K.conv1x1_sb_wrw

    def spy_run(x, weight, transpose=False, bias=None, ax=None, **kw):
        if transpose:
            seen["bwd_data"] = (x, weight, ax)
        return run1(x, weight, transpose, bias, ax=ax, **kw)

    def spy_wrw(x, dy, ax=None, ady=None):
        seen["wrw"] = (x, dy, ax, ady)
        return wrw1(x, dy, ax=ax, ady=ady)
    monkeypatch.setattr(K, "conv1x1_sb_run", spy_run)
    monkeypatch.setattr(K, "conv1x1_sb_wrw", spy_wrw)
    embed = head(feats)
    slot = embed._cseg_grad_slot
    embed.backward(slot.deposit(rows.to(dev), sel.to(dev), embed.shape))
    assert set(seen) == {"affine", "bwd_data", "wrw"}, sorted(seen)       # the row-sparse route, proj.0 on the split kernels
    du, w0, rec = seen["bwd_data"]
    assert seen["wrw"][1] is du and seen["wrw"][3] is rec and K.known_amax(du) is rec
    assert rec.dtype == torch.int32 and rec.numel() == K.AMAX_WORDS and not bool(rec.view(32, 32)[:, 1:].any())
    # lower bound: never below the tensor it describes
    assert _bits(du) <= int(rec.max())
    # upper bound
    u, a32, b32 = (t.detach().cpu().double() for t in seen["affine"])
    aff = a32.view(1, C, 1, 1) + b32.view(1, C, 1, 1) * u
    M = float(aff.abs().max())
    m = 2.0 ** -24
    assert m < 2.0 ** -20
    rec_f = float(rec.max().view(torch.float32))
    top = max(float(du.abs().max()), M)
    assert rec_f <= top * (1.0 + m), (rec_f, top, m)
    # the consumers: proj.0's backward-data and weight-gradient calls with this record against a fresh pass
    fresh = K.tensor_amax(du)
    same_exp = (int(rec.max()) >> 23) == (int(fresh.max()) >> 23)
    print("projection record: exponent %s the fresh one's" % ("equals" if same_exp else "is above"))
    x0, _, ax0, _ = seen["wrw"]
    got = (run1(du, w0, True, ax=rec), wrw1(x0, du, ax=ax0, ady=rec))
    if same_exp:
        assert torch.equal(got[0], run1(du, w0, True, ax=fresh)) and torch.equal(got[1], wrw1(x0, du, ax=ax0, ady=fresh))
    else:
        du64, w64, x64 = du.double().cpu(), w0.detach().double().cpu(), x0.detach().double().cpu()
        refs = (F.conv_transpose2d(du64, w64), torch.einsum("bohw,bihw->oi", du64, x64).view_as(w64))
        for g, ref, fan in zip(got, refs, (C, B * P)):
            assert float((g.double().cpu() - ref).abs().max()) <= 4e-6 * float(ref.abs().max()) * max(1.0, fan ** 0.5 / 8)


# ---- 4. a graph replay starts from zeroed records (GPU only) -----------------------------------------------------------------------
class _Toy(nn.Module):
    def __init__(self):
        super(_Toy, self).__init__()
        from contrastiveseg_amd.lib.models.tools.fused_bn import FusedBatchNorm2d
        from contrastiveseg_amd.lib.models.tools.module_helper import Conv3x3
        self.conv1, self.bn, self.conv2 = Conv3x3(48, 48), FusedBatchNorm2d(48, act="relu"), Conv3x3(48, 48)

    def forward(self, x, with_embed=False, is_eval=False):
        return {"seg": self.conv2(self.bn(self.conv1(x)))}


def test_graph_replay_starts_from_zeroed_records(monkeypatch):
    """Three forward + backward replays of one captured pair of graphs with the same weights: input A with output gradient G, then both
    scaled by 2^30, then A and G again. A record that survived the second replay (a running maximum over replays instead of the memset
    node inside the graph) would scale A by 2^-30 too little: fp16 subnormals, ~8 bits left. The third replay must equal the first bit
    for bit (fixed-order kernels) and stay within the convolution bound of the fp64 chain."""
    dev, K = _dev(), _k()
    if dev.type != "cuda":
        pytest.skip("hipGraph capture needs the GPU")
    from contrastiveseg_amd.segmentor.tools import step_graph
    _fresh_split_state(monkeypatch, K)
    monkeypatch.setattr(step_graph, "ENABLED", True)
    monkeypatch.setattr(step_graph, "MODE", "1")
    # what makes the test about records: both convolutions on the split kernels (they READ records) and BatchNorm handed real ones
    route = {"split": 0, "records": 0, "captured_split": 0, "captured_records": 0}
    split, request = K.conv3x3_split_bf16, K.amax_request

    def spy_split(*a, **k):
        route["split"] += 1
        route["captured_split"] += bool(torch.cuda.is_current_stream_capturing())
        return split(*a, **k)

    def spy_request(t):
        rec = request(t)
        route["records"] += rec is not None
        route["captured_records"] += rec is not None and bool(torch.cuda.is_current_stream_capturing())
        return rec
    monkeypatch.setattr(K, "conv3x3_split_bf16", spy_split)
    monkeypatch.setattr(K, "amax_request", spy_request)
    torch.manual_seed(21)
    net = _Toy().to(dev).train()
    step_graph.GraphedEncoder(net, max_rows=1)
    gen = torch.Generator().manual_seed(22)
    A = torch.randn(1, 48, 8, 64, generator=gen).to(dev)
    G = torch.randn(1, 48, 8, 64, generator=gen).to(dev)
    params = list(net.parameters())
    runs = []
    for scale in (1.0, 2.0 ** 30, 1.0):
        for p in params:
            p.grad = None
        out = net(A * scale)["seg"]
        out.backward(G * scale)
        torch.cuda.synchronize()
        runs.append((out.detach().clone(), [p.grad.detach().clone() for p in params]))
    g = net._cseg_step_graph
    assert g.failed is None and len(g.captured) == 1, g.failed
    # inside the capture: two split convolutions forward, and the records of the BatchNorm's y (forward) and dx (backward)
    assert route["captured_split"] == 2 and route["captured_records"] == 2, route
    assert torch.isfinite(runs[1][0]).all()
    assert torch.equal(runs[0][0], runs[2][0])
    for a, b in zip(runs[0][1], runs[2][1]):
        assert torch.equal(a, b)
    # the fp64 chain (batch statistics)
    ref = nn.Sequential(nn.Conv2d(48, 48, 3, 1, 1, bias=False), nn.BatchNorm2d(48), nn.ReLU(), nn.Conv2d(48, 48, 3, 1, 1, bias=False)).double()
    with torch.no_grad():
        ref[0].weight.copy_(net.conv1.weight); ref[3].weight.copy_(net.conv2.weight)
        ref[1].weight.copy_(net.bn.weight); ref[1].bias.copy_(net.bn.bias)
    y64 = ref(A.double().cpu())
    y64.backward(G.double().cpu())
    y64 = y64.detach()
    bound = lambda r: 4e-6 * float(r.abs().max()) * max(1.0, (9 * 48) ** 0.5 / 8)
    assert float((runs[2][0].double().cpu() - y64).abs().max()) <= bound(y64)
    # the parameter gradients at the same bound, with their own reduction length: sums over the B * H * W = 512 pixels
    errs = []
    for got, p64 in zip(runs[2][1], (ref[0].weight, ref[1].weight, ref[1].bias, ref[3].weight)):
        gscale = float(p64.grad.abs().max())
        errs.append((tuple(got.shape), float((got.double().cpu() - p64.grad).abs().max()) / gscale))
    print("graph replay: gradient errors relative to max|gradient|", errs, "bound %.2e" % (4e-6 * 512 ** 0.5 / 8))
    for shape, err in errs:
        assert err <= 4e-6 * max(1.0, 512 ** 0.5 / 8), (shape, err)
    # eager code after the capture gets arenas of its own again
    y = _bn_output(K, dev, (2, 48, 5, 8), 23, requires_grad=False)
    check_record(K.known_amax(y), y)
