"""Edge cases for the kernels behind the network: anchor mining (csrc/mining.hip), the memory-bank update (csrc/queue.hip), the
contrastive term (csrc/contrast.hip) and the fused upsample + cross entropy (csrc/upsample_ce.hip). A plain module (like
tests/exact_cases.py): seeded generators, references and runners that take the kernels module and a device; the MI355X files
(tests/test_gpu_mining_edges.py, test_gpu_queue_edges.py, test_gpu_loss_edges.py) and the emulated-device replay
(tests/test_emu_cabi.py) are thin users of it.

References are independent of the code under test: torch-CPU (F.interpolate nearest, torch.max, float64 cross entropy), plain
numpy in float64, and oracle/cseg_oracle.py (the restatement of the reference's loss that the golden vectors pin). Bars are the
project's existing ones where one exists; the two new ones (class sums, normalised bank rows) are operation counts, written as
formulas next to their derivation; the contrast-gradient bar is four times the worst error measured against the float64 oracle on
the emulator and on the MI355X."""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cseg_oracle as O

U = 2.0 ** -24               # unit roundoff of float32


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# =================================================================================================================================
# 1. classify / partition / gather / scatter
# =================================================================================================================================
# (B, K, h, w, H, W), ignore label
MINING_SHAPES = [
    ((1, 300, 5, 7, 11, 13), -1),        # 2K = 600 histogram slots > 256 threads; P = 35 inside wave 0
    ((2, 3, 82, 100, 82, 100), 255),     # P = 8200: chunk = 520, every wave makes a second sweep of 8 pixels; P % 8 == 0: 16-byte key loads
    ((2, 171, 13, 21, 97, 161), -1),     # P = 273, odd: scalar key loads; K = 171
    ((1, 4, 33, 55, 39, 65), 255),       # float32 legacy-nearest differs from integer arithmetic in 2 rows and 3 columns
    ((1, 1, 3, 3, 97, 161), -1),         # K = 1
]


def legacy_nearest_disagrees(n_in, n_out):
    """Destination indices where float32 floor(dst * float(in) / float(out)) differs from dst * in // out."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out)
    f = np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), n_in - 1)
    return np.nonzero(f != dst * n_in // n_out)[0]


@functools.lru_cache(maxsize=None)
def mining_case(i):
    """target int64 [B,H,W], seg float32 [B,K,h,w] with the plants of the issue, and the references (computed once, shared)."""
    (B, K, h, w, H, W), ign = MINING_SHAPES[i]
    rs = np.random.RandomState(100 + i)
    target = rs.randint(0, K, size=(B, H, W)).astype(np.int64)
    target[rs.rand(B, H, W) < 0.15] = ign
    # labels that are neither the ignore label nor a class: >= K and < 0
    bad = rs.rand(B, H, W)
    target[bad < 0.03] = K
    target[(bad >= 0.03) & (bad < 0.05)] = K + 1000
    target[(bad >= 0.05) & (bad < 0.07)] = -7
    if ign != -1:
        target[(bad >= 0.07) & (bad < 0.09)] = -1
    iy, ix = O.nearest_src_index(h, H), O.nearest_src_index(w, W)      # ... and one of each kind where the downsampling looks
    target[0, iy[1], ix[0]] = K + 1000
    target[0, iy[0], ix[1]] = -7
    seg = (rs.standard_normal((B, K, h, w)) * 2).astype(np.float32)
    if B == 2:
        if K == 3:
            target[1] = ign                                  # an image that is entirely ignored: all counts 0, seg_off still written
        else:
            target[1] = 5                                    # one class only, all hard: its own logit is the smallest
            seg[1, 5] = -50.0
    # logit plants, at distinct pixels of image 0 (first row and last row of the map)
    px = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]
    seg[0, :, px[0][0], px[0][1]] = 0.25                     # equal logits in all classes: pred 0
    seg[0, :, px[3][0], px[3][1]] = -np.inf                  # all -inf: pred 0
    seg[0, K - 1, px[4][0], px[4][1]] = np.inf               # one +inf: that class
    expect = {px[0]: 0, px[3]: 0, px[4]: K - 1}
    if K >= 4:
        seg[0, 2, px[1][0], px[1][1]] = np.nan               # NaN in class 2, a larger number in class 3: pred 2
        seg[0, 3, px[1][0], px[1][1]] = 1e30
        seg[0, 1, px[2][0], px[2][1]] = np.nan               # two NaNs: the first wins
        seg[0, 3, px[2][0], px[2][1]] = np.nan
        expect.update({px[1]: 2, px[2]: 1})
    else:
        seg[0, K - 1, px[1][0], px[1][1]] = np.nan           # K < 4: a NaN in the last class
        expect[px[1]] = K - 1
    # references: torch-CPU
    lab = F.interpolate(torch.from_numpy(target).float().unsqueeze(1), (h, w), mode="nearest").squeeze(1).long().numpy().reshape(B, -1)
    pred = torch.max(torch.from_numpy(seg), 1)[1].numpy().reshape(B, -1)
    for (y, x), k in expect.items():
        assert pred[0, y * w + x] == k, "torch.max no longer does what the plant was built for"
    assert np.array_equal(lab, O.nearest_downsample_labels(target, h, w).reshape(B, -1))
    return dict(shape=(B, K, h, w, H, W), ignore=ign, target=target, seg=seg, lab=lab, pred=pred)


def check_partition(cp, c, with_maps=True):
    B, K, h, w, H, W = c["shape"]
    lab, pred, ign = c["lab"], c["pred"], c["ignore"]
    if with_maps:
        assert np.array_equal(cp["lab"].cpu().numpy(), lab), "nearest-downsampled labels"
        assert np.array_equal(cp["pred"].cpu().numpy(), pred), "argmax"
    counts, seg_off, part = cp["counts"].cpu().numpy(), cp["seg_off"].cpu().numpy(), cp["part_idx"].cpu().numpy()
    n_bad = int(((lab != ign) & ((lab < 0) | (lab >= K))).sum())
    assert int(cp["status"].cpu().numpy()[0]) == n_bad, "out-of-range label counter"
    for b in range(B):
        off = 0
        for cls in range(K):
            hard = np.nonzero((lab[b] == cls) & (pred[b] != cls))[0]
            easy = np.nonzero((lab[b] == cls) & (pred[b] == cls))[0]
            assert counts[b, cls, 0] == len(hard) and counts[b, cls, 1] == len(easy), (b, cls)
            assert seg_off[b, cls, 0] == off, (b, cls)
            assert np.array_equal(part[b, off:off + len(hard)], hard), (b, cls, "hard")
            off += len(hard)
            assert seg_off[b, cls, 1] == off, (b, cls)
            assert np.array_equal(part[b, off:off + len(easy)], easy), (b, cls, "easy")
            off += len(easy)
    return n_bad


def run_classify_partition(Kk, dev, i):
    c = mining_case(i)
    B, K, h, w, H, W = c["shape"]
    lab, ign = c["lab"], c["ignore"]
    # the case holds what it was built for
    n_bad = int(((lab != ign) & ((lab < 0) | (lab >= K))).sum())
    assert n_bad > 0 and ((lab < 0) & (lab != ign)).any() and (lab >= K).any()
    if (h, w) == (33, 55):
        # the one shape of the suite where float32 floor(dst * float(in) / float(out)) and dst * in // out part ways (2 rows, 3 columns),
        # and the labels there differ, so a kernel on integer arithmetic fails
        assert len(legacy_nearest_disagrees(H, h)) == 2 and len(legacy_nearest_disagrees(W, w)) == 3
        as_int = c["target"][:, np.arange(h) * H // h][:, :, np.arange(w) * W // w].reshape(B, -1)
        assert (as_int != lab).sum() > 20
    if B == 2:
        valid1 = lab[1][(lab[1] >= 0) & (lab[1] < K) & (lab[1] != ign)]
        assert (valid1.size == 0) if K == 3 else (set(valid1) == {5} and (c["pred"][1] != 5).all())
    target = _t(c["target"], dev)
    cp = Kk.classify_partition(target, ign, seg=_t(c["seg"], dev), want_maps=True)
    check_partition(cp, c)
    cp2 = Kk.classify_partition(target, ign, predict=_t(c["pred"].reshape(B, h, w).astype(np.int64), dev), num_classes=K,
                                feat_hw=(h, w), want_maps=True)
    check_partition(cp2, c)


GATHER_D = (8, 24, 64, 72, 256)
GATHER_N = (1, 5, 130)          # 4 rows per block: one partly filled block, two blocks, 33 blocks with a ragged last one


def gather_case(D, N):
    rs = np.random.RandomState(D * 1000 + N)
    B, h, w = 3, 6, 11
    P = h * w
    embed = rs.standard_normal((B, D, h, w)).astype(np.float32)
    part_idx = np.stack([rs.permutation(P) for _ in range(B)]).astype(np.int32)
    sel_pos = rs.permutation(B * P)[:N].astype(np.int32)       # no duplicates (selection without replacement), non-monotone
    if N > 1:
        assert len(set(sel_pos // P)) > 1 and (np.diff(sel_pos) < 0).any()
    b = sel_pos // P
    pix = part_idx.reshape(-1)[sel_pos]
    return embed, part_idx, sel_pos, b, pix


def run_gather(Kk, dev, D, N):
    embed, part_idx, sel_pos, b, pix = gather_case(D, N)
    B, _, h, w = embed.shape
    P = h * w
    want = torch.from_numpy(embed.reshape(B, D, P)[b, :, pix])                 # [N, D]
    want_pix = torch.from_numpy((b * P + pix).astype(np.int32))
    e = _t(embed, dev).requires_grad_(True)
    anchors, sel_pix = Kk.gather_anchors(e.detach(), _t(part_idx, dev), _t(sel_pos, dev))
    assert torch.equal(anchors.cpu(), want) and torch.equal(sel_pix.cpu(), want_pix)
    anchors, sel_pix = Kk.GatherAnchors.apply(e, _t(part_idx, dev), _t(sel_pos, dev))
    assert torch.equal(anchors.detach().cpu(), want) and torch.equal(sel_pix.cpu(), want_pix)
    # its backward is the scatter with one part and scale 1: the rows land where they came from, +0 everywhere else
    g = np.random.RandomState(N).standard_normal((N, D)).astype(np.float32)
    anchors.backward(_t(g, dev))
    ref = np.zeros((B, D, P), dtype=np.float32)
    ref[b, :, pix] = g
    assert np.array_equal(e.grad.cpu().numpy().reshape(B, D, P).view(np.int32), ref.view(np.int32))


def run_scatter(Kk, dev, n_parts, scale):
    """cseg_scatter_anchor_grad called as PixelContrast.backward calls it, against np.float32 arithmetic in the kernel's order:
    parts added in index order starting from 0.f, then ONE multiply."""
    from contrastiveseg_amd import _hip
    rs = np.random.RandomState(7 + n_parts)
    B, D, h, w, N = 2, 72, 5, 7, 37
    P = h * w
    parts = rs.standard_normal((n_parts, N, D)).astype(np.float32)
    sel = rs.permutation(B * P)[:N].astype(np.int32)
    d_embed = torch.zeros(B, D, h, w, dtype=torch.float32, device=dev)
    p_d, s_d = _t(parts, dev), _t(sel, dev)
    _hip.call("cseg_scatter_anchor_grad", _hip.dev(p_d, torch.float32, "parts"), n_parts, _hip.dev(s_d, torch.int32, "sel_pix"), N, D, P,
              float(scale), _hip.dev(d_embed, torch.float32, "d_embed"), _hip.stream_ptr())
    acc = np.zeros((N, D), dtype=np.float32)
    for s in range(n_parts):
        acc = acc + parts[s]
    rows = acc * np.float32(scale)
    assert rows.dtype == np.float32
    ref = np.zeros((B, D, P), dtype=np.float32)
    ref[sel // P, :, sel % P] = rows
    got = d_embed.cpu().numpy().reshape(B, D, P)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), np.abs(got - ref).max()     # bit for bit, +0 where nothing landed


# =================================================================================================================================
# 2. memory bank
# =================================================================================================================================
# (B, K, H, W, stride, D, kh, kw): the first four are the issue's; the rest bring K in {19, 32, 64, 300} and D = 256
BANK_SHAPES = [
    (2, 171, 37, 50, 3, 24, 13, 17),     # Q = 221 = Pk, six class chunks, the last one partial (171 = 5 * 32 + 11)
    (1, 33, 16, 24, 8, 8, 4, 6),         # Q = 6 < 64, Pk = 24 > Q: keys at stride 4 indexed with positions of the stride-8 label map
    (2, 65, 20, 20, 1, 30, 20, 20),      # D = 30: two waves of the last block idle; K = 65: one class in the third chunk
    (1, 1, 9, 9, 2, 8, 5, 5),            # K = 1
    (1, 19, 17, 23, 3, 256, 6, 8),       # D = 256; Q = 48 < 64
    (1, 32, 21, 30, 8, 8, 6, 8),         # K = 32: exactly one chunk; Q = 12, Pk = 48 > Q
    (1, 64, 33, 35, 3, 8, 11, 12),       # K = 64: exactly two chunks; Q = 132
    (1, 300, 37, 50, 3, 8, 13, 17),      # K = 300 > 256: the i += 256 loop of queue_count_kernel
]


@functools.lru_cache(maxsize=None)
def bank_case(i):
    B, K, H, W, stride, D, kh, kw = BANK_SHAPES[i]
    rs = np.random.RandomState(200 + i)
    Hs, Ws = -(-H // stride), -(-W // stride)
    assert Hs * Ws <= kh * kw
    labels = rs.randint(0, K, size=(B, H, W)).astype(np.int64)
    r = rs.rand(B, H, W)
    labels[r < 0.06] = -1
    labels[(r >= 0.06) & (r < 0.12)] = 255
    labels[(r >= 0.12) & (r < 0.16)] = K
    labels[(r >= 0.16) & (r < 0.20)] = K + 1000
    if K > 1:                                                # a class that occurs once in the strided map of image 0
        once = K - 1
        s0 = labels[0, ::stride, ::stride]
        s0[s0 == once] = 0
        s0[Hs // 2, Ws // 2] = once
    keys = (rs.standard_normal((B, D, kh, kw)) * 3).astype(np.float32)
    sl = labels[:, ::stride, ::stride].reshape(B, -1)
    Q = sl.shape[1]
    assert Q == Hs * Ws
    counts = np.zeros((B, K), dtype=np.int64)
    sums = np.zeros((B, K, D))
    mass = np.zeros((B, K, D))
    k64 = keys.astype(np.float64).reshape(B, D, -1)
    for b in range(B):
        for c in range(K):
            idx = np.nonzero(sl[b] == c)[0]
            counts[b, c] = len(idx)
            sums[b, c] = k64[b][:, idx].sum(axis=1)
            mass[b, c] = np.abs(k64[b][:, idx]).sum(axis=1)
    if K > 1:
        assert counts[0, K - 1] == 1
    return dict(labels=labels, keys=keys, counts=counts, sums=sums, mass=mass, Q=Q)


def run_bank_count_and_sums(Kk, dev, i):
    B, K, H, W, stride, D, kh, kw = BANK_SHAPES[i]
    c = bank_case(i)
    labels = _t(c["labels"], dev)
    counts = Kk.queue_count(labels, stride, K).cpu().numpy()
    assert np.array_equal(counts, c["counts"])
    sums = Kk.queue_class_sums(_t(c["keys"], dev), labels, stride, K).cpu().numpy().astype(np.float64)
    # Every lane adds at most ceil(Q / 64) terms in order (a term of another class adds an exact 0.f) and the wave reduction adds 6
    # levels, so every value passes through at most n = ceil(Q / 64) + 6 rounded additions: |err| <= gamma_n * sum|v| over the class's
    # pixels, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2). A class
    # without pixels has sum|v| = 0: its sums are exactly 0.
    n = math.ceil(c["Q"] / 64) + 6
    gamma = n * U / (1 - n * U)
    err = np.abs(sums - c["sums"])
    assert (err <= gamma * c["mass"]).all(), float((err - gamma * c["mass"]).max())


BANK_WRITE_D = (8, 64, 300)        # 300 exceeds both the 256-thread stride (segments) and the 64-lane stride (pixels)


def _pattern(K, ms, D):
    """A recognisable fill for a bank: no two elements alike, none of them a value a normalised row could leave behind."""
    return (np.arange(K * ms * D, dtype=np.float32).reshape(K, ms, D) + 1000.0) * np.float32(-1.0)


def _row_bar(D):
    # mean (1 / count and one multiply: 2 roundings), sum of squares (a square, then at most ceil(D / 64) additions per lane, 6 wave levels and
    # 3 wave partials: ceil(D / 64) + 10 roundings, halved by the square root, which adds 1), one division: at most ceil(D / 64) + 12
    # roundings of 2^-24 relative each on components of magnitude at most 1.
    return (math.ceil(D / 64) + 12) * U


def _l2n64(x):
    x = x.astype(np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=-1, keepdims=True)), 1e-12)


def run_bank_write_segments(Kk, dev, D):
    rs = np.random.RandomState(300 + D)
    B, K, ms = 2, 5, 4
    sums = (rs.standard_normal((B, K, D)) * 20).astype(np.float32)
    counts = rs.randint(1, 60, size=(B, K)).astype(np.int32)
    jobs = np.array([(0, 1, 0), (1, 1, 3), (0, 4, 3), (1, 2, 1), (0, 3, 2), (1, 0, 2)], dtype=np.int32)     # (image, class, row); row ms - 1 twice
    sums[1, 2] = 0.0                                         # a class sum that is exactly zero: a row of zeros, not NaN
    segq0 = _pattern(K, ms, D)
    segq = _t(segq0, dev)
    v0 = segq._version
    Kk.queue_write_segments(_t(sums, dev), _t(counts, dev), _t(jobs[:, 0], dev), _t(jobs[:, 1], dev), _t(jobs[:, 2], dev), segq)
    assert segq._version > v0
    got = segq.cpu().numpy()
    named = np.zeros((K, ms), dtype=bool)
    for b, c, row in jobs:
        named[c, row] = True
        want = _l2n64(sums[b, c].astype(np.float64) / float(counts[b, c]))
        assert np.abs(got[c, row] - want).max() <= _row_bar(D), (b, c, row, np.abs(got[c, row] - want).max())
    assert not got[2, 1].any() and not np.signbit(got[2, 1]).any()
    assert np.array_equal(got[~named].view(np.int32), segq0[~named].view(np.int32)), "a row no job names was touched"


def run_bank_write_pixels(Kk, dev, D):
    rs = np.random.RandomState(400 + D)
    B, K, ms, kh, kw = 2, 5, 4, 5, 7
    Pk = kh * kw
    keys = (rs.standard_normal((B, D, kh, kw)) * 3).astype(np.float32)
    rows = np.array([(0, 0, 1, 0), (1, 34, 1, 3), (0, 17, 4, 3), (1, 5, 2, 1), (0, 33, 3, 2), (1, 20, 0, 0), (0, 9, 4, 0)],
                    dtype=np.int32)                          # (image, position, class, row): 7 rows = two blocks, the second ragged
    keys.reshape(B, D, Pk)[1, :, 5] = 0.0                    # a source pixel that is exactly zero
    pixq0 = _pattern(K, ms, D)
    pixq = _t(pixq0, dev)
    v0 = pixq._version
    Kk.queue_write_pixels(_t(keys, dev), _t(rows[:, 0], dev), _t(rows[:, 1], dev), _t(rows[:, 2], dev), _t(rows[:, 3], dev), pixq)
    assert pixq._version > v0
    got = pixq.cpu().numpy()
    named = np.zeros((K, ms), dtype=bool)
    for b, pos, c, row in rows:
        named[c, row] = True
        want = _l2n64(keys.reshape(B, D, Pk)[b, :, pos])
        assert np.abs(got[c, row] - want).max() <= _row_bar(D), (b, pos, c, row, np.abs(got[c, row] - want).max())
    assert not got[2, 1].any() and not np.signbit(got[2, 1]).any()
    assert np.array_equal(got[~named].view(np.int32), pixq0[~named].view(np.int32)), "a row no job names was touched"


ENQ_WIDE = dict(K=171, B=2, H=40, W=56, network_stride=8, key_stride=4, D=16, memory_size=6, pixel_update_freq=4, rounds=3, seed=1234)


def enq_wide_inputs(r):
    """Round r of the enqueue at the coco_stuff bank shape: about 60 classes in the 2 x 35 positions of the stride-8 label map, among
    them 31 / 32 / 33 (both sides of the first chunk edge of queue_class_sums_kernel), 160 (the last full chunk's first class) and 170
    (the last class). Classes 31, 33 and 170 sit in both images every round, so their segment pointers wrap at memory_size 6 in round 3;
    class 32 has five pixels in image 0, so its pixel pointer takes the `ptr + k >= memory_size` branch."""
    c = ENQ_WIDE
    rs = np.random.RandomState(c["seed"] + r)
    Hs, Ws = c["H"] // c["network_stride"], c["W"] // c["network_stride"]
    labels = rs.randint(0, c["K"], size=(c["B"], c["H"], c["W"])).astype(np.int64)       # what the stride skips: anything
    for b in range(c["B"]):
        pool = [k for k in rs.permutation(np.arange(1, c["K"])) if k not in (31, 32, 33, 160, 170)]
        s = np.array(pool[:Hs * Ws], dtype=np.int64)
        s[:3] = (31, 33, 170)
        if b == 0:
            s[3:8] = 32
            s[8] = 160
        s[9:12] = (0, -1, -1 if b else 0)                    # class 0 and the ignore label are never enqueued (the reference indexes the
                                                             # bank with any other label, so labels >= K are left to the kernel tests)
        labels[b, ::c["network_stride"], ::c["network_stride"]] = rs.permutation(s).reshape(Hs, Ws)
    keys = rs.standard_normal((c["B"], c["D"], c["H"] // c["key_stride"], c["W"] // c["key_stride"])).astype(np.float32)
    return labels, keys


def run_enqueue_wide(Kk, dev):
    """Trainer._dequeue_and_enqueue against O.dequeue_and_enqueue. The random draws are paired the direct way: torch.manual_seed(seed)
    on the product side, O.TorchCpuRng(seed) on the oracle's -- no recorded permutations."""
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    c = ENQ_WIDE
    K, ms, D = c["K"], c["memory_size"], c["D"]
    me = Trainer.__new__(Trainer)
    me.network_stride, me.memory_size, me.pixel_update_freq = c["network_stride"], ms, c["pixel_update_freq"]
    rs = np.random.RandomState(c["seed"] - 1)
    sq0 = _l2n64(rs.standard_normal((K, ms, D))).astype(np.float32)
    pq0 = _l2n64(rs.standard_normal((K, ms, D))).astype(np.float32)
    sq, pq = _t(sq0, dev), _t(pq0, dev)
    sp = torch.zeros(K, dtype=torch.long, device=dev)
    pp = torch.zeros(K, dtype=torch.long, device=dev)
    o_sq, o_pq = sq0.astype(np.float64), pq0.astype(np.float64)
    o_sp, o_pp = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    rng = O.TorchCpuRng(c["seed"])
    torch.manual_seed(c["seed"])
    wrapped_seg, wrapped_pix = False, False
    for r in range(c["rounds"]):
        labels, keys = enq_wide_inputs(r)
        before = o_sp.copy(), o_pp.copy()
        O.dequeue_and_enqueue(keys, labels, o_sq, o_sp, o_pq, o_pp, c["network_stride"], ms, c["pixel_update_freq"], rng)
        wrapped_seg |= bool(((o_sp < before[0])).any())
        wrapped_pix |= bool(((o_pp < before[1])).any())
        sl = labels[:, ::c["network_stride"], ::c["network_stride"]]
        present = set(int(v) for v in np.unique(sl) if 0 < v < K)
        assert {31, 32, 33, 160, 170} <= present and len(present) >= 50, len(present)
        me._dequeue_and_enqueue(_t(keys, dev), _t(labels, dev), sq, sp, pq, pp)
        assert np.array_equal(sp.cpu().numpy(), o_sp), r
        assert np.array_equal(pp.cpu().numpy(), o_pp), r
        assert np.allclose(sq.cpu().numpy(), o_sq, rtol=1e-5, atol=1e-6), (r, np.abs(sq.cpu().numpy() - o_sq).max())
        assert np.allclose(pq.cpu().numpy(), o_pq, rtol=1e-5, atol=1e-6), (r, np.abs(pq.cpu().numpy() - o_pq).max())
    assert wrapped_seg and wrapped_pix


# =================================================================================================================================
# 3. contrastive term
# =================================================================================================================================
LOSS_TOL = 2e-5              # relative to max(1, |ref|): the bar of tests/test_gpu_kernels.py
# Worst |gradient - float64 oracle| over max|oracle gradient| of a case, over all cases below and both forward forms, as measured:
# 1.319e-5 on the emulator and 1.713e-5 on the MI355X (both in plain_pos128; the table is in DESIGN.md section 17). The bar is four times
# the larger of the two, which leaves room for another legal summation order, and never looser than the 2e-3 of tests/test_gpu_kernels.py.
CONTRAST_GRAD_SEEN = {"emu": 1.319e-5, "mi355x": 1.713e-5}
CONTRAST_GRAD_BAR = min(2e-3, 4 * max(CONTRAST_GRAD_SEEN.values()))

# name -> (mode, sizes, construction)
CONTRAST_CASES = {
    "plain_neg130": ("plain", (40, 90, 16), dict(gain=(-3.0, 3.0), tau=0.07)),       # every logit ~ -110 .. -160; M ragged in the last 64-tile and 32-group
    "plain_neg130_grid1": ("plain", (40, 90, 16), dict(gain=(-3.0, 3.0), tau=0.07, grid=1)),
    "plain_pos57": ("plain", (70, 150, 32), dict(gain=(2.0, 2.0), tau=0.07)),        # +2 on both sides
    "plain_pos128": ("plain", (70, 150, 32), dict(gain=(3.0, 3.0), tau=0.07)),       # +3: exp(128) overflows float32 without the max
    "plain_33": ("plain", (33, 33, 8), dict(gain=None, tau=0.07)),                   # N = M, one row past the 32-tile edge
    "bank_tail_max": ("bank", (40, 4, 5, 24), dict(tau=0.07)),                       # the zero tail holds the row maximum
    "self_2": ("self", (2, 8), dict(tau=0.1)),
    "self_33_singleton": ("self", (33, 16), dict(tau=0.1)),
}


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def zlib_seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def contrast_case(name):
    """Inputs in float32 and the float64 oracle's loss and anchor gradient (computed once, shared by both forward forms)."""
    mode, sizes, how = CONTRAST_CASES[name]
    rs = np.random.RandomState(zlib_seed(name.replace("_grid1", "")))      # (the grid-1 form runs on the same inputs)
    tau, base = how["tau"], 0.07
    c = dict(mode=mode, tau=tau, base=base, grid=how.get("grid"))
    if mode == "plain":
        N, M, D = sizes
        if how["gain"] is None:
            A, C = _unit(rs.standard_normal((N, D))), _unit(rs.standard_normal((M, D)))
        else:
            u = _unit(rs.standard_normal(D))
            A = how["gain"][0] * (u + 0.05 * rs.standard_normal((N, D)))
            C = how["gain"][1] * (u + 0.05 * rs.standard_normal((M, D)))
        A, C = A.astype(np.float32), C.astype(np.float32)
        ya, yc = rs.randint(0, 4, size=N), rs.randint(0, 4, size=M)
        loss, G = O._contrast_core(A.astype(np.float64), ya, C.astype(np.float64), yc, tau, base, True)
        c.update(A=A, ya=ya, C=C, yc=yc, loss=loss, grad=G @ C.astype(np.float64) / tau)
    elif mode == "bank":
        N, K, ms, D = sizes
        u = _unit(rs.standard_normal(D))
        sq = _unit(u + 0.05 * rs.standard_normal((K, ms, D))).astype(np.float32)
        pq = _unit(u + 0.05 * rs.standard_normal((K, ms, D))).astype(np.float32)
        A = (-3.0 * _unit(u + 0.05 * rs.standard_normal((N, D)))).astype(np.float32)          # norm 3, anti-aligned with the bank
        ya = rs.randint(0, K, size=N)
        ya[[0, 31, 35]] = 0                  # class 0: positives in the zero tail; rows 31 and 35 are tail columns themselves (self mask)
        queue = np.concatenate([sq, pq], axis=1)
        loss, dA = O.contrastive_mem(A.reshape(N, 1, D), ya, queue, tau, base, return_grad=True)
        S = A.astype(np.float64) @ O.sample_negative(queue)[0].T / tau
        assert (S[:, :(K - 1) * 2 * ms] < -30).all() and (S.max(axis=1) == 0).all()
        c.update(A=A, ya=ya, sq=sq, pq=pq, loss=loss, grad=dA.reshape(N, D))
    else:
        N, D = sizes
        A = _unit(rs.standard_normal((N, D))).astype(np.float32)
        ya = np.zeros(N, dtype=np.int64) if N == 2 else rs.randint(0, 3, size=N)
        if N > 2:
            ya[7] = 97                       # a class of its own: no positives, 0 / 0
        A64 = A.astype(np.float64)
        loss, G = O._contrast_core(A64, ya, A64, ya, tau, base, True)
        c.update(A=A, ya=ya, loss=loss, grad=(G + G.T) @ A64 / tau)
    return c


def run_contrast(Kk, dev, name, fused, monkeypatch):
    """Loss and anchor gradient of kernels.ContrastOnAnchors against the float64 oracle. Returns the gradient error ratio."""
    c = contrast_case(name)
    monkeypatch.setattr(Kk, "CONTRAST_FUSED", fused)
    if c["grid"] is not None:
        monkeypatch.setenv("CSEG_CONTRAST_FUSED_GRID", str(c["grid"]))
    A = _t(c["A"], dev).requires_grad_(True)
    lab = _t(c["ya"].astype(np.int32), dev)
    args = [None, None, None, None]
    if c["mode"] == "plain":
        args[:2] = [_t(c["C"], dev), _t(c["yc"].astype(np.int32), dev)]
    elif c["mode"] == "bank":
        args[2:] = [_t(c["sq"], dev), _t(c["pq"], dev)]
    loss = Kk.ContrastOnAnchors.apply(A, lab, c["mode"], c["tau"], c["base"], *args)
    loss.backward()
    got_loss, got = float(loss.detach()), A.grad.cpu().numpy().astype(np.float64)
    ref_loss, ref = float(c["loss"]), c["grad"]
    if name == "self_33_singleton":
        assert np.isnan(ref_loss) and np.isnan(got_loss) and np.isnan(ref[7]).all() and np.isnan(got[7]).all()
    else:
        assert np.isfinite(ref_loss) and np.isfinite(ref).all()
        assert abs(got_loss - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss)), (got_loss, ref_loss)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN masks of the gradient differ"
    ok = ~np.isnan(ref)
    if not ok.any():
        print("contrast %s fused=%s: loss %r / %r, gradient all NaN in both" % (name, fused, got_loss, ref_loss))
        return 0.0
    scale = np.abs(ref[ok]).max()
    err = np.abs(got[ok] - ref[ok]).max()
    ratio = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
    print("contrast %s fused=%s: loss %.9g / %.9g, gradient max|err| %.3e, max|ref| %.3e, ratio %.3e" % (name, fused, got_loss, ref_loss, err, scale, ratio))
    assert ratio <= CONTRAST_GRAD_BAR, (name, fused, ratio)
    return ratio


CONTRAST_REFUSALS = ("d12", "n_gt_m", "tau0")


def run_contrast_refusal(Kk, dev, what, fused, monkeypatch):
    """Host-side CSEG_REQUIRE of make_col: a RuntimeError before any launch."""
    import pytest
    monkeypatch.setattr(Kk, "CONTRAST_FUSED", fused)
    rs = np.random.RandomState(3)
    N, M, D, tau = {"d12": (5, 9, 12, 0.1), "n_gt_m": (9, 5, 8, 0.1), "tau0": (5, 9, 8, 0.0)}[what]
    A = _t(_unit(rs.standard_normal((N, D))).astype(np.float32), dev)
    C = _t(_unit(rs.standard_normal((M, D))).astype(np.float32), dev)
    ya, yc = _t(rs.randint(0, 2, size=N).astype(np.int32), dev), _t(rs.randint(0, 2, size=M).astype(np.int32), dev)
    with pytest.raises(RuntimeError):
        Kk.ContrastOnAnchors.apply(A, ya, "plain", tau, 0.07, C, yc, None, None)


# =================================================================================================================================
# 4. fused upsample + cross entropy
# =================================================================================================================================
# name -> ((B, K, h, w, H, W), variant)
CE_CASES = {
    "h1": ((1, 5, 1, 6, 4, 21), "plain"),                    # h = 1: the vertical align-corners scale is 0
    "w1": ((2, 4, 6, 1, 20, 1), "weighted"),                 # w = W = 1
    "cell17": ((1, 2, 2, 2, 17, 17), "plain"),               # 16 + 1 pixels per cell: exactly MAX_PX
    "x200": ((1, 3, 4, 5, 9, 11), "x200"),                   # logits x 200: loss ~ 136, overflow without the max subtraction
    "weight0_row": ((1, 6, 5, 6, 17, 23), "weight0_row"),    # a class of weight 0 that is the only class in one row
    "bad_labels": ((1, 6, 5, 6, 17, 23), "bad_labels"),      # 5 labels == K and 3 == -7
    "all_ignored": ((1, 6, 5, 6, 17, 23), "all_ignored"),
}
CE_IGNORE = -1


@functools.lru_cache(maxsize=None)
def ce_case(name):
    (B, K, h, w, H, W), variant = CE_CASES[name]
    rs = np.random.RandomState(zlib_seed(name))
    seg = (rs.standard_normal((B, K, h, w)) * 3).astype(np.float32)
    target = rs.randint(-1, K, size=(B, H, W)).astype(np.int64)
    weight, n_bad = None, 0
    if variant == "x200":
        seg = (seg * 200).astype(np.float32)
    if variant in ("weighted", "weight0_row", "bad_labels"):
        weight = (rs.rand(K) + 0.5).astype(np.float32)
    if variant == "weight0_row":
        weight[2] = 0.0
        target[0, 4, :] = 2
    clean = target.copy()
    if variant == "bad_labels":
        flat = rs.permutation(B * H * W)[:8]
        target.reshape(-1)[flat[:5]] = K
        target.reshape(-1)[flat[5:]] = -7
        clean = target.copy()
        clean.reshape(-1)[flat] = CE_IGNORE                  # the reference: those pixels ignored
        n_bad = 8
    if variant == "all_ignored":
        target[:] = CE_IGNORE
        clean = target.copy()
    # torch-CPU float64
    s64 = torch.from_numpy(seg).double().requires_grad_(True)
    up = F.interpolate(s64, size=(H, W), mode="bilinear", align_corners=True)
    ref = F.cross_entropy(up, torch.from_numpy(clean), weight=None if weight is None else torch.from_numpy(weight).double(), ignore_index=CE_IGNORE)
    (g_ref,) = torch.autograd.grad(ref * 1.7, s64)
    with np.errstate(invalid="ignore", divide="ignore"):
        oracle = O.upsample_ce(seg, clean, weight, CE_IGNORE)
    return dict(seg=seg, target=target, weight=weight, n_bad=n_bad, ref=float(ref.detach()), g_ref=g_ref.numpy() / 1.7, oracle=float(oracle))


def run_upsample_ce(Kk, dev, name):
    c = ce_case(name)
    seg = _t(c["seg"], dev).requires_grad_(True)
    wt = None if c["weight"] is None else _t(c["weight"], dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    loss = Kk.upsample_ce(seg, _t(c["target"], dev), wt, CE_IGNORE, status=status)
    (g,) = torch.autograd.grad(loss * 1.7, seg)
    got, g = float(loss.detach()), g.cpu().numpy().astype(np.float64) / 1.7
    print("upsample_ce %s: loss %.9g, torch float64 %.9g, oracle %.9g, gradient max|err| %.3e" % (name, got, c["ref"], c["oracle"],
                                                                                               np.nanmax(np.abs(g - c["g_ref"]))))
    assert int(status.cpu().numpy()[1]) == c["n_bad"]
    if name == "all_ignored":
        assert np.isnan(c["ref"]) and np.isnan(c["oracle"]) and np.isnan(got)
    else:
        assert np.isfinite(c["ref"])
        assert abs(got - c["ref"]) <= 1e-5 * max(1.0, abs(c["ref"])), (got, c["ref"])
        assert abs(got - c["oracle"]) <= 1e-5 * max(1.0, abs(c["oracle"])), (got, c["oracle"])
    if name == "x200":
        assert c["ref"] > 100.0
    assert np.array_equal(np.isnan(g), np.isnan(c["g_ref"])), "NaN masks of the gradient differ"
    assert np.allclose(g, c["g_ref"], rtol=1e-3, atol=1e-7, equal_nan=True), np.nanmax(np.abs(g - c["g_ref"]))


def run_upsample_ce_refusal(Kk, dev):
    """w = 1, W = 40: 40 label pixels share one coarse tap, more than the 17 a cell holds. A host-side check."""
    import pytest
    seg = torch.zeros(1, 3, 2, 1, dtype=torch.float32, device=dev)
    target = torch.zeros(1, 4, 40, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError):
        Kk.upsample_ce(seg, target, None, CE_IGNORE)
