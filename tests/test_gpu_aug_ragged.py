"""Device half of the mixed-size data pipeline (csrc/augment_ragged.hip: cseg_resize_ragged = stage 1, cseg_augment_ragged = stage 2)
against the reference chain composed FORWARD from the primitives of oracle/aug_oracle.py (resize_cubic_u8, resize_nearest, slices,
[:, ::-1]) in the literal order of the transform sequence. Integer arithmetic on both sides after the coefficient tables: stage 1 and
the labels are compared with array_equal, the normalised image to 1e-5 (the bound of tests/test_gpu_aug.py, for its reason: once every
pixel is on the same grey level only the fp32 normalisation is left). Replayed on the CPU emulation by tests/test_emu_aug_ragged.py."""
import random

import numpy as np
import pytest
import torch

from oracle import aug_oracle as A
from test_gpu_aug import DIV, MEAN, STD, _rows, _smooth_images

pytestmark = pytest.mark.gpu
IDS = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lut():
    lut = np.full(256, 255, np.int16)
    for i, cid in enumerate(IDS):
        lut[cid] = i
    return lut


def make_samples(rs, sizes_hw):
    """[(img u8 [H,W,3], lab u8 [H,W])]: smooth images, raw label ids 0..33 with 5 % 255s."""
    out = []
    for (H, W) in sizes_hw:
        img = _smooth_images(rs, 1, H, W)[0]
        lab = rs.randint(0, 34, size=(H, W)).astype(np.uint8)
        lab[rs.rand(H, W) < 0.05] = 255
        out.append((img, lab))
    return out


def pack(samples):
    """-> (packed image [N,3] u8, packed label [N] u8, pixel offsets)"""
    offs = np.cumsum([0] + [s[0].shape[0] * s[0].shape[1] for s in samples])
    return (np.concatenate([s[0].reshape(-1, 3) for s in samples]), np.concatenate([s[1].reshape(-1) for s in samples]),
            [int(o) for o in offs[:-1]])


def literal(img, lab, ops):
    """The geometric transforms in the order the reference applies them: ("flip",) | ("resize", (W, H)) | ("crop", x, y, tw, th)."""
    for op in ops:
        if op[0] == "flip":
            img, lab = img[:, ::-1], lab[:, ::-1]
        elif op[0] == "resize":
            img, lab = A.resize_cubic_u8(np.ascontiguousarray(img), op[1]), A.resize_nearest(np.ascontiguousarray(lab), op[1])
        else:
            _, x, y, tw, th = op
            img, lab = img[y:y + th, x:x + tw], lab[y:y + th, x:x + tw]
    return np.ascontiguousarray(img), np.ascontiguousarray(lab)


def apply_record(img, lab, rec):
    """The same primitives driven by one CSEG_AUG_RAGGED_PARAM_INTS record (include/cseg_hip.h): stage-1 mirror + resize, stage-2
    mirror + resize, crop window, output flip -> (u8 image, u8 label) of the crop."""
    W0, H0, W1, H1, m1, Wr, Hr, m2, x, y, tw, th, flip = [int(v) for v in rec[:13]]
    assert img.shape[:2] == (H0, W0)
    ops = []
    if W1 > 0:
        ops += [("flip",)] * m1 + [("resize", (W1, H1))]
    ops += [("flip",)] * m2 + [("resize", (Wr, Hr)), ("crop", x, y, tw, th)] + [("flip",)] * flip
    return literal(img, lab, ops)


def finish(im, lb, shift, left, up, Wt, Ht, lut):
    """brightness -> ToTensor / Normalize -> label look-up, ReLabel -> collate padding, by aug_oracle.apply_chain on the finished crop."""
    th, tw = im.shape[:2]
    return A.apply_chain(im, lb, [tw, th, 0, 0, tw, th, 0, shift, left, up, 0, 0], (Wt, Ht), DIV, MEAN, STD, lut)


def run_stage2(dev, samples, recs, Ht, Wt, lut):
    from contrastiveseg_amd import kernels as K
    img, lab, offs = pack(samples)
    recs = np.asarray(recs, np.int32)
    mid_offs = np.cumsum([0] + [int(r[2]) * int(r[3]) for r in recs])[:-1]
    offsets = torch.from_numpy(np.stack([np.asarray(offs, np.int64), mid_offs.astype(np.int64)], 1))
    ti, tl = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    params = torch.from_numpy(recs)
    mid = K.resize_ragged(ti, tl, params, offsets)
    out = K.augment_ragged(ti, tl, torch.from_numpy(lut).to(dev), params, offsets, (Ht, Wt), DIV, MEAN, STD, mid=mid)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def check_against_literal(dev, samples, recs, chains, Ht, Wt):
    lut = _lut()
    got_img, got_lab = run_stage2(dev, samples, recs, Ht, Wt, lut)
    for b, ((img, lab), rec, ops) in enumerate(zip(samples, recs, chains)):
        im, lb = literal(img, lab, ops)
        assert im.shape[:2] == (rec[11], rec[10]), "case %d: the hand-built record and the literal chain disagree on the crop size" % b
        want_img, want_lab = finish(im, lb, rec[13], rec[14], rec[15], Wt, Ht, lut)
        assert np.array_equal(got_lab[b], want_lab), "labels differ for sample %d" % b
        diff = np.abs(got_img[b] - want_img)
        assert diff.max() <= 1e-5, (b, diff.max(), float((diff > 1e-5).mean()))


# ---- 1. stage 1 alone, exact ------------------------------------------------------------------------------------------------------
def test_stage1_is_the_oracles_resize_bit_for_bit():
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    rs = np.random.RandomState(11)
    samples = make_samples(rs, [(61, 83), (96, 160), (40, 33), (5, 3), (40, 33)])
    # (W1, H1), mirror: downscale, non-uniform aspect, upscale, a 3-wide source whose taps are clamped on both axes, identity (skipped)
    plan = [((50, 40), 1), ((100, 90), 0), ((70, 85), 1), ((7, 9), 1), ((0, 0), 0)]
    recs, mid_offs, m = [], [], 0
    for (img, _), ((W1, H1), mirror) in zip(samples, plan):
        H0, W0 = img.shape[:2]
        Wf, Hf = (W1, H1) if W1 else (W0, H0)
        recs.append([W0, H0, W1, H1, mirror, Wf, Hf, 0, 0, 0, Wf, Hf, 0, 0, 0, 0])
        mid_offs.append(m)
        m += W1 * H1
    img, lab, offs = pack(samples)
    offsets = torch.tensor(list(zip(offs, mid_offs)), dtype=torch.int64)
    mid_img, mid_lab = K.resize_ragged(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev),
                                       torch.tensor(recs, dtype=torch.int32), offsets)
    assert mid_img.shape == (m, 3) and mid_lab.shape == (m,)          # the identity sample owns no pixel of the stage-1 buffer
    mid_img, mid_lab = mid_img.cpu().numpy(), mid_lab.cpu().numpy()
    for (im, lb), ((W1, H1), mirror), mo in zip(samples, plan, mid_offs):
        if not W1:
            continue
        src_i, src_l = (im[:, ::-1], lb[:, ::-1]) if mirror else (im, lb)
        assert np.array_equal(mid_img[mo:mo + W1 * H1].reshape(H1, W1, 3), A.resize_cubic_u8(np.ascontiguousarray(src_i), (W1, H1)))
        assert np.array_equal(mid_lab[mo:mo + W1 * H1].reshape(H1, W1), A.resize_nearest(np.ascontiguousarray(src_l), (W1, H1)))


# ---- 2. the full chain in the COCO order: random_hflip, resize (min side 48), random_resize, random_crop [56, 40], brightness --------
def test_full_chain_in_the_coco_order():
    dev = _dev()
    samples = make_samples(np.random.RandomState(12), [(61, 83), (96, 160), (40, 33), (48, 64)])
    Ht, Wt = 48, 64
    #        W0  H0  W1  H1 m1  Wr  Hr m2   x   y  tw  th flip shift left up
    recs = [[83, 61, 65, 48, 1, 80, 57, 0, 10, 7, 56, 40, 0, 6, 5, 3],        # flip first; both resamplings: the flip is stage 1's mirror
            [160, 96, 0, 0, 0, 80, 48, 0, 24, 8, 56, 40, 0, -9, 0, 8],        # no flip; random_resize skipped: one resampling
            [33, 40, 0, 0, 0, 48, 58, 1, 0, 18, 48, 40, 0, 10, 16, 0],        # flip first; random_resize to the same size = a copy
            [64, 48, 0, 0, 0, 45, 30, 1, 0, 0, 45, 30, 0, 0, 11, 17]]         # flip first; resize is the identity, random_resize shrinks
    chains = [[("flip",), ("resize", (65, 48)), ("resize", (80, 57)), ("crop", 10, 7, 56, 40)],
              [("resize", (80, 48)), ("crop", 24, 8, 56, 40)],
              [("flip",), ("resize", (48, 58)), ("resize", (48, 58)), ("crop", 0, 18, 48, 40)],
              [("flip",), ("resize", (64, 48)), ("resize", (45, 30)), ("crop", 0, 0, 45, 30)]]
    check_against_literal(dev, samples, recs, chains, Ht, Wt)


# ---- 3. a flip between the two resamplings, and between a resampling and the crop ---------------------------------------------------
def test_flip_between_resamplings_and_ahead_of_the_crop():
    dev = _dev()
    samples = make_samples(np.random.RandomState(13), [(61, 83), (61, 83), (61, 83), (40, 33)])
    Ht, Wt = 48, 64
    recs = [[83, 61, 65, 48, 0, 90, 70, 1, 20, 11, 56, 40, 0, 4, 8, 8],       # resize, FLIP, random_resize, crop: stage 2's mirror
            [83, 61, 65, 48, 0, 90, 70, 0, 20, 11, 56, 40, 0, 4, 0, 0],       # the same with the coin the other way
            [83, 61, 0, 0, 0, 65, 48, 0, 65 - 3 - 56, 5, 56, 40, 1, -3, 2, 1],   # resize, FLIP, (random_resize skipped), crop at x = 3:
                                                                                # mirrored window W - x - tw and an output flip
            [33, 40, 0, 0, 0, 70, 50, 0, 70 - 9 - 56, 4, 56, 40, 1, 0, 8, 6]]    # random_resize, FLIP, crop at x = 9
    chains = [[("resize", (65, 48)), ("flip",), ("resize", (90, 70)), ("crop", 20, 11, 56, 40)],
              [("resize", (65, 48)), ("resize", (90, 70)), ("crop", 20, 11, 56, 40)],
              [("resize", (65, 48)), ("flip",), ("crop", 3, 5, 56, 40)],
              [("resize", (70, 50)), ("flip",), ("crop", 9, 4, 56, 40)]]
    check_against_literal(dev, samples, recs, chains, Ht, Wt)


# ---- 4. the canonical order on a uniform batch: the old entry point, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("B,Hs,Ws,Ht,Wt", [(4, 96, 160, 64, 128), (3, 61, 83, 48, 80)])
def test_uniform_batch_equals_augment_batch(B, Hs, Ws, Ht, Wt):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    rs = np.random.RandomState(Hs + Wt)
    img = _smooth_images(rs, B, Hs, Ws)
    lab = rs.randint(0, 34, size=(B, Hs, Ws)).astype(np.uint8)
    lab[rs.rand(B, Hs, Ws) < 0.05] = 255
    rows = _rows(B, Hs, Ws, Wt, Ht, rs)
    ti, tl, lut = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(_lut()).to(dev)
    old_img, old_lab = K.augment_batch(ti, tl, lut, torch.from_numpy(rows), (Ht, Wt), DIV, MEAN, STD)
    recs = [[Ws, Hs, 0, 0, 0, r[0], r[1], 0] + [int(v) for v in r[2:10]] for r in rows]
    offsets = torch.tensor([[b * Hs * Ws, 0] for b in range(B)], dtype=torch.int64)
    new_img, new_lab = K.augment_ragged(ti, tl, lut, torch.tensor(recs, dtype=torch.int32), offsets, (Ht, Wt), DIV, MEAN, STD)
    assert torch.equal(new_img, old_img) and torch.equal(new_lab, old_lab)


# ---- 5. refusals: the wrapper and the library ------------------------------------------------------------------------------------------
def _small(dev):
    samples = make_samples(np.random.RandomState(5), [(12, 9), (7, 10)])
    img, lab, offs = pack(samples)
    recs = [[9, 12, 6, 8, 0, 10, 10, 0, 0, 0, 10, 10, 0, 0, 0, 0], [10, 7, 0, 0, 0, 10, 7, 0, 0, 0, 10, 7, 0, 0, 0, 0]]
    return (torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), torch.tensor(recs, dtype=torch.int32),
            torch.tensor([[offs[0], 0], [offs[1], 0]], dtype=torch.int64))


def test_refusals():
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    ti, tl, params, offsets = _small(dev)
    args = ((10, 10), DIV, MEAN, STD)
    mid = K.resize_ragged(ti, tl, params, offsets)
    K.augment_ragged(ti, tl, None, params, offsets, *args, mid=mid)                  # the accepted call
    past = offsets.clone()
    past[1, 0] += 1                                         # the last sample now ends one pixel past the buffer
    with pytest.raises(RuntimeError, match="past the source buffer"):
        K.resize_ragged(ti, tl, params, past)
    with pytest.raises(RuntimeError, match="past the source buffer"):
        K.augment_ragged(ti, tl, None, params, past, *args, mid=mid)
    with pytest.raises(RuntimeError, match="stage-1 buffer"):          # a record that reads stage 1, no stage-1 buffer handed in
        K.augment_ragged(ti, tl, None, params, offsets, *args)
    zero = params.clone()
    zero[1, 0] = 0
    with pytest.raises(RuntimeError, match="non-positive source size"):
        K.resize_ragged(ti, tl, zero, offsets)
    with pytest.raises(RuntimeError, match="non-positive source size"):
        K.augment_ragged(ti, tl, None, zero, offsets, *args, mid=mid)
    outside = params.clone()
    outside[1, 8] = 1                                       # crop 10 wide at x = 1 in a 10-wide image
    with pytest.raises(RuntimeError, match="outside its resized image"):
        K.augment_ragged(ti, tl, None, outside, offsets, *args, mid=mid)
    with pytest.raises(RuntimeError, match="label buffer"):
        K.augment_ragged(ti, tl[:-1].contiguous(), None, params, offsets, *args, mid=mid)


def test_cpu_tensors_are_refused():
    """The product has no CPU path (not replayed on the emulator, whose device IS the CPU)."""
    _dev()
    from contrastiveseg_amd import kernels as K
    ti, tl, params, offsets = _small(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="GPU"):
        K.resize_ragged(ti, tl, params, offsets)
    with pytest.raises(RuntimeError, match="GPU"):
        K.augment_ragged(ti, tl, None, params, offsets, (10, 10), DIV, MEAN, STD)


def test_the_library_refuses_what_the_wrapper_refuses():
    import ctypes
    dev = _dev()
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    ti, tl, params, offsets = _small(dev)
    lib = _hip.lib()
    pd, od = params.to(dev), offsets.to(dev)
    mid_i, mid_l = torch.empty(48, 3, dtype=torch.uint8, device=dev), torch.empty(48, dtype=torch.uint8, device=dev)
    out_i = torch.empty(2, 3, 10, 10, device=dev)
    out_l = torch.empty(2, 10, 10, dtype=torch.int64, device=dev)
    mean3, std3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)
    n = ti.numel() // 3

    def stage1(lab=tl, mid_lab=mid_l, B=2, n=n, m=48, ph=params, oh=offsets):
        return lib.cseg_resize_ragged(P(ti), P(lab), n, P(pd), P(od), P(ph), P(oh), B, P(mid_i), P(mid_lab), m, _hip.stream_ptr())

    def stage2(lab=tl, out_lab=out_l, B=2, n=n, m=48, Ht=10, ph=params, oh=offsets, img=ti):
        return lib.cseg_augment_ragged(P(img), P(lab), n, P(mid_i), P(mid_l), m, P(None), P(pd), P(od), P(ph), P(oh), B, Ht, 10,
                                       DIV, mean3, std3, P(out_i), P(out_lab), _hip.stream_ptr())

    def refused(ret, text):
        assert ret == 0 and text in lib.cseg_last_error().decode(), (ret, lib.cseg_last_error())
    assert stage1() == 1 and stage2() == 1
    refused(stage1(mid_lab=None), "label input and output must come together")
    refused(stage2(out_lab=None), "label input and output must come together")
    refused(stage2(lab=None), "label input and output must come together")
    refused(stage1(n=n - 1), "past the source buffer")
    refused(stage2(n=n - 1), "past the source buffer")
    refused(stage1(m=47), "past the stage-1 buffer")
    refused(stage2(m=47), "past the stage-1 buffer")
    past = offsets.clone()
    past[0, 0] = -1
    refused(stage2(oh=past), "past the source buffer")
    zero = params.clone()
    zero[0, 1] = 0
    refused(stage1(ph=zero), "non-positive source size")
    refused(stage2(ph=zero), "non-positive source size")
    refused(stage2(Ht=0), "bad output size")
    refused(stage1(B=0), "outside 1..65535")
    refused(stage2(B=65536), "outside 1..65535")
    refused(stage2(img=None), "null pointer")
    refused(stage1(ph=None), "null pointer")
    torch.cuda.synchronize()


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    dev = _dev()
    samples = make_samples(np.random.RandomState(6), [(61, 83), (40, 33)])
    recs = [[83, 61, 65, 48, 1, 80, 57, 0, 10, 7, 56, 40, 1, 6, 5, 3], [33, 40, 0, 0, 0, 70, 50, 1, 5, 4, 56, 40, 0, -2, 8, 6]]
    a = run_stage2(dev, samples, recs, 48, 64, _lut())
    b = run_stage2(dev, samples, recs, 48, 64, _lut())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 7. end to end through GPUBatchTransform: the reference's COCO train_trans, scaled down ----------------------------------------
COCO_TRANS = {"trans_seq": ["random_hflip", "resize", "random_resize", "random_crop", "random_brightness"],
              "random_brightness": {"ratio": 1.0, "shift_value": 10},
              "resize": {"min_side_length": 64},
              "random_hflip": {"ratio": 0.5, "swap_pair": []},
              "random_resize": {"ratio": 1.0, "method": "random", "scale_range": [0.5, 2.0], "aspect_range": [0.9, 1.1]},
              "random_crop": {"ratio": 1.0, "crop_size": [96, 64], "method": "random", "allow_outside_center": False}}


def test_gpu_batch_transform_end_to_end_on_mixed_sizes():
    dev = _dev()
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    cfg = Configer(config_dict={
        "data": {"num_classes": 19, "label_list": IDS},
        "train": {"data_transformer": {"size_mode": "fix_size", "input_size": [96, 64], "align_method": "only_pad",
                                       "pad_mode": "random"}},
        "train_trans": COCO_TRANS, "normalize": {"div_value": DIV, "mean": MEAN, "std": STD}})
    t = GPUBatchTransform(cfg)
    samples = make_samples(np.random.RandomState(7), [(96, 160), (120, 90), (81, 123), (64, 64)])
    img, lab, _ = pack(samples)
    sizes = [(s[0].shape[1], s[0].shape[0]) for s in samples]
    random.seed(99)
    out = t(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), sizes=sizes)
    assert out["img"].shape == (4, 3, 64, 96) and out["labelmap"].shape == (4, 64, 96) and out["labelmap"].dtype == torch.int64
    recs = out["aug_params"].cpu().numpy()
    assert recs.shape == (4, 16) and (recs[:, 2] > 0).any()            # at least one sample went through both stages
    got_img, got_lab = out["img"].cpu().numpy(), out["labelmap"].cpu().numpy()
    for b, (im0, lb0) in enumerate(samples):
        im, lb = apply_record(im0, lb0, recs[b])
        want_img, want_lab = finish(im, lb, recs[b][13], recs[b][14], recs[b][15], 96, 64, t.lut.cpu().numpy())
        assert np.array_equal(got_lab[b], want_lab)
        assert np.abs(got_img[b] - want_img).max() <= 1e-5


# ---- 8. files of mixed sizes -> loaders -> Trainer (GPU only) ---------------------------------------------------------------------
def make_mixed_folder_dataset(tmp_path, ids, rs, sizes_hw=((96, 160), (120, 90), (81, 123))):
    from PIL import Image
    for split, n in (("train", 5), ("val", 3)):
        (tmp_path / split / "image").mkdir(parents=True)
        (tmp_path / split / "label").mkdir(parents=True)
        for i in range(n):
            H, W = sizes_hw[i % len(sizes_hw)]
            Image.fromarray(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(str(tmp_path / split / "image" / ("f%02d.png" % i)))
            lab = np.full((H, W), 255, np.uint8)
            for _ in range(8):
                y, x = rs.randint(0, H), rs.randint(0, W)
                lab[y:y + 40, x:x + 60] = ids[rs.randint(0, len(ids))]
            Image.fromarray(lab).save(str(tmp_path / split / "label" / ("f%02d.png" % i)))


def mixed_folder_config(tmp_path, ids, cpu):
    from test_gpu_aug_host import folder_trainer_config
    cfg = folder_trainer_config(tmp_path, ids, cpu)
    cfg.update(["train_trans"], dict(COCO_TRANS))
    cfg.update(["val_trans"], {"trans_seq": ["resize"], "resize": {"min_side_length": 64}})
    cfg.update(["val"], {"batch_size": 2, "data_transformer": {"size_mode": "diverse_size", "align_method": "only_pad",
                                                               "pad_mode": "pad_right_down"}})
    return cfg


def test_mixed_size_folder_feeds_the_trainer_on_gpu(tmp_path):
    """Mixed-size files -> packed upload -> cseg_resize_ragged + cseg_augment_ragged -> Trainer: two SGD steps and a validation pass
    that sees one image per batch at its own resized size."""
    _dev()
    from contrastiveseg_amd.lib.datasets.data_loader import GPUAugLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    ids = [7, 8, 11, 12, 13]
    make_mixed_folder_dataset(tmp_path, ids, np.random.RandomState(0))
    cfg = mixed_folder_config(tmp_path, ids, cpu=False)
    random.seed(5)
    torch.manual_seed(304)
    tr = Trainer(cfg)
    assert isinstance(tr.train_loader, GPUAugLoader) and len(tr.train_loader) == 2
    batch = next(iter(tr.train_loader))
    assert batch["img"].shape == (2, 3, 64, 96) and batch["labelmap"].shape == (2, 64, 96)
    assert int(batch["labelmap"].min()) >= -1 and int(batch["labelmap"].max()) <= 4
    shapes = [tuple(vb["img"].shape) for vb in tr.val_loader]
    # min side 64: 96 x 160 -> 64 x 107, 120 x 90 -> 85 x 64, 81 x 123 -> 64 x 97 (H x W), one image per batch
    assert shapes == [(1, 3, 64, 107), (1, 3, 85, 64), (1, 3, 64, 97)]
    tr.train()
    assert cfg.get("iters") == 2 and 0.0 <= cfg.get("performance") <= 1.0
