"""Training-time augmentation, tensor conversion and batch collation of the reference, re-designed for the GPU
(SURVEY.md section 8 f4). Same config schema as the reference:

    train_trans.trans_seq = [random_resize, random_crop, random_hflip, random_brightness]   (cv2_aug_transforms.py:654-760)
                          | [random_hflip, resize, random_resize, random_crop, random_brightness]   (COCO-Stuff, ADE20K, ...)
    val_trans.trans_seq   = [] | [resize]
    normalize = {div_value, mean, std}                                                     (data_loader.py:39-49)
    train.data_transformer = {size_mode: fix_size, input_size: [W, H], align_method: only_pad, pad_mode: random}
    val.data_transformer   = the same | {size_mode: diverse_size, align_method: only_pad, pad_mode, fit_stride}
    data.label_list (raw id -> train id), data.reduce_zero_label                            (default_loader.py:83-106)

What moves where: every RANDOM DECISION stays on the host and is drawn from Python's `random` module in exactly the
reference's order (per sample: resize scale, aspect, resize coin; crop x, y, crop coin; flip coin; brightness coin and
shift -- then per batch the collate pad offsets), so a seed gives the same geometric decisions as the reference loader
with workers=0. Everything that touches pixels -- cv2.resize, the crop slice, cv2.flip, the brightness arithmetic,
ToTensor / Normalize, label encoding, ReLabel and the padding of collate -- runs on the raw uint8 images on the device:
the host only decodes files and uploads uint8.

Two device paths. A batch of equal-sized images whose sequence has no `resize` and no flip ahead of a crop or resampling is
ONE kernel launch with a 12-int record per image (cseg_augment_batch), as it always was. Everything else -- images of differing
sizes in one packed buffer, the `resize` transform, a flip that does not come last -- takes the ragged path
(csrc/augment_ragged.hip): stage 1 (cseg_resize_ragged) for the samples that undergo two resamplings, whose intermediate image
the reference rounds to bytes, then stage 2 (cseg_augment_ragged) for everything else, with a 16-int record per image.

Composition rule (GPUAugCompose.draw). The sequence is walked in order with a PENDING MIRROR bit: random_hflip toggles it; a
resampling consumes it as that stage's `mirror` flag (cv2.resize of the flipped image is not the flip of cv2.resize: cv2's
nearest rule min(floor(d * scale), W - 1) and the cubic taps are not symmetric on the pixel grid); a crop under a pending mirror
takes the mirrored window x -> W - x - tw and leaves the bit pending; what is pending at the end is the output flip. A
resampling to the size the image already has is a copy (cv::resize does that) and counts as no resampling.

random_hflip.swap_pair (the LIP configs: left / right arm, leg, shoe). An applied flip also trades the listed label ids (swap_table).
That is a value map, which draws no random number and commutes with the nearest resamplings, the crop and the padding, so a sample's
labels are swapped iff its number of applied flips is odd: stage-1 mirror ^ stage-2 mirror ^ output flip on the ragged path, the flip
bit on the one-kernel path (a mirrored crop window leaves its flip pending and does not count). The kernels pick between two
tables, lut and lut_mirrored = lut o swap."""
import math
import random

import numpy as np
import torch

from contrastiveseg_amd import kernels as K

SUPPORTED = ('random_resize', 'random_crop', 'random_hflip', 'random_brightness', 'resize')
RESAMPLINGS = ('resize', 'random_resize')


def swap_table(swap_pair):
    """random_hflip.swap_pair -> the value map of RandomHFlip._process_labelmap (cv2_aug_transforms.py:151-162) as uint8 [256], or
    None without pairs. The reference assigns, for every pair in order and from a copy of the flipped map, labelmap[temp == a] = b and
    labelmap[temp == b] = a: swap[v] is the partner of v in the LAST pair that mentions v, v itself where none does. It acts on raw
    label ids, ahead of the label_list / reduce_zero_label encoding. 255 is the pad / ignore value of the label path (a label-free
    sample reads 255, ReLabel maps it to -1) and cannot be swapped."""
    if not swap_pair:
        return None
    if not isinstance(swap_pair, (list, tuple)):
        raise ValueError('random_hflip.swap_pair {!r}: expected a list of [a, b] pairs'.format(swap_pair))
    swap = np.arange(256, dtype=np.uint8)
    for pair in swap_pair:
        if not isinstance(pair, (list, tuple)) or len(pair) != 2 or \
                not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in pair):
            raise ValueError('random_hflip.swap_pair entry {!r}: expected two integer label ids [a, b]'.format(pair))
        a, b = int(pair[0]), int(pair[1])
        if a == 255 or b == 255:
            raise ValueError('random_hflip.swap_pair entry {!r} mentions 255, the pad / ignore value of the label path'.format(pair))
        if not (0 <= a <= 254 and 0 <= b <= 254):
            raise ValueError('random_hflip.swap_pair entry {!r}: label ids must lie in 0..254'.format(pair))
        swap[a], swap[b] = b, a
    return swap


class SampleParams(object):
    """Decisions for one sample, in the reference's drawing order. Wr x Hr: the size after the last resampling; x_off .. th: the
    crop window in that image; flip: the output flip; stages: the non-identity resamplings [(W, H, mirror)], two at the most."""
    __slots__ = ('W0', 'H0', 'Wr', 'Hr', 'x_off', 'y_off', 'tw', 'th', 'flip', 'shift', 'stages')

    def as_list(self, left_pad=0, up_pad=0):
        """The CSEG_AUG_PARAM_INTS record of cseg_augment_batch (no mirror flags: the caller has ruled them out)."""
        return [self.Wr, self.Hr, self.x_off, self.y_off, self.tw, self.th, int(self.flip), self.shift, left_pad, up_pad,
                0, 0]

    def as_ragged(self, left_pad=0, up_pad=0):
        """The CSEG_AUG_RAGGED_PARAM_INTS record of cseg_resize_ragged / cseg_augment_ragged (include/cseg_hip.h)."""
        W1 = H1 = m1 = m2 = 0
        if len(self.stages) == 2:
            W1, H1, m1 = self.stages[0]
        if self.stages:
            m2 = self.stages[-1][2]
        return [self.W0, self.H0, W1, H1, int(m1), self.Wr, self.Hr, int(m2), self.x_off, self.y_off, self.tw, self.th,
                int(self.flip), self.shift, left_pad, up_pad]


class GPUAugCompose(object):
    """Host half of CV2AugCompose (cv2_aug_transforms.py:654-760): parses the same config and draws the decisions."""

    def __init__(self, configer, split='train'):
        self.configer = configer
        self.split = split
        key = 'train_trans' if split == 'train' else 'val_trans'
        self.cfg = configer.get(key) if configer.exists(key) else {'trans_seq': []}
        if split == 'test':
            self.cfg = {'trans_seq': []}                   # the reference's test loader has no aug_transform (data_loader.py:205-240)
        if self.cfg.get('shuffle_trans_seq'):
            raise NotImplementedError('shuffle_trans_seq is outside the accelerated data path')
        self.seq = list(self.cfg.get('trans_seq', []))
        for name in self.seq:
            if name not in SUPPORTED:
                raise NotImplementedError('augmentation {!r} is outside the accelerated data path; supported: {}'
                                          .format(name, SUPPORTED))
        for name in RESAMPLINGS:
            if self.seq.count(name) > 1:
                raise NotImplementedError('trans_seq holds {!r} {} times: one resize and one random_resize at the most (two '
                                          'resampling stages on the device)'.format(name, self.seq.count(name)))
        crops = [i for i, name in enumerate(self.seq) if name == 'random_crop']
        for i, name in enumerate(self.seq):
            if name in RESAMPLINGS and crops and crops[0] < i:
                raise NotImplementedError('{!r} after random_crop in trans_seq: a resampling of a cropped image is outside the '
                                          'accelerated data path'.format(name))
        rr = self.cfg.get('random_resize', {})
        if 'random_resize' in self.seq and rr.get('method', 'random') != 'random':
            raise NotImplementedError("random_resize.method {!r}: only 'random' is implemented".format(rr.get('method')))
        rc = self.cfg.get('random_crop', {})
        if 'random_crop' in self.seq and rc.get('method', 'random') not in ('random', 'center'):
            raise NotImplementedError("random_crop.method {!r}: only 'random' / 'center'".format(rc.get('method')))
        hf = self.cfg.get('random_hflip', {})
        self.swap = swap_table(hf.get('swap_pair')) if 'random_hflip' in self.seq else None
        if self.swap is not None and self.seq.count('random_hflip') > 1 and not np.array_equal(self.swap[self.swap], np.arange(256)):
            # the kernels swap by the PARITY of the applied flips, which is the reference's result only when swapping twice is the
            # identity; pairs that share an id are not, and two flips would apply such a map twice
            raise NotImplementedError('random_hflip.swap_pair {!r} with pairs that share an id, in a trans_seq with more than one '
                                      'random_hflip, is outside the accelerated data path'.format(hf.get('swap_pair')))
        if 'resize' in self.seq:
            rz = self.cfg.get('resize', {})
            if not any(rz.get(k) is not None for k in ('target_size', 'min_side_length', 'max_side_length')):
                raise RuntimeError('resize needs one of target_size / min_side_length / max_side_length')
        # the one-kernel path expresses a single flip AFTER the crop and the resampling, and no `resize`
        flips = [i for i, name in enumerate(self.seq) if name == 'random_hflip']
        geometric = [i for i, name in enumerate(self.seq) if name in RESAMPLINGS or name == 'random_crop']
        self.canonical = 'resize' not in self.seq and not (flips and geometric and flips[0] < geometric[-1])

    @staticmethod
    def _resize_target(c, width, height):
        """Resize.__call__ (cv2_aug_transforms.py:618-651): no random number, never skipped."""
        if c.get('target_size') is not None:
            target = list(c['target_size'])
            w_ratio, h_ratio = target[0] / width, target[1] / height
        elif c.get('min_side_length') is not None:
            w_ratio = h_ratio = c['min_side_length'] / min(width, height)
            target = [int(round(width * w_ratio)), int(round(height * h_ratio))]
        else:
            w_ratio = h_ratio = c['max_side_length'] / max(width, height)
            target = [int(round(width * w_ratio)), int(round(height * h_ratio))]
        bound = c.get('max_side_bound')
        if bound is not None and max(target) > bound:
            d = bound / max(target)
            w_ratio, h_ratio = d * w_ratio, d * h_ratio
            target = [int(round(width * w_ratio)), int(round(height * h_ratio))]
        return int(target[0]), int(target[1])

    def draw(self, width, height):
        """One sample of size (width, height). Reference order of `random` calls:
        RandomResize.__call__ :405-443 (uniform scale | scale_list index, uniform aspect, coin), RandomCrop :580-603
        (randint x, randint y, coin), RandomHFlip :202-208 (coin), RandomBrightness :318-324 + :310-315 (coin, then
        randint shift only when applied); Resize :618-651 draws nothing."""
        p = SampleParams()
        p.W0, p.H0 = width, height
        p.Wr, p.Hr = width, height
        p.x_off = p.y_off = 0
        p.tw, p.th = width, height
        p.shift, p.stages = 0, []
        mirror = False                                     # the pending mirror bit

        def resample(size):
            nonlocal mirror
            if size == (p.tw, p.th):                       # cv::resize to the same size copies: the mirror stays pending
                return
            p.stages.append((size[0], size[1], mirror))
            mirror = False
            p.Wr, p.Hr = size
            p.tw, p.th = size
        for name in self.seq:
            c = self.cfg[name]
            if name == 'resize':
                resample(self._resize_target(c, p.tw, p.th))
            elif name == 'random_resize':
                if c.get('scale_list') is None:
                    scale = random.uniform(c['scale_range'][0], c['scale_range'][1])
                else:
                    scale = c['scale_list'][random.randint(0, len(c['scale_list']) - 1)]
                aspect = random.uniform(*c['aspect_range'])
                w_ratio = math.sqrt(aspect) * scale
                h_ratio = math.sqrt(1.0 / aspect) * scale
                bound = c.get('max_side_bound')
                if bound is not None and max(p.Hr * h_ratio, p.Wr * w_ratio) > bound:
                    d = bound / max(p.Hr * h_ratio, p.Wr * w_ratio)
                    w_ratio *= d
                    h_ratio *= d
                size = (int(p.Wr * w_ratio), int(p.Hr * h_ratio))
                if not (random.random() > c['ratio']):
                    if size[0] <= 0 or size[1] <= 0:
                        raise RuntimeError('random_resize produced an empty image ({}x{})'.format(*size))
                    resample(size)
            elif name == 'random_crop':
                cw, ch = c['crop_size']
                tw, th = min(cw, p.tw), min(ch, p.th)
                if c.get('method', 'random') == 'center':
                    x, y = (p.tw - tw) // 2, (p.th - th) // 2
                else:
                    x = random.randint(0, p.tw - tw)
                    y = random.randint(0, p.th - th)
                if not (random.random() > c['ratio']):
                    if mirror:                             # the reference crops the flipped image: the mirrored window of this one
                        x = p.tw - x - tw
                    p.x_off, p.y_off, p.tw, p.th = p.x_off + x, p.y_off + y, tw, th
            elif name == 'random_hflip':
                if not (random.random() > c['ratio']):
                    mirror = not mirror
            elif name == 'random_brightness':
                if not (random.random() > c['ratio']):
                    p.shift += random.randint(-c['shift_value'], c['shift_value'])
        p.flip = mirror
        if p.Wr <= 0 or p.Hr <= 0:
            raise RuntimeError('resize produced an empty image ({}x{})'.format(p.Wr, p.Hr))
        return p


class GPUBatchTransform(object):
    """aug_transform + img_transform + label_transform + collate of the reference's train loader
    (lib/datasets/data_loader.py:130-140 -> DefaultLoader.__getitem__ -> collate) for one batch."""

    def __init__(self, configer, split='train'):
        self.configer = configer
        self.aug = GPUAugCompose(configer, split)
        dt = configer.get(split if split in ('train', 'test') else 'val', 'data_transformer')
        self.size_mode = dt.get('size_mode', 'fix_size')
        if self.size_mode not in ('fix_size', 'diverse_size'):
            raise NotImplementedError("size_mode {!r}: only 'fix_size' and 'diverse_size' are implemented"
                                      .format(dt.get('size_mode')))
        if dt.get('align_method', 'only_pad') != 'only_pad':
            raise NotImplementedError("align_method {!r}: only 'only_pad' is implemented".format(dt.get('align_method')))
        self.pad_mode = dt.get('pad_mode', 'random')
        if self.pad_mode not in ('random', 'pad_left_up', 'pad_right_down', 'pad_center'):
            raise NotImplementedError('pad_mode {!r}'.format(self.pad_mode))
        if self.size_mode == 'fix_size':
            self.target_w, self.target_h = dt['input_size']
        else:                                              # every image at its own size: batches of one (data_helper.py:107-112)
            self.target_w = self.target_h = None
        self.fit_stride = dt.get('fit_stride') if self.size_mode == 'diverse_size' else None
        norm = configer.get('normalize') if configer.exists('normalize') else \
            {'div_value': 255.0, 'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}
        self.div, self.mean, self.std = norm['div_value'], norm['mean'], norm['std']
        self.lut = None
        reduce_zero = configer.exists('data', 'reduce_zero_label') and configer.get('data', 'reduce_zero_label')
        if configer.exists('data', 'label_list'):
            lut = np.full(256, 255, dtype=np.int16)               # default_loader.py:94-106: unlisted ids -> 255
            for i, cid in enumerate(configer.get('data', 'label_list')):
                lut[cid] = i
            if reduce_zero:                                       # :51-55: encoded first, then shifted (COCO-Stuff: "unlabeled" is
                lut = np.where(lut == 255, 255, lut - 1)          # entry 0 of the list and becomes ignore); unlisted ids stay ignore
                lut = np.where(lut < 0, 255, lut).astype(np.int16)
            self.lut = torch.from_numpy(lut)
        elif reduce_zero:
            lut = np.arange(256, dtype=np.int16) - 1              # default_loader.py:83-92 (uint8 wrap: 0 -> 255)
            lut[0] = 255
            self.lut = torch.from_numpy(lut)
        # random_hflip.swap_pair: the table of the samples with an odd number of applied flips, lut o swap (the swap acts on raw
        # ids, the encoding follows); over the identity table when there is no encoding
        self.lut_mirrored = None
        if self.aug.swap is not None:
            base = self.lut.numpy() if self.lut is not None else np.arange(256, dtype=np.int16)
            self.lut_mirrored = torch.from_numpy(np.ascontiguousarray(base[self.aug.swap].astype(np.int16)))

    def _target(self, samples):
        """(Wt, Ht) of the batch: the fixed input size, or under diverse_size the single sample's own size, padded right / down to
        fit_stride (collate.py:39-41, 61-68)."""
        if self.size_mode == 'fix_size':
            return self.target_w, self.target_h
        if len(samples) != 1:
            raise RuntimeError("size_mode 'diverse_size' collates one image per batch (got {}): the reference runs each image "
                               'through the network alone at its own size'.format(len(samples)))
        tw, th = samples[0].tw, samples[0].th
        if self.fit_stride:
            tw, th = tw + (-tw) % self.fit_stride, th + (-th) % self.fit_stride
        return tw, th

    def _plan(self, sizes):
        """Sample decisions first (one __getitem__ per sample), then the collate pads in sample order (collate.py:108-121)."""
        samples = [self.aug.draw(w, h) for (w, h) in sizes]
        target_w, target_h = self._target(samples)
        pads = []
        for p in samples:
            pad_w, pad_h = target_w - p.tw, target_h - p.th
            if pad_w < 0 or pad_h < 0:
                raise RuntimeError('sample of {}x{} exceeds the fixed input size {}x{} (the reference asserts here, '
                                   'collate.py:106)'.format(p.tw, p.th, target_w, target_h))
            left = up = 0
            if pad_w > 0 or pad_h > 0:
                if self.pad_mode == 'random':
                    left = random.randint(0, pad_w)
                    up = random.randint(0, pad_h)
                elif self.pad_mode == 'pad_left_up':
                    left, up = pad_w, pad_h
                elif self.pad_mode == 'pad_center':
                    left, up = pad_w // 2, pad_h // 2
            pads.append((left, up))
        return samples, pads, (target_w, target_h)

    def plan(self, sizes):
        """-> int32 [B, AUG_PARAM_INTS], the records of the one-kernel path."""
        samples, pads, _ = self._plan(sizes)
        return torch.tensor([p.as_list(left, up) for p, (left, up) in zip(samples, pads)], dtype=torch.int32)

    def plan_ragged(self, sizes):
        """-> (int32 [B, AUG_RAGGED_PARAM_INTS], int64 [B, 2] pixel offsets of the raw and of the stage-1 buffer, (Wt, Ht)) for
        images packed in the order of `sizes`."""
        samples, pads, target = self._plan(sizes)
        rows = [p.as_ragged(left, up) for p, (left, up) in zip(samples, pads)]
        offsets, raw, mid = [], 0, 0
        for r in rows:
            offsets.append([raw, mid])
            raw += r[0] * r[1]
            mid += r[2] * r[3]
        return torch.tensor(rows, dtype=torch.int32), torch.tensor(offsets, dtype=torch.int64), target

    def __call__(self, img_u8, lab_u8, sizes=None):
        """A uniform batch: img_u8 [B,Hs,Ws,3] uint8, lab_u8 [B,Hs,Ws] uint8 (raw label ids) or None. A ragged batch: `sizes` =
        [(W, H)] per sample, img_u8 the packed HWC images ([N,3] uint8), lab_u8 the packed labels ([N] uint8) or None. All already
        on the device. -> img, labelmap, aug_params (the records of the path taken), border_size [(tw, th)], pad_offset [(left, up)]."""
        if self.lut is not None and self.lut.device != img_u8.device:
            self.lut = self.lut.to(img_u8.device)
        if self.lut_mirrored is not None and self.lut_mirrored.device != img_u8.device:
            self.lut_mirrored = self.lut_mirrored.to(img_u8.device)
        lab_u8 = None if lab_u8 is None else lab_u8.contiguous()
        swap = {} if self.lut_mirrored is None else {'lut_mirrored': self.lut_mirrored}      # without pairs: the calls as they were
        if sizes is None and self.aug.canonical and self.size_mode == 'fix_size':
            B, Hs, Ws, _ = img_u8.shape
            params = self.plan([(Ws, Hs)] * B)
            img, lab = K.augment_batch(img_u8.contiguous(), lab_u8, self.lut, params, (self.target_h, self.target_w), self.div,
                                       self.mean, self.std, **swap)
            rows = params.tolist()
            return {'img': img, 'labelmap': lab, 'aug_params': params, 'border_size': [(r[4], r[5]) for r in rows],
                    'pad_offset': [(r[8], r[9]) for r in rows]}
        if sizes is None:                                  # equal sizes, but a sequence the one-kernel path cannot express
            B, Hs, Ws, _ = img_u8.shape
            sizes = [(Ws, Hs)] * B
        params, offsets, (Wt, Ht) = self.plan_ragged(sizes)
        img_u8 = img_u8.contiguous()
        mid = K.resize_ragged(img_u8, lab_u8, params, offsets) if bool((params[:, 2] > 0).any()) else None
        img, lab = K.augment_ragged(img_u8, lab_u8, self.lut, params, offsets, (Ht, Wt), self.div, self.mean, self.std, mid=mid, **swap)
        rows = params.tolist()
        return {'img': img, 'labelmap': lab, 'aug_params': params, 'aug_offsets': offsets,
                'border_size': [(r[10], r[11]) for r in rows], 'pad_offset': [(r[14], r[15]) for r in rows]}
