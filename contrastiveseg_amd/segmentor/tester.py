"""Test phase with the reference's surface (segmentor/tester.py:56-523: `Tester(configer).test()`, `ss_test`, `ms_test`, `sscrop_test`,
`mscrop_test`, `ms_test_depth`) and config keys (test.mode, test.scale_search, optional test.scale_weights, test.crop_size,
test.batch_size, test.out_dir, test.save_prob, network.resume; test.depth_dir is this project's own).

What the reference does per scale -- upsample two coarse logit maps to the input size, flip one, add, scale, accumulate into a
[B,K,H,W] tensor (:310-327, :380-398), then move everything to the host for the argmax (:169-189) -- is linear up to the argmax.
Here the model runs once per scale and once more on the mirrored input, only the coarse `seg` maps are kept, and one
kernels.ms_fuse_argmax call per batch writes the prediction as one byte per pixel; the fused fp32 map exists only under
test.save_prob. Scoring (where ground truth exists) is kernels.confusion_update into an on-device RunningScore.

The sliding-crop modes (:351-378, :505-523) build a logits canvas and a count canvas of [B,K,H*scale,W*scale] per scale and flip. Here
the resized input is cut into the reference's tiles, the model runs once per tile, its coarse output goes into a preallocated stack
[tiles,B,K,hc,wc], and one kernels.crop_fuse_argmax call per batch does the rest: no canvas exists.

Datasets whose images differ in size (`test.data_transformer.size_mode: diverse_size`, every *_TEST.json of the reference outside
Cityscapes and CamVid): a batch is a LIST of [1,3,Hp_b,Wp_b] tensors, each image padded right / down to fit_stride (collate.py:61-68,
107-146). As in the reference's list branches (:328-341, :400-421) every image goes through the network alone -- images of equal
size are not batched either: the split-operand kernels scale each tensor by its own max|.|, so batch composition would show in the
result -- and only the coarse maps are kept; one kernels.ms_fuse_argmax_ragged call scores the batch over each image's own unpadded
region into packed buffers, which the confusion matrix takes as they are. The reference's test loader applies no resize
(default_loader.py:273-289: ori_img_size = border_size = the file's own size; collate.py:91-92 changes border_size only under the
scaling align methods), so under only_pad its final cv2.resize(outputs[:border_h, :border_w], ori_img_size, INTER_CUBIC) (:180-181)
has equal source and target size and copies.

test.flip_swap_pair (this project's own key, like contrast.use_ohem; absent by default, which is the reference's behaviour): a list of
class pairs that trade places under the mirror (LIP: left / right arm, leg, shoe). The mirrored pass of ms_test is then read through
that channel permutation inside the scoring kernel (kernels.ms_fuse_argmax(perm=...)); the sliding-crop modes refuse the key.

ms_test_depth (:426-482, the recipe of configs/cityscapes/H_48_D_4_TEST_DEPTH.json): ms_test with flips whose per-scale weight is
per PIXEL, 0.8 ** |bin - index of the scale|, the bin coming from the image's uint16 disparity PNG. The reference's float64 numpy
statements are evaluated once per Tester over the whole uint16 domain (depth_fusion_tables): a byte table of 65 536 bins and an fp32
table [scales, bins]. Per batch the disparity maps <test.depth_dir>/<name>.png are placed at each image's pad_offset in a zero
uint16 [B,H,W] buffer (disparity 0 = infinitely far, as the reference's division by zero gives), uploaded once, binned by
kernels.lut_u16_u8 and handed to kernels.ms_fuse_argmax(pixel_weights=...); no weight map and no [B,K,H,W] tensor exists.
test.depth_dir replaces the reference's hard-coded stereo paths (:450-453); the mode is refused without it, under size_mode
diverse_size (the reference raises on list inputs, :444-445) and together with test.flip_swap_pair. test.scale_weights is not read,
as in the reference. A disparity map of another size than the image is refused: the reference's cv2.resize of the weight map (:471)
is the identity only for equal sizes, and it is not approximated.

test.evaluator: "cityscapes" (this project's own key; absent by default, and then nothing changes) adds the reference's third stage,
`python -m lib.metrics.cityscapes_evaluator`, to the test phase: per-class and per-category IoU and instance-weighted iIoU, the four
averages, priors and pixel accuracy (lib/metrics/cityscapes_score.py). The loader additionally yields every image's raw label ids and
its 16-bit instance ids (<test.instance_dir>/<name>.png, default <test_dir>/../instance) at the image's pad_offset; per batch
CityscapesScore.update runs kernels.cs_eval_update / cs_eval_reduce on the prediction that is on the device anyway; rank 0 logs the
reference's two tables and writes <out_dir>/evaluationResults/resultPixelLevelSemanticLabeling.json. The mIoU line and last_miou stay
as they are. Refused by name: another evaluator, size_mode diverse_size, a data.label_list with an entry outside 0..33, a missing
label or instance directory or file, an instance map of another size than its image.

test.segfix_offset_dir (this project's own key; absent by default, and then nothing changes) with test.segfix_scale (default 2.0) adds
the reference's second stage, scripts/cityscapes/segfix.py, to the test phase: every pixel's label moves along a precomputed
boundary offset (<dir>/<name>.mat as the script reads it, else <dir>/<name>.npy; lib/datasets/segfix_offsets.py). The loader yields
the offsets at each image's pad_offset, int8 where the file's integers fit; per batch one kernels.segfix_shift call (csrc/segfix.hip)
refines the finished prediction of whatever test.mode inside every image's unpadded region -- the script's grid_sample blend of class
INDICES, in its fp32 order, rounded half to even -- and returns the dataset ids and the number of changed pixels with it. label/ and
the `Test mIoU` line stay as they are; the refined maps go to <out_dir>/label_w_segfix/, a second confusion matrix feeds a `Test mIoU
(SegFix)` line, and with test.evaluator a second CityscapesScore writes evaluationResults_w_segfix/. Refused by name: size_mode
diverse_size, a data.label_list other than the 19 Cityscapes train classes the script hard-codes, a missing directory, an image
without an offset file, an array that is not [h, w, 2] of the image's size, non-numeric or with non-finite values. Outside: predicting
the offsets (segfix_hrnet, tester_offset.py), segfix_instance.py and segfix_ade20k.py.

Outside the accelerated path, refused by name: crf_ss_test, the offset path; align_method scale_and_pad / only_scale
(border_size is scaled there and the final cubic resize is a real one) and size_mode max_size / multi_size; under diverse_size a
pad_mode other than an explicit pad_right_down (the reference's crop at :180 is top-left, so only right / down padding makes its
result the image's prediction; an absent key means `random`, collate.py:114) and the sliding-crop modes (the reference does not
support them on differing sizes, :353, :507). The colour `vis/` output is not written."""
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from contrastiveseg_amd import kernels as K
from contrastiveseg_amd.lib.metrics import cityscapes_score as CS
from contrastiveseg_amd.lib.metrics.running_score import RunningScore
from contrastiveseg_amd.lib.utils.distributed import get_rank
from contrastiveseg_amd.lib.utils.tools.logger import Logger as Log

SUPPORTED_MODES = ('ss_test', 'ms_test', 'sscrop_test', 'mscrop_test', 'ms_test_depth')
CROP_MODES = ('sscrop_test', 'mscrop_test')
REFUSED_MODES = ('crf_ss_test',)
DEPTH_MAX, DEPTH_POWER_BASE = 63, 0.8      # MAX_DEPTH, POWER_BASE of the reference's fuse_with_depth (:448-449)


def check_config(configer):
    """Everything that can be refused before a model is built. -> (mode, scales, weights or None)."""
    if configer.exists('data', 'use_offset') and configer.get('data', 'use_offset'):
        raise NotImplementedError('data.use_offset {!r}: the offset path (offset_test) is outside the accelerated test phase'
                                  .format(configer.get('data', 'use_offset')))
    mode = configer.get('test', 'mode') if configer.exists('test', 'mode') else 'ss_test'
    if mode not in SUPPORTED_MODES:
        if mode in REFUSED_MODES:
            raise NotImplementedError('test.mode {!r} is outside the accelerated test phase; supported: {}'
                                      .format(mode, SUPPORTED_MODES))
        raise NotImplementedError('test.mode {!r} is not a test mode; supported: {}'.format(mode, SUPPORTED_MODES))
    resolve_depth_dir(configer, mode)
    scales, weights = [1.0], None
    if mode in ('ms_test', 'mscrop_test', 'ms_test_depth'):
        scales = list(configer.get('test', 'scale_search')) if configer.exists('test', 'scale_search') else [1.0]
        # (mscrop_test takes no weights: reference :511-522; ms_test_depth neither: :434-441)
        if mode == 'ms_test' and configer.exists('test', 'scale_weights') and configer.get('test', 'scale_weights') is not None:
            weights = list(configer.get('test', 'scale_weights'))
            if len(weights) != len(scales):
                raise ValueError('test.scale_weights has {} entries for the {} scales of test.scale_search'
                                 .format(len(weights), len(scales)))
        if not 1 <= len(scales) <= K.MS_MAX_TERMS:
            raise ValueError('test.scale_search has {} scales; 1 to {} are supported'.format(len(scales), K.MS_MAX_TERMS))
    if configer.exists('test', 'data_transformer'):
        dt = configer.get('test', 'data_transformer')
        if dt.get('size_mode', 'fix_size') not in ('fix_size', 'diverse_size') or dt.get('align_method', 'only_pad') != 'only_pad':
            raise NotImplementedError('test.data_transformer {}: only size_mode fix_size / diverse_size with align_method only_pad is '
                                      'implemented (the final resize to the original size is the identity there; it is not '
                                      'approximated)'.format(dt))
        if dt.get('size_mode', 'fix_size') == 'diverse_size':
            if mode == 'ms_test_depth':
                raise NotImplementedError('test.mode {!r} under test.data_transformer size_mode diverse_size: the depth-aware fusion '
                                          'takes batches of equal-sized images only, as in the reference'.format(mode))
            if mode in CROP_MODES:
                raise NotImplementedError('test.mode {!r} under test.data_transformer size_mode diverse_size: the sliding-crop modes do '
                                          'not support images of differing sizes, as in the reference'.format(mode))
            if dt.get('pad_mode') != 'pad_right_down':
                raise NotImplementedError("test.data_transformer {}: size_mode diverse_size needs pad_mode 'pad_right_down' stated "
                                          'explicitly: the prediction of a padded image is cropped top-left, so only right / down '
                                          "padding makes it the image's prediction, and an absent pad_mode means 'random'".format(dt))
    flip_swap_perm(configer, mode)
    resolve_evaluator(configer)
    resolve_segfix(configer)
    return mode, scales, weights


EVALUATORS = ('cityscapes',)
IMG_EXT = ('.jpg', '.jpeg', '.png', '.bmp')
SEGFIX_LABEL_DIR = 'label_w_segfix'                        # the reference script's directory name
SEGFIX_RESULT_DIR = 'evaluationResults_w_segfix'


def resolve_segfix(configer):
    """test.segfix_offset_dir / test.segfix_scale -- this project's own keys, like test.depth_dir: the SegFix refinement of the
    reference's scripts/cityscapes/segfix.py inside the test phase. -> (offset_dir, scale), or (None, None) without the key.
    Everything the mode needs is checked here, before a model is built: the size mode, data.label_list, the directory, and --
    where the image directory is known -- one offset file per image."""
    from contrastiveseg_amd.lib.datasets import segfix_offsets as SO
    offset_dir = configer.get('test', 'segfix_offset_dir') if configer.exists('test', 'segfix_offset_dir') else None
    if offset_dir is None:
        return None, None
    if not isinstance(offset_dir, str) or not offset_dir:
        raise ValueError('test.segfix_offset_dir {!r}: expected a directory name'.format(offset_dir))
    scale = configer.get('test', 'segfix_scale') if configer.exists('test', 'segfix_scale') else 2.0
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not np.isfinite(scale):
        raise ValueError('test.segfix_scale {!r}: expected a finite number'.format(scale))
    if is_ragged(configer):
        raise NotImplementedError('test.segfix_offset_dir under test.data_transformer size_mode diverse_size: the refinement takes '
                                  'batches of equal-sized images only')
    label_list = list(configer.get('data', 'label_list')) if configer.exists('data', 'label_list') else None
    if label_list != SO.LABEL_LIST:
        raise NotImplementedError('test.segfix_offset_dir with data.label_list {}: the refinement is the Cityscapes script of the '
                                  'reference, which hard-codes the label list {}'.format(label_list, SO.LABEL_LIST))
    if not os.path.isdir(offset_dir):
        raise FileNotFoundError('test.segfix_offset_dir {} does not exist'.format(offset_dir))
    image_dir = image_dir_of(configer)
    if image_dir is not None and os.path.isdir(image_dir):           # (otherwise the loader names the missing image directory)
        for fname in sorted(os.listdir(image_dir)):
            stem, ext = os.path.splitext(fname)
            if ext.lower() in IMG_EXT and SO.find_offset_file(offset_dir, stem) is None:
                raise FileNotFoundError('test.segfix_offset_dir {} has neither {}.mat nor {}.npy'.format(offset_dir, stem, stem))
    return offset_dir, float(scale)


def image_dir_of(configer):
    """test.test_dir, or <data.data_dir>/val/image as DataLoader.get_testloader resolves it; None when neither key is set."""
    if configer.exists('test', 'test_dir') and configer.get('test', 'test_dir'):
        return configer.get('test', 'test_dir')
    if configer.exists('data', 'data_dir') and configer.get('data', 'data_dir'):
        data_dir = configer.get('data', 'data_dir')
        return os.path.join(data_dir[0] if isinstance(data_dir, (list, tuple)) else data_dir, 'val', 'image')
    return None


def resolve_evaluator(configer):
    """test.evaluator -- this project's own key, like test.depth_dir: 'cityscapes' adds the pixel-level Cityscapes evaluation to the
    test phase. -> (evaluator, instance_dir), or (None, None) without the key. Everything the mode needs is checked here, before a model
    is built: the name, the size mode, data.label_list, and -- where the image directory is known -- the label and instance
    directories with one file per image."""
    name = configer.get('test', 'evaluator') if configer.exists('test', 'evaluator') else None
    if name is None:
        return None, None
    if name not in EVALUATORS:
        raise NotImplementedError('test.evaluator {!r} is not an evaluator; supported: {}'.format(name, EVALUATORS))
    if is_ragged(configer):
        raise NotImplementedError('test.evaluator {!r} under test.data_transformer size_mode diverse_size: the evaluation takes '
                                  'batches of equal-sized images only'.format(name))
    if configer.exists('data', 'label_list'):
        CS.check_label_list(list(configer.get('data', 'label_list')))
    elif configer.get('data', 'num_classes') > CS.NUM_LABELS:
        raise ValueError('data.num_classes {} without data.label_list: under test.evaluator {!r} the predictions must be Cityscapes '
                         'label ids 0..{}'.format(configer.get('data', 'num_classes'), name, CS.NUM_LABELS - 1))
    image_dir = image_dir_of(configer)
    instance_dir = configer.get('test', 'instance_dir') if configer.exists('test', 'instance_dir') else None
    if instance_dir is not None and (not isinstance(instance_dir, str) or not instance_dir):
        raise ValueError('test.instance_dir {!r}: expected a directory name'.format(instance_dir))
    if image_dir is None or not os.path.isdir(image_dir):
        return name, instance_dir                          # the loader names the missing image directory
    parent = os.path.dirname(os.path.normpath(image_dir))
    label_dir = os.path.join(parent, 'label')
    if instance_dir is None:
        instance_dir = os.path.join(parent, 'instance')
    if not os.path.isdir(label_dir):
        raise FileNotFoundError('test.evaluator {!r} needs the raw label ids of every image: the label directory {} does not exist'
                                .format(name, label_dir))
    if not os.path.isdir(instance_dir):
        raise FileNotFoundError('test.evaluator {!r} needs the instance ids of every image: test.instance_dir {} does not exist'
                                .format(name, instance_dir))
    for fname in sorted(os.listdir(image_dir)):
        stem, ext = os.path.splitext(fname)
        if ext.lower() not in IMG_EXT:
            continue
        if not os.path.exists(os.path.join(label_dir, stem + '.png')):
            raise FileNotFoundError('test.evaluator {!r}: the label directory {} has no {}.png'.format(name, label_dir, stem))
        if not os.path.exists(os.path.join(instance_dir, stem + '.png')):
            raise FileNotFoundError('test.evaluator {!r}: test.instance_dir {} has no {}.png'.format(name, instance_dir, stem))
    return name, instance_dir


def flip_swap_perm(configer, mode=None):
    """test.flip_swap_pair -- this project's own key, the reference has none: its tester mirrors without swapping channels
    (:345-349, :380-421), also for LIP, and that stays the default -- a list of [a, b] class pairs that trade places under the
    mirror. -> the channel permutation ms_test hands to kernels.ms_fuse_argmax / ms_fuse_argmax_ragged (output class k reads class
    perm[k] of the mirrored pass), or None without the key. Pairs that share a class do not describe an exchange of channels and
    are refused."""
    pairs = configer.get('test', 'flip_swap_pair') if configer.exists('test', 'flip_swap_pair') else None
    if not pairs:
        return None
    if mode is None:
        mode = configer.get('test', 'mode') if configer.exists('test', 'mode') else 'ss_test'
    if mode in CROP_MODES:
        raise NotImplementedError('test.flip_swap_pair together with test.mode {!r}: the sliding-crop kernel takes no channel '
                                  'permutation; use ss_test / ms_test'.format(mode))
    if mode == 'ms_test_depth':
        raise NotImplementedError('test.flip_swap_pair together with test.mode {!r}: the depth-weighted kernel takes no channel '
                                  'permutation; use ss_test / ms_test'.format(mode))
    n = configer.get('data', 'num_classes')
    perm = list(range(n))
    for pair in pairs:
        if not isinstance(pair, (list, tuple)) or len(pair) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in pair):
            raise ValueError('test.flip_swap_pair entry {!r}: expected two class indices [a, b]'.format(pair))
        if not all(0 <= v < n for v in pair):
            raise ValueError('test.flip_swap_pair entry {!r} lies outside the {} classes of data.num_classes'.format(pair, n))
        perm[pair[0]], perm[pair[1]] = pair[1], pair[0]
    if sorted(perm) != list(range(n)):
        raise ValueError('test.flip_swap_pair {!r} is not a permutation of the classes: a class is mentioned by more than one pair'
                         .format(pairs))
    return perm


def is_ragged(configer):
    """True when the test loader yields list batches (images of differing sizes, each at its own padded size)."""
    return bool(configer.exists('test', 'data_transformer')
                and configer.get('test', 'data_transformer').get('size_mode', 'fix_size') == 'diverse_size')


def tile_starts(total, crop):
    """Tile starts along one axis, the reference's _decide_intersection (:525-533) with its stride = the crop length:
    min(i * crop, total - crop) for i < ceil(total / crop). Every index is covered by one or two tiles."""
    if crop < 1 or total < crop:
        raise ValueError('a canvas of {} cannot be tiled with crops of {}'.format(total, crop))
    return [min(i * crop, total - crop) for i in range(K.crop_tiles(total, crop))]


def resolve_crop_size(configer, mode):
    """test.crop_size = [crop_h, crop_w] of the sliding-crop modes (crop_size[0] is the height, as the reference indexes it), or None
    for the other modes."""
    if mode not in CROP_MODES:
        return None
    crop = configer.get('test', 'crop_size') if configer.exists('test', 'crop_size') else None
    if crop is None:
        raise NotImplementedError('test.mode {!r} needs test.crop_size = [crop_h, crop_w]; it is not set'.format(mode))
    if not isinstance(crop, (list, tuple)) or len(crop) != 2 or not all(isinstance(c, int) and c > 0 for c in crop):
        raise ValueError('test.crop_size {!r}: expected two positive integers [crop_h, crop_w]'.format(crop))
    return int(crop[0]), int(crop[1])


def resolve_depth_dir(configer, mode):
    """test.depth_dir of ms_test_depth -- this project's own key in place of the reference's hard-coded stereo paths (:450-453): the
    directory of the uint16 disparity PNGs, <depth_dir>/<name>.png -- or None for the other modes."""
    if mode != 'ms_test_depth':
        return None
    depth_dir = configer.get('test', 'depth_dir') if configer.exists('test', 'depth_dir') else None
    if depth_dir is None:
        raise NotImplementedError('test.mode {!r} needs test.depth_dir = the directory of the uint16 disparity PNGs; it is not set'
                                  .format(mode))
    if not isinstance(depth_dir, str) or not depth_dir:
        raise ValueError('test.depth_dir {!r}: expected a directory name'.format(depth_dir))
    return depth_dir


def depth_fusion_tables(scales):
    """The depth arithmetic of the reference's fuse_with_depth (:459-470), its float64 numpy statements evaluated over every uint16
    disparity value -> (lut uint8 [65536], table float32 [S, nbins]): lut[s] is the depth bin of disparity s, table[i, b] the weight
    float32(0.8 ** |b - idx(i)|) of scale i in bin b, idx(i) the FIRST index j with scales[j] == scales[i] (_locate_scale_index,
    :477-482). Disparity 0 divides by zero: inf, clipped to 63, the last bin. This is the only place the arithmetic lives; the device
    looks both tables up."""
    S = len(scales)
    if not 1 <= S <= K.MS_MAX_TERMS:
        raise ValueError('{} scales; 1 to {} are supported'.format(S, K.MS_MAX_TERMS))
    stereo_map = np.arange(65536, dtype=np.uint16)
    with np.errstate(divide='ignore'):
        depth_map = stereo_map / 256.0
        depth_map = 0.5 / depth_map
        depth_map = 500 * depth_map
    depth_map = np.clip(depth_map, 0, DEPTH_MAX)
    depth_map = depth_map // (DEPTH_MAX // S)
    nbins = int(depth_map.max()) + 1
    table = np.empty((S, nbins), dtype=np.float32)
    for i, scale in enumerate(scales):
        scale_index = next((j for j, s in enumerate(scales) if s == scale), 0)
        weight_map = np.abs(np.arange(nbins, dtype=np.float64) - scale_index)
        table[i] = np.power(DEPTH_POWER_BASE, weight_map)           # float64 -> float32, the reference's .type(FloatTensor)
    return depth_map.astype(np.uint8), table


def load_disparity(path):
    """-> the uint16 [h, w] array of a single-channel 16-bit PNG (cv2.imread(path, -1) of the reference, :459); anything else is
    refused by name."""
    from PIL import Image
    with Image.open(path) as img:
        if not img.mode.startswith('I;16'):
            raise ValueError('{}: a disparity map must be a single-channel 16-bit image, this one has mode {!r}'.format(path, img.mode))
        return np.asarray(img).astype(np.uint16, copy=False)


def check_canvas(input_size, crop, scale):
    """-> the canvas (int(H * scale), int(W * scale)) of one sliding-crop scale; ValueError when a crop does not fit into it (the
    reference runs into an IndexError there)."""
    hs, ws = int(input_size[0] * scale), int(input_size[1] * scale)
    if hs < crop[0] or ws < crop[1]:
        raise ValueError('scale {}: the canvas {} x {} of a {} x {} input is smaller than the crop {} x {}'
                         .format(scale, hs, ws, input_size[0], input_size[1], crop[0], crop[1]))
    return hs, ws


def dataset_id_lut(configer):
    """uint8 [256]: train id -> dataset id, the inverse of the loader's label encoding (reference :189-197: reduce_zero_label
    adds one, then label_list relabels; ids that label_list does not cover become 0)."""
    ids = np.arange(256, dtype=np.int64)
    if configer.exists('data', 'reduce_zero_label') and configer.get('data', 'reduce_zero_label'):
        ids = (ids + 1) & 255
    if configer.exists('data', 'label_list'):
        label_list = configer.get('data', 'label_list')
        out = np.zeros(256, dtype=np.int64)
        for i in range(configer.get('data', 'num_classes')):
            out[ids == i] = label_list[i]
        ids = out
    return ids.astype(np.uint8)


def to_dataset_ids(pred, configer):
    """pred: uint8 array of train ids -> uint8 array of dataset ids."""
    return dataset_id_lut(configer)[np.asarray(pred, dtype=np.uint8)]


class Tester(object):
    def __init__(self, configer, seg_net=None, test_loader=None):
        self.configer = configer
        self.mode, self.scales, self.weights = check_config(configer)
        self.crop_size = resolve_crop_size(configer, self.mode)
        self.perm = flip_swap_perm(configer, self.mode)
        self.depth_dir = resolve_depth_dir(configer, self.mode)
        if self.mode == 'mscrop_test' and configer.exists('test', 'scale_weights') and configer.get('test', 'scale_weights') is not None:
            Log.warn('test.scale_weights is ignored in mscrop_test, as in the reference')
        from contrastiveseg_amd.lib.models.model_manager import ModelManager
        from contrastiveseg_amd.segmentor.tools.module_runner import ModuleRunner
        self.module_runner = ModuleRunner(configer)
        self.device = self.module_runner.device()
        if seg_net is None:
            seg_net = ModelManager(configer).semantic_segmentor()
            if configer.exists('network', 'channels_last') and configer.get('network', 'channels_last'):
                seg_net = seg_net.to(memory_format=torch.channels_last)
            if not (configer.exists('network', 'resume') and configer.get('network', 'resume')):
                Log.warn('network.resume is not set: testing a randomly initialised model')
            seg_net = self.module_runner.load_net(seg_net)
        self.seg_net = seg_net
        self.seg_net.eval()
        self.save_dir = configer.get('test', 'out_dir') if configer.exists('test', 'out_dir') else None
        self.save_prob = bool(configer.exists('test', 'save_prob') and configer.get('test', 'save_prob'))
        self.test_loader = test_loader
        self.running_score = RunningScore(configer, ignore_index=-1)
        self.lut = dataset_id_lut(configer)
        self.last_miou = None
        self.evaluator = resolve_evaluator(configer)[0]
        self.cs_score = CS.CityscapesScore(self.lut, self.device) if self.evaluator == 'cityscapes' else None
        self.last_cityscapes = None                        # (result dictionary, pixel accuracy) of the last test()
        self.segfix_dir, self.segfix_scale = resolve_segfix(configer)
        self.segfix_lut = self.running_score_segfix = self.cs_score_segfix = None
        self.last_miou_segfix = self.last_cityscapes_segfix = None             # the same two for the refined maps
        if self.segfix_dir is not None:
            self.segfix_lut = torch.from_numpy(self.lut).to(self.device)
            self.running_score_segfix = RunningScore(configer, ignore_index=-1)
            self.cs_score_segfix = CS.CityscapesScore(self.lut, self.device) if self.evaluator == 'cityscapes' else None
        self.depth_tables = self.depth_lut = self.depth_table = None
        if self.mode == 'ms_test_depth':                   # once per Tester: host tables, device copies
            self.depth_tables = depth_fusion_tables(self.scales)
            self.depth_lut = torch.from_numpy(self.depth_tables[0]).to(self.device)
            self.depth_table = torch.from_numpy(self.depth_tables[1]).to(self.device)

    # ------------------------------------------------------------------------------------------------------
    def _coarse(self, x):
        out = self.seg_net(x, is_eval=True)
        if isinstance(out, dict):
            out = out['seg']
        elif isinstance(out, (list, tuple)):
            out = out[-1]
        return out

    @staticmethod
    def _scaled(inputs, scale):
        h, w = inputs.shape[-2:]
        return F.interpolate(inputs, size=(int(h * scale), int(w * scale)), mode='bilinear', align_corners=True)

    @torch.no_grad()
    def _fuse(self, terms, inputs, want_fused):
        h, w = inputs.shape[-2:]
        mirrored = any(b is not None for _, b, _ in terms)          # test.flip_swap_pair acts on the mirrored pass only
        return K.ms_fuse_argmax(terms, h, w, want_fused=want_fused, perm=self.perm if mirrored else None)

    @torch.no_grad()
    def _fuse_ragged(self, inputs, scales, weights, flip, borders, want_fused):
        """The list branches (:328-341, :400-421): per image and scale one forward pass at batch 1, one more on the flip of the PADDED
        tensor; only coarse maps are kept; one kernels.ms_fuse_argmax_ragged call for the batch. borders: [(h, w)] per image, the
        unpadded top-left region that is scored (default: the whole padded image)."""
        if borders is not None and len(borders) != len(inputs):
            raise ValueError('{} borders for {} images'.format(len(borders), len(inputs)))
        images = []
        for k, x in enumerate(inputs):
            if x.dim() != 4 or x.shape[0] != 1:
                raise ValueError('image {} of a list batch is {}, expected [1, 3, H, W]'.format(k, tuple(x.shape)))
            mirrored = torch.flip(x, dims=[3]) if flip else None
            terms = []
            for i, scale in enumerate(scales):
                a = self._coarse(self._scaled(x, scale))
                b = self._coarse(self._scaled(mirrored, scale)) if flip else None
                terms.append((a, b, 1.0 if weights is None else weights[i]))
            padded = tuple(x.shape[-2:])
            images.append((terms, padded, padded if borders is None else (int(borders[k][0]), int(borders[k][1]))))
        return K.ms_fuse_argmax_ragged(images, want_fused=want_fused, perm=self.perm if flip else None)

    @torch.no_grad()
    def ss_test(self, inputs, scale=1, want_fused=False, borders=None):
        """reference :310-327 + the argmax: -> pred u8 [B,H,W], or (pred, fused) when want_fused. A list of [1,3,Hp,Wp] tensors
        (:328-341) -> kernels.RaggedScores over each image's border."""
        self.seg_net.eval()
        if isinstance(inputs, (list, tuple)):
            return self._fuse_ragged(inputs, [scale], None, False, borders, want_fused)
        return self._fuse([(self._coarse(self._scaled(inputs, scale)), None, 1.0)], inputs, want_fused)

    @torch.no_grad()
    def ms_test(self, inputs, want_fused=False, flip=True, borders=None):
        """reference :380-398 + the argmax: one forward per scale and one more on the mirrored input; only the coarse maps are kept.
        flip=False leaves the mirrored pass out (ms_test of one scale is then ss_test). A list of [1,3,Hp,Wp] tensors (:400-421) ->
        kernels.RaggedScores over each image's border."""
        self.seg_net.eval()
        if isinstance(inputs, (list, tuple)):
            return self._fuse_ragged(inputs, self.scales, self.weights, flip, borders, want_fused)
        mirrored = torch.flip(inputs, dims=[3]) if flip else None
        terms = []
        for i, scale in enumerate(self.scales):
            a = self._coarse(self._scaled(inputs, scale))
            b = self._coarse(self._scaled(mirrored, scale)) if flip else None
            terms.append((a, b, 1.0 if self.weights is None else self.weights[i]))
        return self._fuse(terms, inputs, want_fused)

    def _disparity(self, names, size, borders, pad_offsets):
        """uint16 [B,H,W]: every image's disparity map at its pad_offset (left, up); zero -- infinitely far -- in the padding."""
        H, W = size
        stereo = np.zeros((len(names), H, W), dtype=np.uint16)
        for k, name in enumerate(names):
            bh, bw = (H, W) if borders is None else (int(borders[k][0]), int(borders[k][1]))
            x0, y0 = (0, 0) if pad_offsets is None else (int(pad_offsets[k][0]), int(pad_offsets[k][1]))
            path = os.path.join(self.depth_dir, '{}.png'.format(name))
            disp = load_disparity(path)
            if disp.shape != (bh, bw):
                raise ValueError('{}: the disparity map is {} x {}, the image {} x {}; the reference resizes the weight map with '
                                 'cv2.resize, which is the identity only for equal sizes and is not approximated'
                                 .format(path, disp.shape[0], disp.shape[1], bh, bw))
            stereo[k, y0:y0 + bh, x0:x0 + bw] = disp
        return stereo

    @torch.no_grad()
    def ms_test_depth(self, inputs, names, want_fused=False, borders=None, pad_offsets=None):
        """reference :426-475 + the argmax: the forwards of ms_test with flips, the per-scale weight per pixel from the disparity maps
        <test.depth_dir>/<name>.png. borders [(h, w)] and pad_offsets [(left, up)] per image say where the unpadded image lies in the
        input (default: all of it). One upload, kernels.lut_u16_u8, one kernels.ms_fuse_argmax(pixel_weights=...)."""
        self.seg_net.eval()
        if self.depth_table is None:
            raise RuntimeError('ms_test_depth on a Tester of test.mode {!r}: the depth tables are built for ms_test_depth'
                               .format(self.mode))
        if isinstance(inputs, (list, tuple)):
            raise NotImplementedError('ms_test_depth takes a batch of equal-sized images, not a list, as in the reference')
        if len(names) != inputs.shape[0]:
            raise ValueError('{} names for {} images'.format(len(names), inputs.shape[0]))
        h, w = inputs.shape[-2:]
        stereo = self._disparity(names, (h, w), borders, pad_offsets)          # before the first forward pass
        mirrored = torch.flip(inputs, dims=[3])
        terms = [(self._coarse(self._scaled(inputs, scale)), self._coarse(self._scaled(mirrored, scale)), 1.0) for scale in self.scales]
        # (int16 carries the bits; the look-up reads them as uint16)
        bins = K.lut_u16_u8(torch.from_numpy(stereo.view(np.int16)).to(self.device), self.depth_lut)
        return K.ms_fuse_argmax(terms, h, w, want_fused=want_fused, pixel_weights=(bins, self.depth_table))

    def _crop_stack(self, scaled, crop):
        """The coarse outputs of the net on the reference's tiles of `scaled`, height-major (:364-373) -> [ny*nx,B,K,hc,wc]."""
        ch, cw = crop
        stack, t = None, 0
        ys, xs = tile_starts(scaled.shape[2], ch), tile_starts(scaled.shape[3], cw)
        for y0 in ys:
            for x0 in xs:
                out = self._coarse(scaled[:, :, y0:y0 + ch, x0:x0 + cw].contiguous())
                if stack is None:
                    stack = torch.empty((len(ys) * len(xs),) + tuple(out.shape), dtype=out.dtype, device=out.device)
                stack[t].copy_(out)
                t += 1
        return stack

    def _crop_term(self, inputs, mirrored, crop, scale):
        """One scale of mscrop_test (:511-522): a plain term below 1, a tiled term from 1 on; mirrored=None leaves the flip out."""
        if scale < 1:
            return (self._coarse(self._scaled(inputs, scale)), None if mirrored is None else self._coarse(self._scaled(mirrored, scale)))
        canvas = check_canvas(inputs.shape[-2:], crop, scale)
        return (self._crop_stack(self._scaled(inputs, scale), crop),
                None if mirrored is None else self._crop_stack(self._scaled(mirrored, scale), crop), canvas, crop)

    @torch.no_grad()
    def sscrop_test(self, inputs, crop_size, scale=1, want_fused=False):
        """reference :351-378 + the argmax: -> pred u8 [B,H,W], or (pred, fused) when want_fused. As in the reference, the scale is
        taken as a sliding-crop scale whatever its value."""
        self.seg_net.eval()
        crop = (int(crop_size[0]), int(crop_size[1]))
        canvas = check_canvas(inputs.shape[-2:], crop, scale)
        h, w = inputs.shape[-2:]
        return K.crop_fuse_argmax([(self._crop_stack(self._scaled(inputs, scale), crop), None, canvas, crop)], h, w, want_fused=want_fused)

    @torch.no_grad()
    def mscrop_test(self, inputs, crop_size, want_fused=False, flip=True):
        """reference :505-523 + the argmax: per scale of test.scale_search ss_test below 1 and sscrop_test from 1 on, each once more on
        the mirrored input; test.scale_weights plays no part. Only coarse maps are kept."""
        self.seg_net.eval()
        crop = (int(crop_size[0]), int(crop_size[1]))
        for scale in self.scales:          # before the first forward pass
            if scale >= 1:
                check_canvas(inputs.shape[-2:], crop, scale)
        mirrored = torch.flip(inputs, dims=[3]) if flip else None
        terms = [self._crop_term(inputs, mirrored, crop, scale) for scale in self.scales]
        h, w = inputs.shape[-2:]
        return K.crop_fuse_argmax(terms, h, w, want_fused=want_fused)

    def _predict(self, inputs, borders=None, batch=None):
        if self.mode == 'ms_test_depth':
            if batch is None or isinstance(inputs, (list, tuple)):      # check_config has refused size_mode diverse_size
                raise NotImplementedError('test.mode ms_test_depth on a list batch: images of differing sizes are not supported')
            return self.ms_test_depth(inputs, batch['name'], self.save_prob, [(bh, bw) for bw, bh in batch['border_size']],
                                      batch.get('pad_offset'))
        if isinstance(inputs, (list, tuple)):              # check_config has refused the sliding-crop modes
            if self.mode == 'ms_test':
                return self.ms_test(inputs, self.save_prob, borders=borders)
            return self.ss_test(inputs, 1, self.save_prob, borders=borders)
        if self.mode == 'ms_test':
            return self.ms_test(inputs, self.save_prob)
        if self.mode == 'sscrop_test':
            return self.sscrop_test(inputs, self.crop_size, 1, self.save_prob)
        if self.mode == 'mscrop_test':
            return self.mscrop_test(inputs, self.crop_size, self.save_prob)
        return self.ss_test(inputs, 1, self.save_prob)

    # ------------------------------------------------------------------------------------------------------
    def _loader(self):
        if self.test_loader is None:
            from contrastiveseg_amd.lib.datasets.data_loader import DataLoader
            self.test_loader = DataLoader(self.configer, self.device).get_testloader()
            check_config(self.configer)                    # the loader may have taken test.data_transformer from val's
        return self.test_loader

    def _test_ragged(self, batch, confusion, label_dir, n_img):
        """One list batch: predictions over each image's own h x w (reference :169-189: the top-left crop; the resize to the original
        size is the identity), one device-to-host copy of the packed bytes, the confusion matrix on the packed buffers. -> whether
        the batch was scored."""
        from PIL import Image
        inputs = [x if x.device == self.device else x.to(self.device, non_blocking=True) for x in batch['img']]
        if any(tuple(o) != (0, 0) for o in batch.get('pad_offset', [])):
            raise RuntimeError('a list batch with pad_offset {}: only right / down padding is scored'.format(batch['pad_offset']))
        borders = [(int(bh), int(bw)) for bw, bh in batch['border_size']]
        out = self._predict(inputs, borders)
        labels = batch.get('labelmap')
        if labels is not None:
            flat = torch.cat([lab.to(self.device)[0, :h, :w].reshape(-1) for lab, (h, w) in zip(labels, borders)])
            K.confusion_update(out.pred, flat, confusion, ignore_index=-1)
        pred_np, off = out.pred.cpu().numpy(), 0
        for k, name in enumerate(batch['name']):
            h, w = borders[k]
            Image.fromarray(self.lut[pred_np[off:off + h * w].reshape(h, w)]).save(os.path.join(label_dir, '{}.png'.format(name)))
            off += h * w
            if self.save_prob:
                np.save(os.path.join(self.save_dir, 'prob', '{}.npy'.format(name)),
                        torch.softmax(out.fuseds[k].permute(1, 2, 0), dim=-1).cpu().numpy())
            Log.info('{:4d} label map generated'.format(n_img + k + 1))
        return labels is not None

    @staticmethod
    def _records(batch):
        """Every image's unpadded region (x0, y0, bw, bh) in the batch."""
        offsets = batch.get('pad_offset') or [(0, 0)] * len(batch['border_size'])
        return [(int(x0), int(y0), int(bw), int(bh)) for (x0, y0), (bw, bh) in zip(offsets, batch['border_size'])]

    def _cityscapes_update(self, pred, batch, score=None):
        """One batch of the Cityscapes evaluation: the prediction as the scoring kernel wrote it (score: the CityscapesScore that takes
        it, default the unrefined one), the loader's raw label and instance maps, and every image's unpadded region."""
        for key in ('labelmap_raw', 'instancemap'):
            if key not in batch:
                raise RuntimeError('test.evaluator {!r}: the batch carries no {!r}; the test loader yields it when the key is set'
                                   .format(self.evaluator, key))
        score = self.cs_score if score is None else score
        score.update(pred, batch['labelmap_raw'].to(self.device), batch['instancemap'].to(self.device), self._records(batch))

    def _segfix(self, pred, batch):
        """One batch of the SegFix refinement -> (refined train ids, refined dataset ids, changed pixels per image), all on the device."""
        if 'segfix_offset' not in batch:
            raise RuntimeError("test.segfix_offset_dir: the batch carries no 'segfix_offset'; the test loader yields it when the key is "
                               'set')
        return K.segfix_shift(pred, batch['segfix_offset'].to(self.device), self._records(batch), self.segfix_scale, self.segfix_lut)

    @torch.no_grad()
    def test(self, data_loader=None):
        from PIL import Image
        if not self.save_dir or self.save_dir == 'none':
            raise RuntimeError('test.out_dir (--out_dir) is not set')
        loader = self._loader() if data_loader is None else data_loader
        label_dir = os.path.join(self.save_dir, 'label')
        os.makedirs(label_dir, exist_ok=True)
        if self.save_prob:
            os.makedirs(os.path.join(self.save_dir, 'prob'), exist_ok=True)
        Log.info('save dir {}'.format(self.save_dir))
        self.running_score.reset()
        if self.cs_score is not None:
            self.cs_score.reset()
        K_cls = self.configer.get('data', 'num_classes')
        confusion = torch.zeros(K_cls, K_cls, dtype=torch.int64, device=self.device)
        segfix, confusion_sf = self.segfix_dir is not None, None
        if segfix:
            segfix_dir = os.path.join(self.save_dir, SEGFIX_LABEL_DIR)
            os.makedirs(segfix_dir, exist_ok=True)
            self.running_score_segfix.reset()
            confusion_sf = torch.zeros_like(confusion)
            if self.cs_score_segfix is not None:
                self.cs_score_segfix.reset()
        start, n_img, scored = time.time(), 0, False
        for batch in loader:
            inputs = batch['img']
            if isinstance(inputs, (list, tuple)):
                if self.cs_score is not None:              # check_config has refused size_mode diverse_size
                    raise NotImplementedError('test.evaluator {!r} on a list batch: images of differing sizes are not supported'
                                              .format(self.evaluator))
                if segfix:
                    raise NotImplementedError('test.segfix_offset_dir on a list batch: images of differing sizes are not supported')
                scored = self._test_ragged(batch, confusion, label_dir, n_img) or scored
                n_img += len(inputs)
                continue
            if inputs.device != self.device:
                inputs = inputs.to(self.device, non_blocking=True)
            out = self._predict(inputs, batch=batch)
            pred, fused = out if self.save_prob else (out, None)
            labels = batch.get('labelmap')
            if labels is not None:
                # pixels outside an image's unpadded region carry the ignore label (-1): the loader's padding
                K.confusion_update(pred, labels.to(self.device), confusion, ignore_index=-1)
                scored = True
            if self.cs_score is not None:
                self._cityscapes_update(pred, batch)
            if segfix:                                     # the finished prediction of whatever test.mode, refined on the device
                refined, refined_ids, changed = self._segfix(pred, batch)
                if labels is not None:
                    K.confusion_update(refined, labels.to(self.device), confusion_sf, ignore_index=-1)
                if self.cs_score_segfix is not None:
                    self._cityscapes_update(refined, batch, self.cs_score_segfix)
                ids_np, changed = refined_ids.cpu().numpy(), changed.cpu().tolist()
                for k, (name, (x0, y0, bw, bh)) in enumerate(zip(batch['name'], self._records(batch))):
                    Image.fromarray(ids_np[k, y0:y0 + bh, x0:x0 + bw]).save(os.path.join(segfix_dir, '{}.png'.format(name)))
                    Log.info('SegFix {}: {} of {} pixels changed'.format(name, changed[k], bw * bh))
            pred_np = pred.cpu().numpy()
            for k, name in enumerate(batch['name']):
                bw, bh = batch['border_size'][k]
                x0, y0 = batch['pad_offset'][k] if 'pad_offset' in batch else (0, 0)
                n_img += 1
                Image.fromarray(self.lut[pred_np[k, y0:y0 + bh, x0:x0 + bw]]).save(os.path.join(label_dir, '{}.png'.format(name)))
                if self.save_prob:
                    logits = fused[k, :, y0:y0 + bh, x0:x0 + bw].permute(1, 2, 0)
                    np.save(os.path.join(self.save_dir, 'prob', '{}.npy'.format(name)), torch.softmax(logits, dim=-1).cpu().numpy())
                Log.info('{:4d} label map generated'.format(n_img))
        Log.info('Test Time {:.3f}s'.format(time.time() - start))
        self.running_score.update_from_hist(confusion)
        self.running_score.reduce_scores()
        if scored or float(self.running_score.reduced_confusion_matrix.sum()) > 0:
            self.last_miou = float(self.running_score.get_mean_iou())
            if get_rank() == 0:
                Log.info('Test mIoU {:.6f}\tPixel acc {:.6f}'.format(self.last_miou, float(self.running_score.get_pixel_acc())))
        if self.cs_score is not None:
            self.cs_score.reduce_scores()                  # every rank: a collective under a process group
            self.last_cityscapes = self.cs_score.results()
            if get_rank() == 0:
                for line in CS.format_tables(*self.last_cityscapes):
                    Log.info(line)
                Log.info('Cityscapes scores written to {}'.format(self.cs_score.write_json(self.save_dir)))
        if segfix:
            self.running_score_segfix.update_from_hist(confusion_sf)
            self.running_score_segfix.reduce_scores()
            if scored or float(self.running_score_segfix.reduced_confusion_matrix.sum()) > 0:
                self.last_miou_segfix = float(self.running_score_segfix.get_mean_iou())
                if get_rank() == 0:
                    Log.info('Test mIoU (SegFix) {:.6f}\tPixel acc {:.6f}'.format(self.last_miou_segfix,
                                                                                 float(self.running_score_segfix.get_pixel_acc())))
            if self.cs_score_segfix is not None:
                self.cs_score_segfix.reduce_scores()       # every rank: a collective under a process group
                self.last_cityscapes_segfix = self.cs_score_segfix.results()
                if get_rank() == 0:
                    Log.info('Cityscapes scores of the SegFix refinement ({})'.format(SEGFIX_LABEL_DIR))
                    for line in CS.format_tables(*self.last_cityscapes_segfix):
                        Log.info(line)
                    Log.info('Cityscapes scores of the SegFix refinement written to {}'
                             .format(self.cs_score_segfix.write_json(self.save_dir, SEGFIX_RESULT_DIR)))
        return self.last_miou
