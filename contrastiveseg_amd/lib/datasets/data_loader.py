"""Train / validation loaders with the reference's entry points (lib/datasets/data_loader.py:27-140: `DataLoader(configer)
.get_trainloader() / .get_valloader()`) and directory layout (lib/datasets/loader/default_loader.py:108-200:
`<data_dir>/<split>/image/*.png|jpg` + `<data_dir>/<split>/label/<same stem>.png`).

MI355X-first split of the work: the host only DECODES files (PIL, a small thread pool) and hands
raw uint8 batches to the device through pinned memory on a side HIP stream, one batch ahead of the training step;
augmentation, tensor conversion, label encoding and collation are one kernel on the GPU
(lib/datasets/tools/gpu_aug.py -> cseg_augment_batch). Sample order: a fresh torch.randperm per epoch like the
reference's RandomSampler; with a process group every rank takes its strided share of it (DistributedSampler semantics,
data_loader.py:137: batch_size // world_size per rank). A batch of equal-sized images (Cityscapes) travels as one stacked array and
takes the one-kernel path; a batch of differing sizes (COCO-Stuff, ADE20K, ...) travels as one packed buffer with the sizes beside it
and takes the ragged path (cseg_resize_ragged + cseg_augment_ragged). Under `val.data_transformer.size_mode: diverse_size` the
validation loader yields one image per batch at its own size, as the reference does (data_helper.py:107-112); under
`test.data_transformer.size_mode: diverse_size` the test loader yields LIST batches of up to test.batch_size images, each at its own
size padded right / down to fit_stride (collate.py:39-41, 61-68 with stack=False). Still outside the accelerated path, refused by
name: `random_rotate` and the colour transforms (saturation, hue, contrast, perm), `size_mode` `multi_size` / `max_size`, `align_method`
`scale_and_pad` / `only_scale`, a resampling after a crop."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
from contrastiveseg_amd.lib.utils.distributed import get_rank, get_world_size
from contrastiveseg_amd.lib.utils.tools.logger import Logger as Log

IMG_EXT = ('.png', '.jpg', '.jpeg', '.bmp')


def list_pairs(root_dir, split):
    """(image path, label path) pairs of default_loader.py:108-200's layout, sorted by name."""
    image_dir = os.path.join(root_dir, split, 'image')
    label_dir = os.path.join(root_dir, split, 'label')
    pairs = []
    for name in sorted(os.listdir(image_dir)):
        stem, ext = os.path.splitext(name)
        if ext.lower() not in IMG_EXT:
            continue
        lab = os.path.join(label_dir, stem + '.png')
        if not os.path.exists(lab):
            Log.error('Label Path: {} not exists.'.format(lab))
            continue
        pairs.append((os.path.join(image_dir, name), lab))
    return pairs


def _decode(pair, bgr):
    from PIL import Image
    img = np.asarray(Image.open(pair[0]).convert('RGB'))
    if bgr:
        img = img[:, :, ::-1]
    lab = np.asarray(Image.open(pair[1]))
    if lab.ndim == 3:
        lab = lab[:, :, 0]
    return np.ascontiguousarray(img), np.ascontiguousarray(lab.astype(np.uint8))


def pack_ragged(images, labels):
    """Images [H_b,W_b,3] u8 of differing sizes -> (one packed [N,3] u8 buffer, sample after sample in HWC order, the packed [N] u8
    labels or None, [(W_b, H_b)]): the ragged batch of csrc/augment_ragged.hip. Pixel offsets are the running sums of W_b * H_b."""
    img = np.concatenate([im.reshape(-1, 3) for im in images])
    lab = np.concatenate([lb.reshape(-1) for lb in labels]) if labels is not None else None
    return img, lab, [(im.shape[1], im.shape[0]) for im in images]


class FolderSource(object):
    """Raw uint8 batches from image / label files: (stacked images, stacked labels) when the images of a batch share a size,
    (packed images, packed labels, sizes) otherwise."""

    def __init__(self, configer, split, batch_size, shuffle, drop_last=True, workers=8):
        self.pairs = list_pairs(configer.get('data', 'data_dir'), split)
        if not self.pairs:
            raise RuntimeError('no image/label pairs under {}/{}'.format(configer.get('data', 'data_dir'), split))
        mode = configer.get('data', 'input_mode') if configer.exists('data', 'input_mode') else 'BGR'
        self.bgr = (mode == 'BGR')
        self.batch_size, self.shuffle, self.drop_last = batch_size, shuffle, drop_last
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.epoch = 0
        self.seed = configer.get('seed') if configer.exists('seed') and configer.get('seed') is not None else 0

    def set_epoch(self, epoch):
        """torch.utils.data.DistributedSampler.set_epoch: the permutation of an epoch is a function of (seed, epoch) only."""
        self.epoch = int(epoch)

    def shard(self, epoch=None):
        """This rank's sample indices for one epoch, the way the reference's DistributedSampler (lib/datasets/data_loader.py:81-82
        of the reference -> torch.utils.data.distributed.DistributedSampler) produces them: a permutation drawn from a PRIVATE
        generator seeded with seed + epoch (identical on every rank, untouched by the randperm calls of the anchor sampling / the
        memory bank, which advance the global CPU generator by rank-dependent amounts), cut to a multiple of world x batch when
        drop_last (train), padded by wrapping around otherwise, so that every rank yields the same number of batches (a rank with
        fewer forward calls would hang DDP's collectives), then strided by rank."""
        n, world, rank = len(self.pairs), get_world_size(), get_rank()
        epoch = self.epoch if epoch is None else epoch
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(int(self.seed) + int(epoch))
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        chunk = world * self.batch_size
        if self.drop_last:
            order = order[:(n // chunk) * chunk]
        else:
            total = ((n + world - 1) // world) * world
            order = order + order[:total - n]              # n >= 1, total - n < world <= ... wraps once at most for n >= world
            while len(order) < total:
                order = order + order[:total - len(order)]
        return order[rank::world]

    def __len__(self):
        n, world = len(self.pairs), get_world_size()
        if self.drop_last:
            return n // (world * self.batch_size)
        per_rank = (n + world - 1) // world
        return (per_rank + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = self.shard()
        self.epoch += 1                                    # a caller that never calls set_epoch still gets a new permutation
        for i in range(0, len(order), self.batch_size):
            items = list(self.pool.map(lambda k: _decode(self.pairs[k], self.bgr), order[i:i + self.batch_size]))
            for img, lab in items:
                if img.shape[:2] != lab.shape:
                    raise RuntimeError('image {} and label {} of one pair differ in size'.format(img.shape[:2], lab.shape))
            if len({it[0].shape for it in items}) == 1:
                yield np.stack([it[0] for it in items]), np.stack([it[1] for it in items])
            else:
                yield pack_ragged([it[0] for it in items], [it[1] for it in items])


class SyntheticRawSource(object):
    """Seeded raw uint8 images + label ids of `data.raw_size` (default: twice the input size), for runs without files."""

    def __init__(self, configer, batch_size, length, seed=304):
        W, H = configer.get('train', 'data_transformer')['input_size']
        if configer.exists('data', 'raw_size'):
            W0, H0 = configer.get('data', 'raw_size')
        else:
            W0, H0 = 2 * W, 2 * H
        self.shape, self.batch_size, self.length = (H0, W0), batch_size, length
        self.ids = configer.get('data', 'label_list') if configer.exists('data', 'label_list') else \
            list(range(configer.get('data', 'num_classes')))
        self.rs = np.random.RandomState(seed + 1000 * get_rank())

    def __len__(self):
        return self.length

    def __iter__(self):
        H0, W0 = self.shape
        for _ in range(self.length):
            img = self.rs.randint(0, 256, size=(self.batch_size, H0, W0, 3)).astype(np.uint8)
            lab = np.full((self.batch_size, H0, W0), 255, np.uint8)
            for b in range(self.batch_size):
                for _r in range(12):
                    y0, x0 = self.rs.randint(0, H0), self.rs.randint(0, W0)
                    lab[b, y0:y0 + H0 // 3, x0:x0 + W0 // 3] = self.ids[self.rs.randint(0, len(self.ids))]
            yield img, lab


class GPUAugLoader(object):
    """Iterable of {'img': f32 [B,3,H,W], 'labelmap': i64 [B,H,W]} batches on `device`. Raw batch k+1 is decoded and
    uploaded (pinned memory, side stream) while the caller trains on batch k. The 'val' loader under val.score_resize 'cubic' adds
    'ori_labelmap' (a list of i64 [H_b,W_b] tensors: the label files at their own sizes) and 'border_size' ([(w, h)])."""

    def __init__(self, configer, source, device, split='train'):
        self.source, self.device = source, device
        self.transform = GPUBatchTransform(configer, split)
        # the trainer calls `loader.sampler.set_epoch(epoch)` like the reference does (trainer_contrastive.py:183-184)
        self.sampler = source if hasattr(source, 'set_epoch') else None
        self._stream = None
        # val.score_resize 'cubic' (segmentor/trainer_contrastive.py: score_cubic): the validation batches also carry the label files
        # at their own sizes and the transform's border records, the reference's meta['ori_target'] and meta['border_size']
        self.with_ori = split == 'val' and configer.exists('val', 'score_resize') and configer.get('val', 'score_resize') == 'cubic'

    def __len__(self):
        return len(self.source)

    def _upload(self, raw):
        """raw: (images, labels) stacked, or (images, labels, sizes) packed -> (device images, device labels, sizes or None, event)"""
        img, lab = raw[0], raw[1]
        sizes = raw[2] if len(raw) > 2 else None
        if self.device.type != 'cuda':
            return torch.from_numpy(img), torch.from_numpy(lab), sizes, None
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self._stream):
            ti = torch.from_numpy(img).pin_memory().to(self.device, non_blocking=True)
            tl = torch.from_numpy(lab).pin_memory().to(self.device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._stream)
        return ti, tl, sizes, done

    def __iter__(self):
        it = iter(self.source)
        try:
            nxt = self._upload(next(it))
        except StopIteration:
            return
        while nxt is not None:
            ti, tl, sizes, done = nxt
            try:
                nxt = self._upload(next(it))        # overlaps the kernel + the training step of the current batch
            except StopIteration:
                nxt = None
            if done is not None:
                torch.cuda.current_stream(self.device).wait_event(done)
                ti.record_stream(torch.cuda.current_stream(self.device))
                tl.record_stream(torch.cuda.current_stream(self.device))
            out = self.transform(ti, tl, sizes=sizes)
            batch = {'img': out['img'], 'labelmap': out['labelmap']}
            if self.with_ori:
                batch['ori_labelmap'] = self._ori_labels(tl, sizes)
                batch['border_size'] = [(int(w), int(h)) for w, h in out['border_size']]
            yield batch

    def _ori_labels(self, tl, sizes):
        """The reference's ori_target (lib/datasets/loader/default_loader.py:51-58): every raw label at the file's own size through
        the transform's encoding table alone, 255 -> -1; no resampling, no padding. -> a list of i64 [H_b,W_b] device tensors."""
        lut = self.transform.lut
        if lut is not None and lut.device != tl.device:
            lut = lut.to(tl.device)
        if sizes is None:
            raws = list(tl)
        else:
            raws, off = [], 0
            for w, h in sizes:
                raws.append(tl[off:off + w * h].view(h, w))
                off += w * h
        out = []
        for raw in raws:
            lab = raw.long() if lut is None else lut.long()[raw.long()]
            out.append(torch.where(lab == 255, torch.full_like(lab, -1), lab))
        return out


class TestFolderLoader(object):
    """Iterable of {'img': f32 [B,3,H,W], 'name': [stem], 'border_size': [(w, h)], 'pad_offset': [(left, up)] and, where label
    files exist, 'labelmap': i64 [B,H,W] (-1 = ignore, the collate padding included)} for the test phase (the reference's
    get_testloader, lib/datasets/data_loader.py:205-240, yields names and metas the same way). No shuffling, no dropped or
    repeated samples: with a process group every rank takes its strided share, so that the reduced confusion matrix counts every
    image once. Under size_mode diverse_size 'img' is a list of [1,3,Hp_b,Wp_b] tensors and 'labelmap' a list of [1,Hp_b,Wp_b], every
    image at its own size padded to fit_stride (image 0, label -1), each through the transform alone as the reference collates it.
    With test.evaluator set also 'labelmap_raw': u8 [B,H,W] and 'instancemap': i16 [B,H,W] (the bits of the uint16 instance ids of
    <test.instance_dir>/<stem>.png, default <image dir>/../instance), every image at its pad_offset. With test.segfix_offset_dir set
    also 'segfix_offset': int8 or f32 [B,H,W,2], the boundary offsets <dir>/<stem>.mat (else .npy) of every image at its pad_offset,
    zero in the padding (lib/datasets/segfix_offsets.py)."""

    def __init__(self, configer, image_dir, label_dir, batch_size, device, workers=8):
        self.device = device
        self.items = []
        for name in sorted(os.listdir(image_dir)):
            stem, ext = os.path.splitext(name)
            if ext.lower() in IMG_EXT:
                self.items.append((os.path.join(image_dir, name), stem))
        if not self.items:
            raise RuntimeError('no images under {}'.format(image_dir))
        self.label_dir = label_dir if label_dir is not None and all(
            os.path.exists(os.path.join(label_dir, stem + '.png')) for _, stem in self.items) else None
        mode = configer.get('data', 'input_mode') if configer.exists('data', 'input_mode') else 'BGR'
        self.bgr = (mode == 'BGR')
        self.batch_size = max(1, int(batch_size))
        self.transform = GPUBatchTransform(configer, 'test')
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        # test.evaluator (this project's own key): every batch additionally carries the raw label ids and the 16-bit instance ids
        self.instance_dir = None
        if configer.exists('test', 'evaluator') and configer.get('test', 'evaluator') is not None:
            if self.label_dir is None:
                raise FileNotFoundError('test.evaluator {!r} needs the raw label ids of every image under {}'
                                        .format(configer.get('test', 'evaluator'), label_dir))
            self.instance_dir = configer.get('test', 'instance_dir') if configer.exists('test', 'instance_dir') and configer.get(
                'test', 'instance_dir') else os.path.join(os.path.dirname(os.path.normpath(image_dir)), 'instance')
            for _, stem in self.items:
                if not os.path.exists(os.path.join(self.instance_dir, stem + '.png')):
                    raise FileNotFoundError('test.evaluator {!r}: test.instance_dir {} has no {}.png'
                                            .format(configer.get('test', 'evaluator'), self.instance_dir, stem))

        # test.segfix_offset_dir (this project's own key): every batch additionally carries the boundary offsets of its images
        self.segfix_dir, self.segfix_files = None, {}
        if configer.exists('test', 'segfix_offset_dir') and configer.get('test', 'segfix_offset_dir') is not None:
            from contrastiveseg_amd.lib.datasets.segfix_offsets import find_offset_file
            self.segfix_dir = configer.get('test', 'segfix_offset_dir')
            if not isinstance(self.segfix_dir, str) or not os.path.isdir(self.segfix_dir):
                raise FileNotFoundError('test.segfix_offset_dir {!r} does not exist'.format(self.segfix_dir))
            if self.transform.size_mode == 'diverse_size':
                raise NotImplementedError('test.segfix_offset_dir under test.data_transformer size_mode diverse_size: the refinement '
                                          'takes batches of equal-sized images only')
            for _, stem in self.items:
                self.segfix_files[stem] = find_offset_file(self.segfix_dir, stem)
                if self.segfix_files[stem] is None:
                    raise FileNotFoundError('test.segfix_offset_dir {} has neither {}.mat nor {}.npy'.format(self.segfix_dir, stem, stem))

    def _mine(self):
        return self.items[get_rank()::get_world_size()]

    def _segfix_offsets(self, chunk, items, out):
        """int8 or f32 [B,H,W,2]: every image's offsets at its pad_offset, zero in the padding."""
        from contrastiveseg_amd.lib.datasets.segfix_offsets import batch_offsets, load_offsets
        regions = []
        for k, (item, (img, _)) in enumerate(zip(chunk, items)):
            h, w = img.shape[:2]
            if (int(out['border_size'][k][0]), int(out['border_size'][k][1])) != (w, h):
                raise ValueError('{}: the image is {} x {} and its region in the batch {} x {}; test.segfix_offset_dir refines every '
                                 'image at its own size'.format(item[0], h, w, int(out['border_size'][k][1]), int(out['border_size'][k][0])))
            regions.append((int(out['pad_offset'][k][0]), int(out['pad_offset'][k][1]), w, h))
        arrays = list(self.pool.map(lambda a: load_offsets(self.segfix_files[a[0][1]], a[1][0].shape[:2]), zip(chunk, items)))
        return torch.from_numpy(batch_offsets(arrays, regions, out['img'].shape[-2:])).to(self.device)

    def _instance(self, item, shape):
        from contrastiveseg_amd.lib.metrics.cityscapes_score import load_instance_map
        path = os.path.join(self.instance_dir, item[1] + '.png')
        inst = load_instance_map(path)
        if inst.shape != tuple(shape):
            raise ValueError('{}: the instance map is {} x {}, the image {} x {}'.format(path, inst.shape[0], inst.shape[1], shape[0],
                                                                                         shape[1]))
        return inst

    def _raw_maps(self, chunk, items, out):
        """labelmap_raw u8 [B,H,W] (the label file's bytes, no label_list look-up) and instancemap i16 [B,H,W] (the 16-bit instance ids;
        int16 carries the bits, as for the disparity maps of ms_test_depth), every image at its pad_offset, zero in the padding."""
        B, (H, W) = len(items), out['img'].shape[-2:]
        raw = np.zeros((B, H, W), dtype=np.uint8)
        inst = np.zeros((B, H, W), dtype=np.uint16)
        for k, (item, (img, lab)) in enumerate(zip(chunk, items)):
            h, w = img.shape[:2]
            x0, y0 = int(out['pad_offset'][k][0]), int(out['pad_offset'][k][1])
            if (int(out['border_size'][k][0]), int(out['border_size'][k][1])) != (w, h) or lab.shape != (h, w):
                raise ValueError('{}: the image is {} x {}, its label map {} x {} and its region in the batch {} x {}; test.evaluator '
                                 'scores every image at its own size'.format(item[0], h, w, lab.shape[0], lab.shape[1],
                                                                             int(out['border_size'][k][1]), int(out['border_size'][k][0])))
            raw[k, y0:y0 + h, x0:x0 + w] = lab
            inst[k, y0:y0 + h, x0:x0 + w] = self._instance(item, (h, w))
        return torch.from_numpy(raw).to(self.device), torch.from_numpy(inst.view(np.int16)).to(self.device)

    def __len__(self):
        return (len(self._mine()) + self.batch_size - 1) // self.batch_size

    def _decode(self, item):
        from PIL import Image
        img = np.asarray(Image.open(item[0]).convert('RGB'))
        if self.bgr:
            img = img[:, :, ::-1]
        lab = None
        if self.label_dir is not None:
            lab = np.asarray(Image.open(os.path.join(self.label_dir, item[1] + '.png')))
            if lab.ndim == 3:
                lab = lab[:, :, 0]
            lab = np.ascontiguousarray(lab.astype(np.uint8))
        return np.ascontiguousarray(img), lab

    def _list_batch(self, chunk, items):
        batch = {'img': [], 'name': [stem for _, stem in chunk], 'border_size': [], 'pad_offset': []}
        if self.label_dir is not None:
            batch['labelmap'] = []
        for img, lab in items:
            ti = torch.from_numpy(img[None]).to(self.device)
            tl = torch.from_numpy(lab[None]).to(self.device) if lab is not None else None
            out = self.transform(ti, tl)
            batch['img'].append(out['img'])
            batch['border_size'].append((int(out['border_size'][0][0]), int(out['border_size'][0][1])))
            batch['pad_offset'].append((int(out['pad_offset'][0][0]), int(out['pad_offset'][0][1])))
            if tl is not None:
                batch['labelmap'].append(out['labelmap'])
        return batch

    def __iter__(self):
        mine = self._mine()
        for i in range(0, len(mine), self.batch_size):
            chunk = mine[i:i + self.batch_size]
            items = list(self.pool.map(self._decode, chunk))
            labels = [it[1] for it in items] if self.label_dir is not None else None
            if self.transform.size_mode == 'diverse_size':
                yield self._list_batch(chunk, items)
                continue
            if len({it[0].shape for it in items}) == 1:
                img, lab, sizes = np.stack([it[0] for it in items]), np.stack(labels) if labels is not None else None, None
            else:                                          # mixed sizes under fix_size + only_pad: every image padded to input_size
                img, lab, sizes = pack_ragged([it[0] for it in items], labels)
            ti = torch.from_numpy(img).to(self.device)
            tl = torch.from_numpy(lab).to(self.device) if lab is not None else None
            out = self.transform(ti, tl, sizes=sizes)
            batch = {'img': out['img'], 'name': [stem for _, stem in chunk],
                     'border_size': [(int(w), int(h)) for w, h in out['border_size']],
                     'pad_offset': [(int(l), int(u)) for l, u in out['pad_offset']]}
            if tl is not None:
                batch['labelmap'] = out['labelmap']
            if self.instance_dir is not None:
                batch['labelmap_raw'], batch['instancemap'] = self._raw_maps(chunk, items, out)
            if self.segfix_dir is not None:
                batch['segfix_offset'] = self._segfix_offsets(chunk, items, out)
            yield batch


class DataLoader(object):
    def __init__(self, configer, device=None):
        self.configer = configer
        self.device = device if device is not None else torch.device(
            'cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')

    def _workers(self):
        return self.configer.get('data', 'workers') if self.configer.exists('data', 'workers') else 8

    def get_trainloader(self):
        bs = max(1, self.configer.get('train', 'batch_size') // get_world_size())
        src = FolderSource(self.configer, 'train', bs, shuffle=True, drop_last=True, workers=self._workers())
        Log.info('train: {} image/label pairs, {} batches of {} per rank'.format(len(src.pairs), len(src), bs))
        return GPUAugLoader(self.configer, src, self.device, 'train')

    def get_valloader(self, dataset='val'):
        bs = max(1, self.configer.get('val', 'batch_size') // get_world_size())
        dt = self.configer.get('val', 'data_transformer') if self.configer.exists('val', 'data_transformer') else {}
        if dt.get('size_mode', 'fix_size') == 'diverse_size':
            bs = 1                                         # every image alone at its own size (data_helper.py:107-112)
        src = FolderSource(self.configer, dataset, bs, shuffle=False, drop_last=False, workers=self._workers())
        return GPUAugLoader(self.configer, src, self.device, 'val')

    def get_testloader(self):
        """Images of test.test_dir (default: <data_dir>/val/image) with their stems; labels from <image dir>/../label where every
        image has one; resized / padded as test.data_transformer says (default: val.data_transformer, else the images' own size)."""
        c = self.configer
        image_dir = c.get('test', 'test_dir') if c.exists('test', 'test_dir') else None
        if image_dir is None:
            data_dir = c.get('data', 'data_dir')
            image_dir = os.path.join(data_dir[0] if isinstance(data_dir, (list, tuple)) else data_dir, 'val', 'image')
        if not os.path.isdir(image_dir):
            raise RuntimeError('test image directory {} does not exist'.format(image_dir))
        label_dir = os.path.join(os.path.dirname(os.path.normpath(image_dir)), 'label')
        if not c.exists('test', 'data_transformer'):
            if c.exists('val', 'data_transformer'):
                c.add(['test', 'data_transformer'], dict(c.get('val', 'data_transformer')))
            else:
                from PIL import Image
                first = sorted(n for n in os.listdir(image_dir) if os.path.splitext(n)[1].lower() in IMG_EXT)
                if not first:
                    raise RuntimeError('no images under {}'.format(image_dir))
                with Image.open(os.path.join(image_dir, first[0])) as im:
                    c.add(['test', 'data_transformer'], {'size_mode': 'fix_size', 'input_size': list(im.size),
                                                         'align_method': 'only_pad', 'pad_mode': 'pad_right_down'})
        bs = c.get('test', 'batch_size') if c.exists('test', 'batch_size') else \
            (c.get('val', 'batch_size') if c.exists('val', 'batch_size') else 1)
        bs = bs or 1
        loader = TestFolderLoader(c, image_dir, label_dir if os.path.isdir(label_dir) else None, bs, self.device, self._workers())
        Log.info('test: {} images under {}, labels: {}'.format(len(loader.items), image_dir, loader.label_dir is not None))
        return loader
