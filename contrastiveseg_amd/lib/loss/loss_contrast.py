"""PixelContrastLoss / ContrastCELoss / ContrastAuxCELoss with the reference's constructor and forward contracts
(lib/loss/loss_contrast.py:15-234), computed by the HIP kernels of libcseg_hip.so:

  reference step (loss_contrast.py)                       here
  ------------------------------------------------------  --------------------------------------------------
  :180-181 F.interpolate(seg) + FSCELoss                  cseg_upsample_ce_fwd/bwd (no [B,K,H,W] tensor)
  :183 torch.max(seg,1); :131-134 nearest label resize;   cseg_classify_partition (one pass over seg, stable
  :35-64 unique / nonzero per (image,class)               hard/easy partition in .nonzero() order)
  :66-82 keep rule + torch.randperm                       anchor_sampling.plan_selection (host, same CPU RNG
                                                          stream => bit-identical indices)
  :141-142 NHWC copy, :85-87 gather                       cseg_gather_anchors straight from NCHW
  :91-128 _contrastive                                    cseg_contrast_fwd/bwd (fp32 MFMA)

Data-parallel (one process per GPU, RCCL). Two modes, chosen by `contrast.cross_rank`:
  * false (the code default = the reference's DDP behaviour): every rank contrasts only the <= max_samples anchors
    mined from its own images; nothing but DDP's gradient all-reduce crosses ranks.
  * true (opt-in; set by the shipped HRNet configs because BASELINE.json's multi-GPU configuration asks for it): the
    contrast set is the union of every rank's anchors: counts are all-gathered so all ranks derive the same global
    selection from the same RNG stream, each rank gathers its own rows, rows are all-gathered, and every rank
    evaluates the global loss while back-propagating only into its own embeddings (gradient scaled by world_size so
    that DDP's gradient averaging reproduces the single-process gradient of the global loss). This CHANGES the
    objective relative to the reference's DDP run (world x more negatives per anchor); its oracle is the reference's
    single-process loss on the concatenated global batch. The anchor budget of the global set is
    max_samples * world_size by default (`contrast.cross_rank_budget`: 'per_rank' | 'global').
The memory-bank criterion (loss_contrast_mem.py) always contrasts a rank's own anchors against its own copy of the
bank, as the reference does; `cross_rank` does not apply to it.

`contrast.device_sampling` (opt-in, CSEG_DEVICE_SAMPLING=0|1 overrides): the keep rule and the torch.randperm
replicas run on the device too (csrc/sampling.hip), from a device copy of the CPU generator's mt19937 state, and the gather / contrast /
scatter kernels read the number of anchors from device memory. No device-to-host copy, no data-dependent host value, so the criterion
can be captured in a hipGraph; same picks, loss and gradient as the host path under the same seed.

`contrast.device_bank` (opt-in, CSEG_DEVICE_BANK=0|1 overrides): the same for the memory-bank criteria, together with
the enqueue of Trainer._dequeue_and_enqueue -- both draw from the criterion's one device generator, in the reference's order."""
from abc import ABC

import numpy as np
import torch
import torch.nn as nn

from contrastiveseg_amd import _host
from contrastiveseg_amd import kernels as K
from contrastiveseg_amd.lib.loss.anchor_sampling import plan_selection
from contrastiveseg_amd.lib.loss.loss_helper import (FSAuxCELOVASZLoss, FSAuxCELoss, FSAuxOhemCELoss, FSAuxRMILoss, FSCELOVASZLoss,
                                                     FSCELoss, FSOhemCELoss, FSRMILoss)
from contrastiveseg_amd.lib.utils import distributed as D
from contrastiveseg_amd.lib.utils.tools.logger import Logger as Log


class _GradScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def _counts_to_host(cp):
    """One D2H copy (the only host sync of the loss): counts + status."""
    if "host_counts" in cp:
        flat, done = cp["host_counts"]
        done.synchronize()                       # waits for the side stream only
    else:
        flat = torch.cat([cp["counts"].reshape(-1), cp["status"]]).cpu()
    counts = flat[:-4].reshape(cp["counts"].shape).numpy()
    if int(flat[-4]) != 0:
        raise RuntimeError("PixelContrastLoss: %d label values are neither ignore_label nor in [0, num_classes); "
                           "the HIP mining kernel handles classes 0..K-1 only" % int(flat[-4]))
    return counts


def device_sampling_wanted(configer):
    """contrast.device_sampling (bool, default false), overridden by CSEG_DEVICE_SAMPLING=0|1."""
    want = bool(configer.get('contrast', 'device_sampling')) if configer.exists('contrast', 'device_sampling') else False
    env = getattr(K, "DEVICE_SAMPLING", None)      # (a stand-in for the kernels module, as the CPU port of the tests, has no switches)
    if env in ("0", "1"):
        want = env == "1"
    return want


def device_bank_wanted(configer):
    """contrast.device_bank (bool, default false), overridden by CSEG_DEVICE_BANK=0|1. Read by the memory-bank criteria only."""
    want = bool(configer.get('contrast', 'device_bank')) if configer.exists('contrast', 'device_bank') else False
    env = getattr(K, "DEVICE_BANK", None)
    if env in ("0", "1"):
        want = env == "1"
    return want


def _refuse_device_bank_multi_rank():
    if D.get_world_size() > 1 or D.exercise_single_rank():
        raise NotImplementedError("contrast.device_bank on more than one rank (or under CSEG_DIST_SINGLE_RANK=1) is a follow-up: the "
                                  "multi-rank enqueue (Trainer._enqueue_global) plans the global batch on the host")


def _grad_slot(embed):
    """kernels.SparseGradSlot the projection head attached to the embedding it produced (row-sparse backward, opt-in:
    lib/models/modules/projection.py), or None = the dense zero-filled gradient."""
    return getattr(embed, '_cseg_grad_slot', None)


class PixelContrastLoss(nn.Module, ABC):
    uses_memory_bank = False     # loss_contrast_mem.PixelContrastLoss: True

    def __init__(self, configer):
        super(PixelContrastLoss, self).__init__()
        self.configer = configer
        self.temperature = self.configer.get('contrast', 'temperature')
        self.base_temperature = self.configer.get('contrast', 'base_temperature')
        self.ignore_label = -1
        if self.configer.exists('loss', 'params') and 'ce_ignore_index' in self.configer.get('loss', 'params'):
            self.ignore_label = self.configer.get('loss', 'params')['ce_ignore_index']
        self.max_samples = self.configer.get('contrast', 'max_samples')
        self.max_views = self.configer.get('contrast', 'max_views')
        self.cross_rank = False      # reference parity unless the config opts in (see the module docstring)
        if self.configer.exists('contrast', 'cross_rank'):
            self.cross_rank = bool(self.configer.get('contrast', 'cross_rank'))
        # anchor budget of the cross-rank set: 'per_rank' = max_samples * world_size anchors in total (every rank of
        # the reference's DDP run owns a max_samples budget), 'global' = max_samples in total (parity with a
        # single process that sees the concatenated global batch).
        self.cross_rank_budget = 'per_rank'
        if self.configer.exists('contrast', 'cross_rank_budget'):
            self.cross_rank_budget = self.configer.get('contrast', 'cross_rank_budget')
        assert self.cross_rank_budget in ('per_rank', 'global')
        # RNG of the cross-rank set: 'local' = every rank draws only its own segments from its own generator (host
        # cost independent of world size); 'global' = every rank draws for all global segments in global image order,
        # which reproduces a single process on the concatenated batch index for index (host cost grows with world).
        self.cross_rank_rng = 'local'
        if self.configer.exists('contrast', 'cross_rank_rng'):
            self.cross_rank_rng = self.configer.get('contrast', 'cross_rank_rng')
        assert self.cross_rank_rng in ('local', 'global')
        self._side = None            # side HIP stream for mining (created lazily on the first GPU call)
        self.last_selection = None   # {'sel_pix': i32 [N] (b*P+pixel, view-major), 'plan': SelectionPlan}
        self.device_sampling = device_sampling_wanted(configer)
        # memory-bank criteria: anchor sampling AND Trainer._dequeue_and_enqueue on the device, one generator stream
        self.device_bank = self.uses_memory_bank and device_bank_wanted(configer)
        if self.device_bank:
            self._check_device_bank()
        if self.device_sampling and self.uses_memory_bank and not self.device_bank:
            # follow-up: the enqueue draws of Trainer._dequeue_and_enqueue come from the same CPU generator stream; one stream split over
            # two generators would silently leave the reference's index sequence
            raise NotImplementedError("contrast.device_sampling is not available for the memory-bank criteria (their enqueue draws "
                                      "share the CPU generator stream with the anchor sampling)")
        # plain attributes, not buffers: state_dict keys stay those of the reference
        self._rng_state = None       # i32 [625] on the device: mt19937 words + pos, imported from torch's CPU generator on first use
        self.sampling_sticky = None  # i32 [1] on the device: OR of the status bits of every step (Trainer._display reads it)

    def _check_device_bank(self):
        """What the device route of the memory-bank criteria cannot do, refused when the criterion is built."""
        c = self.configer
        _refuse_device_bank_multi_rank()
        ms = c.get('contrast', 'memory_size') if c.exists('contrast', 'memory_size') else None
        freq = c.get('contrast', 'pixel_update_freq') if c.exists('contrast', 'pixel_update_freq') else None
        if ms is not None and freq is not None and freq > ms:
            # the reference's `[-K:]` write fails there; the device writers would have to invent a rule
            raise ValueError("contrast.device_bank: pixel_update_freq=%d is larger than memory_size=%d" % (freq, ms))
        num_classes = c.get('data', 'num_classes') if c.exists('data', 'num_classes') else None
        if ms is not None and num_classes is not None and self.max_samples > num_classes * 2 * ms:
            # the kernels need N <= M (the reference's self mask, loss_contrast_mem.py:134-138) and N is not known on the host
            raise ValueError("contrast.device_bank: max_samples=%d is larger than the bank's num_classes * 2 * memory_size = %d columns"
                             % (self.max_samples, num_classes * 2 * ms))

    # -- mining ------------------------------------------------------------------------------------------
    def _classify(self, feats, labels, predict, seg, prezeroed=False):
        """The one cseg_classify_partition call. `prezeroed` (device sampling) is passed on only when set: the CPU restatement of the
        kernels module (oracle/cpu_port.py) has no such argument."""
        kw = {"prezeroed": True} if prezeroed else {}
        if seg is not None:
            return K.classify_partition(labels, self.ignore_label, seg=seg, **kw)
        return K.classify_partition(labels, self.ignore_label, predict=predict.contiguous(),
                                    num_classes=self.configer.get('data', 'num_classes'), feat_hw=tuple(feats.shape[2:]), **kw)

    @staticmethod
    def _overlaps(seg_ready, seg):
        """Whether mining goes to the side stream: the model recorded `seg_ready` (a HIP event, right after the logits were produced,
        see nets/hrnet.py) and the logits are on the GPU. Otherwise it is a plain call on the current stream."""
        return seg_ready is not None and seg is not None and seg.is_cuda

    def _fork_join(self, seg_ready, seg, labels, run):
        """Runs `run()` on the side stream behind `seg_ready` and joins the compute stream behind it, so that what `run` enqueues --
        and any host work that follows -- overlaps the projection head still running on the compute stream. `run` returns
        (result, tensors it produced that the compute stream consumes); returns (result, the event recorded behind the work)."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=seg.device)
        main = torch.cuda.current_stream(seg.device)
        with torch.cuda.stream(self._side):
            self._side.wait_event(seg_ready)
            result, consumed = run()
            done = torch.cuda.Event()
            done.record(self._side)
        for t in consumed:
            t.record_stream(main)                # produced on the side stream, consumed on the compute stream
        seg.record_stream(self._side)
        labels.record_stream(self._side)
        main.wait_event(done)
        return result, done

    def _mine(self, feats, labels, predict, seg, seg_ready=None, gather=False):
        """Runs cseg_classify_partition. With `seg_ready` the kernels and the counts D2H copy go to the side stream (_fork_join), so
        they -- and the host-side selection plan that follows -- overlap the projection head."""
        if not self._overlaps(seg_ready, seg):
            return self._classify(feats, labels, predict, seg)

        def run():
            cp = self._classify(feats, labels, predict, seg)
            flat = torch.cat([cp["counts"].reshape(-1), cp["status"]])
            if gather:
                # cross-rank contrast set: the all-gather of the per-rank counts is issued HERE, on the side stream, so that it -- like
                # the mining itself and the D2H copy -- runs under the CE kernels / projection head on the compute stream and the host
                # only waits on the event below (round 3: a blocking all-gather + .cpu() in the middle of the loss forward)
                flat = D.all_gather_cat(flat.unsqueeze(0))
            host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
            host.copy_(flat, non_blocking=True)
            return (cp, host), list(cp.values())
        (cp, host), done = self._fork_join(seg_ready, seg, labels, run)
        cp["host_counts_global" if gather else "host_counts"] = (host, done)
        return cp

    def _plan(self, counts, budget_mult=1, draw_images=None):
        plan = plan_selection(counts, self.max_samples * budget_mult, self.max_views, draw_images)
        if plan is None:
            # the reference returns (None, None) and then fails on None.shape (loss_contrast.py:44-45, :92)
            raise RuntimeError("PixelContrastLoss: no (image, class) segment has more than max_views=%d pixels"
                               % self.max_views)
        return plan

    # -- device-side sampling -----------------------------------------------------------------------------
    def _rng_on(self, dev):
        """The device generator, created on first use from the state of torch's default CPU generator."""
        if self._rng_state is None or self._rng_state.device != dev:
            words = _host.mt_export()                               # raises without libcseg_host.so: no silent fallback
            self._rng_state = torch.from_numpy(words.view(np.int32).copy()).to(dev)
            self.sampling_sticky = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._rng_state

    def import_rng_from_torch(self):
        """Takes the state of torch's default CPU generator again (e.g. after torch.manual_seed), into the existing device buffer."""
        if self._rng_state is not None:
            self._rng_state.copy_(torch.from_numpy(_host.mt_export().view(np.int32).copy()))

    def export_rng_to_torch(self):
        """Hands the generator stream back: writes the device state into torch's default CPU generator (synchronises). For tests
        and for code that goes on drawing from the CPU generator."""
        if self._rng_state is not None:
            _host.mt_import(self._rng_state.cpu().numpy().view(np.uint32))

    def _forward_device(self, feats, labels, predict, seg, seg_ready, segment_queue=None, pixel_queue=None):
        """Mining, selection, gather, contrast: all enqueued, nothing read back. Mining and planning keep the side-stream fork and
        join of _mine when the model recorded `seg_ready`. With the two queues the contrast set is the memory bank, read in place."""
        rng = self._rng_on(feats.device)

        def run():
            cp = self._classify(feats, labels, predict, seg, prezeroed=True)
            out = (cp["part_idx"],) + tuple(K.sample_anchors(cp, self.max_samples, self.max_views, rng, self.sampling_sticky))
            return out, out
        if self._overlaps(seg_ready, seg):
            (part_idx, sel_pos, a_lab, header), _ = self._fork_join(seg_ready, seg, labels, run)
        else:
            (part_idx, sel_pos, a_lab, header), _ = run()
        if segment_queue is not None:
            loss, sel_pix = K.PixelContrastDeviceBank.apply(feats, part_idx, sel_pos, a_lab, header, self.temperature,
                                                            self.base_temperature, segment_queue.contiguous(), pixel_queue.contiguous(),
                                                            _grad_slot(feats))
        else:
            loss, sel_pix = K.PixelContrastDevice.apply(feats, part_idx, sel_pos, a_lab, header, self.temperature,
                                                        self.base_temperature, _grad_slot(feats))
        self.last_selection = {"sel_pix": sel_pix, "header": header, "plan": None}
        return loss

    # -- forward -----------------------------------------------------------------------------------------
    def forward(self, feats, labels=None, predict=None, seg=None, seg_ready=None, segment_queue=None, pixel_queue=None):
        """feats [B,D,h,w] (L2-normalised embeddings), labels [B,H,W] long, and either `predict` [B,h,w] long
        (reference signature, loss_contrast.py:130) or `seg` [B,K,h,w] logits (argmax fused into the mining
        kernel). With the two queues (loss_contrast_mem.PixelContrastLoss passes them) the contrast set is the memory bank: a
        rank's own anchors against its own copy of the bank, whatever `cross_rank` says."""
        assert labels is not None and (predict is not None or seg is not None)
        world = D.get_world_size()
        cross = segment_queue is None and (world > 1 or D.exercise_single_rank()) and self.cross_rank
        if self.device_bank:
            # (also without the queues -- the bank-free term of a memory criterion: the enqueue draws from the device generator, and one
            # stream split over two generators would leave the reference's index sequence)
            _refuse_device_bank_multi_rank()
            return self._forward_device(feats, labels, predict, seg, seg_ready, segment_queue, pixel_queue)
        if self.device_sampling:
            if cross:
                raise NotImplementedError("contrast.device_sampling with contrast.cross_rank on more than one rank (or under "
                                          "CSEG_DIST_SINGLE_RANK=1) is a follow-up: the cross-rank set needs the global plan on the host")
            return self._forward_device(feats, labels, predict, seg, seg_ready)
        cp = self._mine(feats, labels, predict, seg, seg_ready, gather=cross)
        if cross:
            return self._forward_cross_rank(feats, cp, feats.shape[2] * feats.shape[3], world)
        plan = self._plan(_counts_to_host(cp))
        if segment_queue is None:
            return self._forward_plan(feats, cp, plan, "self")
        return self._forward_plan(feats, cp, plan, "bank", segment_queue.contiguous(), pixel_queue.contiguous())

    def _forward_plan(self, feats, cp, plan, mode, segment_queue=None, pixel_queue=None):
        """The local contrast term of a host plan: the picks to the device, gather + contrast against the anchors themselves
        (mode "self") or the memory bank ("bank", read in place)."""
        P = feats.shape[2] * feats.shape[3]
        dev = feats.device
        sel_pos = torch.from_numpy(plan.row_img.astype(np.int32) * P + plan.row_off).to(dev, non_blocking=True)
        a_lab = torch.from_numpy(plan.row_lab.astype(np.int32)).to(dev, non_blocking=True)
        loss, sel_pix = K.PixelContrast.apply(feats, cp["part_idx"], sel_pos, a_lab, mode, self.temperature,
                                              self.base_temperature, segment_queue, pixel_queue, _grad_slot(feats))
        self.last_selection = {"sel_pix": sel_pix, "plan": plan}
        return loss

    def _forward_cross_rank(self, feats, cp, P, world):
        rank = D.get_rank()
        B = feats.shape[0]
        dev = feats.device
        if "host_counts_global" in cp:
            host, done = cp["host_counts_global"]               # gathered and copied on the side stream (_mine)
            done.synchronize()
        else:
            local = torch.cat([cp["counts"].reshape(-1), cp["status"]])
            host = D.all_gather_cat(local.unsqueeze(0)).cpu()  # RCCL all-gather, B*K*2+4 ints per rank
        if int(host[:, -4].sum()) != 0:
            raise RuntimeError("PixelContrastLoss: labels outside [0, num_classes) on some rank")
        counts = host[:, :-4].reshape((world * B,) + tuple(cp["counts"].shape[1:])).numpy()
        # T, n_view, labels and row order are identical on every rank (same counts); the drawn offsets are needed
        # for the rank's own images only
        plan = self._plan(counts, world if self.cross_rank_budget == 'per_rank' else 1,
                          (rank * B, (rank + 1) * B) if self.cross_rank_rng == 'local' else None)
        T, V = plan.T, plan.n_view
        owner = plan.seg_img // B                               # rank of every segment
        mine = np.nonzero(owner == rank)[0]
        t_r = [int((owner == r).sum()) for r in range(world)]
        # local rows, view-major inside this rank's segment range
        rows_local = (np.arange(V)[:, None] * T + mine[None, :]).reshape(-1)
        sel_pos = torch.from_numpy(((plan.row_img[rows_local] - rank * B) * P + plan.row_off[rows_local])
                                   .astype(np.int32)).to(dev)
        anchors_l, sel_pix = K.GatherAnchors.apply(feats, cp["part_idx"], sel_pos, _grad_slot(feats))
        t_max = max(t_r)
        pad = torch.zeros(t_max * V, feats.shape[1], dtype=feats.dtype, device=dev)
        pad[:anchors_l.shape[0]] = anchors_l.detach()
        bufs = D.all_gather_cat(pad.unsqueeze(0))               # RCCL all-gather, <= max_samples x D floats in total
        pieces = []
        order = np.empty(T * V, dtype=np.int64)                 # global row -> position in cat(pieces)
        base = 0
        for r in range(world):
            n_r = t_r[r] * V
            pieces.append(_GradScale.apply(anchors_l, float(world)) if r == rank else bufs[r][:n_r])
            seg_r = np.nonzero(owner == r)[0]
            glob_rows = (np.arange(V)[:, None] * T + seg_r[None, :]).reshape(-1)
            order[glob_rows] = base + np.arange(n_r)
            base += n_r
        allrows = torch.cat(pieces, dim=0)
        anchors_g = allrows.index_select(0, torch.from_numpy(order).to(dev))
        a_lab = torch.from_numpy(plan.row_lab.astype(np.int32)).to(dev)
        loss = K.ContrastOnAnchors.apply(anchors_g, a_lab, "self", self.temperature, self.base_temperature,
                                         None, None, None, None)
        self.last_selection = {"sel_pix": sel_pix, "plan": plan, "rows_local": rows_local}
        return loss


# the segmentation criterion of the composite criteria: [takes the auxiliary map too][term]. 'rmi' without an auxiliary map: the
# reference constructs FSAuxRMILoss there and unpacks the single logit tensor as a pair, which cannot run; FSRMILoss is what it sets
# out to be
SEG_CRITERIA = {False: {"ce": FSCELoss, "rmi": FSRMILoss, "lovasz": FSCELOVASZLoss, "ohem": FSOhemCELoss},
                True: {"ce": FSAuxCELoss, "rmi": FSAuxRMILoss, "lovasz": FSAuxCELOVASZLoss, "ohem": FSAuxOhemCELoss}}


class _ContrastComposite(nn.Module, ABC):
    """seg_criterion(seg | [seg_aux, seg]) + loss_weight * contrast_criterion(embed): the four registered contrast criteria (this
    module and loss_contrast_mem.py) are this class with other data.

    `contrast.use_ohem` (bool, default false; all four criteria) gives the segmentation term hard-pixel mining: FSOhemCELoss on the
    segmentation map (FSAuxOhemCELoss with an auxiliary map), with loss.params.ohem_thresh / ohem_minkeep. The switch is the project's own,
    like FSAuxCELOVASZLoss: the reference reaches its OHEM criteria only through the fs_ohemce_loss / fs_auxohemce_loss keys, never from
    a contrast criterion. Together with use_rmi or use_lovasz it is refused: each of the three replaces the same term."""
    aux = False                          # the segmentation criterion takes [seg_aux, seg]
    contrast_class = PixelContrastLoss   # the memory pair: loss_contrast_mem.PixelContrastLoss
    reads_lovasz = False                 # the memory pair reads contrast.use_lovasz too (the reference's bank-free pair has no such switch)

    def __init__(self, configer=None):
        super(_ContrastComposite, self).__init__()
        self.configer = configer
        ignore_index = -1
        if self.configer.exists('loss', 'params') and 'ce_ignore_index' in self.configer.get('loss', 'params'):
            ignore_index = self.configer.get('loss', 'params')['ce_ignore_index']
        Log.info('ignore_index: {}'.format(ignore_index))
        self.loss_weight = self.configer.get('contrast', 'loss_weight')
        self.use_rmi = self.configer.get('contrast', 'use_rmi')
        term = "rmi" if self.use_rmi else "ce"
        if self.reads_lovasz:
            self.use_lovasz = self.configer.get('contrast', 'use_lovasz') \
                if self.configer.exists('contrast', 'use_lovasz') else False
            if self.use_lovasz and self.use_rmi:
                raise NotImplementedError("contrast.use_lovasz together with contrast.use_rmi: the reference silently takes RMI there; "
                                          "switch one of them off")
            if self.use_lovasz:
                term = "lovasz"
        self.use_ohem = bool(self.configer.get('contrast', 'use_ohem')) if self.configer.exists('contrast', 'use_ohem') else False
        if self.use_ohem:
            for other in ("use_rmi", "use_lovasz"):
                if getattr(self, other, False):
                    raise NotImplementedError("contrast.use_ohem together with contrast.%s: both replace the segmentation term; "
                                              "switch one of them off" % other)
            term = "ohem"
        self.seg_criterion = SEG_CRITERIA[self.aux][term](configer=configer)
        self.contrast_criterion = self.contrast_class(configer=configer)

    def forward(self, preds, target, with_embed=False):
        assert "seg" in preds
        if self.aux:
            assert "seg_aux" in preds
        assert "embed" in preds
        seg = preds['seg']
        loss = self.seg_criterion([preds['seg_aux'], seg] if self.aux else seg, target)   # upsample fused into the CE kernel
        queues = {}
        if self.contrast_class.uses_memory_bank:
            queues = {k: preds.get(k) for k in ('segment_queue', 'pixel_queue')}
        if None in queues.values():
            # no queues in `preds` (the validation pass: seg_net(..., is_eval=True) returns seg / embed only): the reference's
            # `loss + 0 * 0` -- a zero scalar on the loss's device, made there without a host round trip
            loss_contrast = loss.new_zeros(())
        else:
            loss_contrast = self.contrast_criterion(preds['embed'], target, seg=seg, seg_ready=preds.get('seg_ready'), **queues)
        # the two terms of the last call, detached (no host sync): the segmentation term is a smooth function of the weights, the
        # contrastive term is not (argmax decides hard / easy, rounding-level changes of the logits move anchors between the sets) --
        # tests that compare two implementations after an SGD step bound the former tightly and the latter loosely
        self.last_terms = (loss.detach(), loss_contrast.detach())
        if with_embed is True:
            return loss + self.loss_weight * loss_contrast
        return loss + 0 * loss_contrast  # same trick as the reference: keeps every parameter in the DDP graph


class ContrastCELoss(_ContrastComposite):
    """'contrast_ce_loss' (reference lib/loss/loss_contrast.py:150-189)."""


class ContrastAuxCELoss(_ContrastComposite):
    """'contrast_auxce_loss' (reference :192-234)."""
    aux = True
