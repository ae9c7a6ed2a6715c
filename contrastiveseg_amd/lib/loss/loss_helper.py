"""Segmentation criteria on the hot path: FSCELoss / FSAuxCELoss with the reference's constructor contract
(lib/loss/loss_helper.py:169-212, 301-313), computed by the fused upsample+CE HIP kernel
(cseg_upsample_ce_fwd/bwd) instead of F.interpolate + nn.CrossEntropyLoss.

`inputs` may be at label resolution (what the reference passes) or coarser: the kernel interpolates on the fly
with bilinear(align_corners=True), which is the identity when the sizes match."""
import torch
import torch.nn as nn

from contrastiveseg_amd import kernels as K
from contrastiveseg_amd.lib.loss.rmi_loss import RMILoss


def _ce_params(configer):
    weight, reduction, ignore_index = None, "elementwise_mean", -1
    if configer.exists("loss", "params"):
        p = configer.get("loss", "params")
        if "ce_weight" in p:
            weight = torch.tensor(p["ce_weight"], dtype=torch.float32)
        if "ce_reduction" in p:
            reduction = p["ce_reduction"]
        if "ce_ignore_index" in p:
            ignore_index = p["ce_ignore_index"]
    return weight, reduction, ignore_index


class FSCELoss(nn.Module):
    def __init__(self, configer=None):
        super(FSCELoss, self).__init__()
        self.configer = configer
        weight, reduction, ignore_index = _ce_params(configer)
        if reduction not in ("elementwise_mean", "mean"):
            raise NotImplementedError("ce_reduction %r: only the mean reduction of the shipped configs is "
                                      "implemented on the HIP path" % reduction)
        self.register_buffer("weight", weight, persistent=False)
        self.register_buffer("status", torch.zeros(4, dtype=torch.int32), persistent=False)
        self.ignore_index = ignore_index

    def _one(self, inp, target):
        return K.upsample_ce(inp, target, self.weight, self.ignore_index, self.status)

    def bad_label_count(self, reset=True):
        """Labels seen since the last call that are neither `ce_ignore_index` nor a class id: the kernel drops them
        (nn.CrossEntropyLoss of the reference would assert). One D2H copy: call it where the host syncs anyway
        (Trainer._display reads the same counters through bad_label_total, with the loss, and raises)."""
        n = int(self.status[1])
        if reset:
            self.status.zero_()
        return n

    def forward(self, inputs, *targets, weights=None, **kwargs):
        if isinstance(inputs, (tuple, list)):
            if weights is None:
                weights = [1.0] * len(inputs)
            loss = 0.0
            for i, inp in enumerate(inputs):
                tgt = targets[i] if len(targets) > 1 else targets[0]
                loss = loss + weights[i] * self._one(inp, tgt)
            return loss
        return self._one(inputs, targets[0])


class FSRMILoss(nn.Module):
    """RMILoss on the segmentation map (reference :360-369)."""

    def __init__(self, configer=None):
        super(FSRMILoss, self).__init__()
        self.configer = configer
        self.rmi_loss = RMILoss(self.configer)

    def forward(self, inputs, targets, **kwargs):
        return self.rmi_loss(inputs, targets)


class FSCELOVASZLoss(nn.Module):
    """CE + Lovasz-softmax on the segmentation map (reference :77-124, lib/loss/lovasz_loss.py:216-267): the fused upsample+CE kernel
    plus the sort + scan kernels of csrc/lovasz.hip, both on the coarse logits. Same constructor contract as FSCELoss (ce_weight,
    ce_reduction, ce_ignore_index; the weights apply to the CE part only, as in the reference). The reference's list / tuple branch
    (CE only, no Lovasz term) has no caller in this package and is refused."""

    def __init__(self, configer=None):
        super(FSCELOVASZLoss, self).__init__()
        self.configer = configer
        self.ce_loss = FSCELoss(self.configer)
        self.ignore_index = self.ce_loss.ignore_index

    def bad_label_count(self, reset=True):
        """FSCELoss.bad_label_count of the CE part: both parts see the same labels and drop the same ones; the CE kernel counts."""
        return self.ce_loss.bad_label_count(reset)

    def forward(self, inputs, *targets, weights=None, **kwargs):
        if isinstance(inputs, dict) and "seg" in inputs:
            inputs = inputs["seg"]
        if isinstance(inputs, (tuple, list)):
            raise NotImplementedError("FSCELOVASZLoss: a list / tuple of maps (the reference applies CE only there) is not "
                                      "implemented; pass the segmentation map or a dict with 'seg'")
        return self.ce_loss(inputs, targets[0]) + K.lovasz_softmax(inputs, targets[0], ignore_index=self.ignore_index)


class FSOhemCELoss(FSCELoss):
    """Cross entropy over the hard pixels only (reference :215-261): among the valid pixels, those whose probability of the true class
    lies below max(ohem_thresh, the probability of rank min(ohem_minkeep, n - 1) in ascending order), averaged over their count (not over
    the sum of ce_weight as FSCELoss). Computed by the kernels of csrc/ohem.hip on the coarse logits. The reference's constructor contract:
    loss.params.ohem_thresh and ohem_minkeep are required, max(1, ohem_minkeep) is applied, ce_weight / ce_reduction / ce_ignore_index as
    FSCELoss (the mean reduction only). Takes the segmentation map or the trainer's dict with 'seg'. When no pixel is kept the loss is NaN
    (kernels.ohem_ce). An FSCELoss, so that bad_label_count / bad_label_total see its `status`."""

    def __init__(self, configer=None):
        super(FSOhemCELoss, self).__init__(configer)
        params = configer.get("loss", "params") if configer.exists("loss", "params") else {}
        for key in ("ohem_thresh", "ohem_minkeep"):
            if key not in params:
                raise KeyError("FSOhemCELoss: loss.params.%s is required" % key)
        self.thresh = float(params["ohem_thresh"])
        self.min_kept = max(1, int(params["ohem_minkeep"]))

    def _one(self, inp, target):
        return K.ohem_ce(inp, target, self.weight, self.ignore_index, self.thresh, self.min_kept, self.status)

    def forward(self, inputs, *targets, **kwargs):
        if isinstance(inputs, dict) and "seg" in inputs:
            inputs = inputs["seg"]
        return super(FSOhemCELoss, self).forward(inputs, *targets, **kwargs)


class _FSAuxLoss(nn.Module):
    """term(seg) * w_seg + ce(aux) * w_aux (reference :301-329): `ce_loss` always takes the auxiliary map; the sub-module `seg_name`
    takes the segmentation map -- `ce_loss` again, or an instance of `seg_class` built next to it."""
    seg_name, seg_class = "ce_loss", None

    def __init__(self, configer=None):
        super(_FSAuxLoss, self).__init__()
        self.configer = configer
        self.ce_loss = FSCELoss(self.configer)
        if self.seg_class is not None:
            setattr(self, self.seg_name, self.seg_class(self.configer))

    def forward(self, inputs, targets, **kwargs):
        aux_out, seg_out = inputs
        seg_loss = getattr(self, self.seg_name)(seg_out, targets)
        aux_loss = self.ce_loss(aux_out, targets)
        lw = self.configer.get("network", "loss_weights")
        return lw["seg_loss"] * seg_loss + lw["aux_loss"] * aux_loss


class FSAuxCELoss(_FSAuxLoss):
    """ce(seg) * w_seg + ce(aux) * w_aux (reference :301-313)."""


class FSAuxRMILoss(_FSAuxLoss):
    """rmi(seg) * w_seg + ce(aux) * w_aux (reference :316-329): CE on the auxiliary map through the fused upsample+CE kernel, RMI
    on the segmentation map through the fused RMI kernels."""
    seg_name, seg_class = "rmi_loss", RMILoss


class FSAuxCELOVASZLoss(_FSAuxLoss):
    """(ce + lovasz)(seg) * w_seg + ce(aux) * w_aux: the analogue of FSAuxRMILoss. The reference has no such class -- its only
    Lovasz criterion for the contrast losses is FSCELOVASZLoss in the registered memory criterion; this is the project's own composite
    for mem_contrast_auxce_loss (the DeepLab / OCR memory models, whose auxiliary map gets the plain CE as everywhere else)."""
    seg_name, seg_class = "lovasz_loss", FSCELOVASZLoss


class FSAuxOhemCELoss(_FSAuxLoss):
    """ohem(seg) * w_seg + ce(aux) * w_aux (reference :264-298): plain CE on the auxiliary map, hard-pixel mining on the segmentation map."""
    seg_name, seg_class = "ohem_ce_loss", FSOhemCELoss


def bad_label_total(criterion, device=None):
    """Device scalar (int32, nothing read back): the labels the CE kernels under `criterion` dropped since their counters were last
    reset, summed over the FSCELoss instances -- the modules that own a `status` counter (FSCELOVASZLoss and the aux composites
    forward to theirs). `device`: where the zero lives when `criterion` holds no FSCELoss at all (contrast_ce_loss under use_rmi)."""
    return sum((m.status[1] for m in criterion.modules() if isinstance(m, FSCELoss)),
               torch.zeros((), dtype=torch.int32, device=device))
