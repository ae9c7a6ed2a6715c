"""Region mutual information loss (lib/loss/rmi_loss.py of the reference: RMILoss.forward -> forward_sigmoid -> rmi_lower_bound)
with the reference's constructor contract, computed by the fused HIP kernels of csrc/rmi.hip (kernels.rmi_loss).

`cls_score` may be at label resolution (what the reference passes) or coarser: the kernels interpolate on the fly with
bilinear(align_corners=True), which is the identity when the sizes match. The label tensor is not modified (the reference rewrites
negative labels to 255 and back in place; here a label is valid when 0 <= label < num_classes, which is the same set)."""
import torch.nn as nn

from contrastiveseg_amd import kernels as K

_KEYS = ("use_sigmoid", "num_classes", "rmi_radius", "rmi_pool_way", "rmi_pool_size", "rmi_pool_stride", "loss_weight_lambda",
         "loss_weight", "lambda_way")


class RMILoss(nn.Module):
    def __init__(self, configer=None):
        super(RMILoss, self).__init__()
        self.configer = configer
        params = configer.get("loss", "params") if configer.exists("loss", "params") else {}
        missing = [k for k in _KEYS if k not in params]
        if missing:
            raise KeyError("RMILoss: loss.params lacks %s" % ", ".join(missing))
        self.use_sigmoid = params["use_sigmoid"]            # read and otherwise unused, as in the reference
        self.num_classes = params["num_classes"]
        self.rmi_radius = params["rmi_radius"]
        self.rmi_pool_way = params["rmi_pool_way"]
        self.rmi_pool_size = params["rmi_pool_size"]
        self.rmi_pool_stride = params["rmi_pool_stride"]
        # the values of every *_RMI.json of the reference; anything else is refused by key name
        for key, want in (("rmi_radius", 3), ("rmi_pool_way", 0), ("rmi_pool_size", 3), ("rmi_pool_stride", 3)):
            if params[key] != want:
                raise NotImplementedError("loss.params.%s = %r: only %r is implemented on the HIP path" % (key, params[key], want))
        self.weight_lambda = params["loss_weight_lambda"]
        self.loss_weight = params["loss_weight"]
        self.lambda_way = params["lambda_way"]
        self.half_d = self.rmi_radius * self.rmi_radius
        self.last_parts = None

    def forward(self, cls_score, label, weight=None, **kwargs):
        if cls_score.shape[1] != self.num_classes:
            raise RuntimeError("RMILoss: loss.params.num_classes = %d but the logits have %d channels"
                               % (self.num_classes, cls_score.shape[1]))
        loss, parts = K.rmi_loss(cls_score, label, self.weight_lambda, self.lambda_way, self.loss_weight, want_terms=True)
        self.last_parts = parts          # f64 [4] on the device: loss, bce, rmi_loss, valid pixels (no host sync)
        return loss
