"""Memory-bank variant: PixelContrastLoss / ContrastCELoss of lib/loss/loss_contrast_mem.py:15-231.

Differences from the bank-free loss (lib/loss/loss_contrast.py of this package) follow the reference:
the contrast set is `cat(segment_queue, pixel_queue, dim=1)` with class 0 skipped and the last 2*ms rows left
zero with label 0 (:91-105), `contrast_count = 1`, and the self mask still removes column i of row i although
the columns are bank entries (:134-138). The bank is read IN PLACE by cseg_contrast_fwd/bwd (mode 2): no
[K*2*ms, D] copy and no N x M temporaries besides the similarity workspace. Anchors get gradients, the bank does
not. Every rank contrasts its own anchors against its own copy of the bank, as in the reference."""
from contrastiveseg_amd import kernels as K  # noqa: F401  (unused here, but oracle/cpu_port.install swaps the `K` of every loss module)
from contrastiveseg_amd.lib.loss import loss_contrast


class PixelContrastLoss(loss_contrast.PixelContrastLoss):
    uses_memory_bank = True      # contrast.device_sampling alone is refused; contrast.device_bank moves sampling and enqueue (loss_contrast.py)

    def forward(self, feats, labels=None, predict=None, queue=None, seg=None, segment_queue=None,
                pixel_queue=None, seg_ready=None):
        """Reference signature is (feats, labels, predict, queue) with queue = cat(segment, pixel) [K, 2*ms, D]
        (:154, :221). Passing the two queues separately avoids that concat. Without queues: the bank-free term."""
        if queue is not None and segment_queue is None:
            ms = queue.shape[1] // 2
            segment_queue = queue[:, :ms].contiguous()
            pixel_queue = queue[:, ms:].contiguous()
        return super(PixelContrastLoss, self).forward(feats, labels, predict=predict, seg=seg, seg_ready=seg_ready,
                                                      segment_queue=segment_queue, pixel_queue=pixel_queue)


class ContrastCELoss(loss_contrast._ContrastComposite):
    """'mem_contrast_ce_loss' (reference :174-231): the contrast term only when `preds` carries both queues."""
    contrast_class = PixelContrastLoss
    reads_lovasz = True


class ContrastAuxCELoss(ContrastCELoss):
    """FSAuxCELoss([seg_aux, seg]) + the memory-bank contrast term: what loss_contrast_mem.py:234-276 of the reference
    sets out to be. As written there it is unregistered, reads the key 'embedding' (the models emit 'embed'), never
    receives the queues and names an un-imported criterion; here it takes the same `preds` dict
    as the registered memory criterion plus 'seg_aux', registered as 'mem_contrast_auxce_loss' for the DeepLab / OCR
    memory models (BASELINE.json configs[3] / [4])."""
    aux = True
