"""Anchor mining at its edges (csrc/mining.hip): cseg_classify_partition through both entries of kernels.classify_partition,
cseg_gather_anchors through kernels.gather_anchors and kernels.GatherAnchors, cseg_scatter_anchor_grad called as PixelContrast.backward
calls it. Everything is compared for exact equality: labels with torch-CPU F.interpolate(nearest), the argmax with torch-CPU torch.max
(NaN, ties, -inf, +inf planted), the hard / easy lists with np.nonzero order, gathered rows with embed[b, :, pix], the scattered
gradient with np.float32 arithmetic in the kernel's order. Cases, plants and references: tests/loss_edge_cases.py; the same bodies run
on the emulated device in tests/test_emu_cabi.py."""
import pytest
import torch

from tests import loss_edge_cases as L

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("i", range(len(L.MINING_SHAPES)), ids=["x".join(map(str, s)) for s, _ in L.MINING_SHAPES])
def test_classify_partition_edges(i):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_classify_partition(K, dev, i)


@pytest.mark.parametrize("N", L.GATHER_N)
@pytest.mark.parametrize("D", L.GATHER_D)
def test_gather_anchors_equals_indexing(D, N):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_gather(K, dev, D, N)


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("n_parts", [1, 3])
def test_scatter_anchor_grad_is_bit_exact(n_parts, scale):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_scatter(K, dev, n_parts, scale)
