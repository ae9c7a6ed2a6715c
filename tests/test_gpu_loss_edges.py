"""The contrastive term away from unit-norm rows (csrc/contrast.hip) and the fused upsample + cross entropy at its limits
(csrc/upsample_ce.hip). Contrast: kernels.ContrastOnAnchors with the three-launch and the fused forward, loss and anchor gradient
against the float64 oracle (O._contrast_core) on logits near -130, +57 and +128, a bank whose zero tail holds the row maximum, N = 2 and a
singleton class (NaN in both); refusals of the host-side checks. Upsample-CE: h = 1, w = W = 1, 17 pixels per cell, logits x 200, a
zero-weight class alone in a row, labels outside [0, K), an all-ignored target, against torch-CPU float64 and the oracle. Cases and
references: tests/loss_edge_cases.py; the same bodies run on the emulated device in tests/test_emu_cabi.py."""
import pytest
import torch

from tests import loss_edge_cases as L

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("name", list(L.CONTRAST_CASES))
def test_contrast_edges_match_float64_oracle(name, fused, monkeypatch):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_contrast(K, dev, name, fused, monkeypatch)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("what", L.CONTRAST_REFUSALS)
def test_contrast_refusals(what, fused, monkeypatch):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_contrast_refusal(K, dev, what, fused, monkeypatch)


@pytest.mark.parametrize("name", list(L.CE_CASES))
def test_upsample_ce_edges_match_torch_float64_and_oracle(name):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_upsample_ce(K, dev, name)


def test_upsample_ce_refuses_40_pixels_on_one_tap():
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_upsample_ce_refusal(K, dev)
