"""The memory-bank kernels beyond the first chunk of 32 classes (csrc/queue.hip): cseg_queue_count and cseg_queue_class_sums at K up to
300 against float64 numpy on labels[:, ::stride, ::stride] (counts exact, sums within the bound of their operation count),
cseg_queue_write_segments / cseg_queue_write_pixels against float64 x / max(|x|, 1e-12) with every unnamed bank row bit-identical, and
Trainer._dequeue_and_enqueue at the 171-class bank of configs/coco_stuff/H_48_D_4_MEM.json against the oracle's restatement of the
reference. Cases and references: tests/loss_edge_cases.py; the same bodies run on the emulated device in tests/test_emu_cabi.py."""
import pytest
import torch

from tests import loss_edge_cases as L

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("i", range(len(L.BANK_SHAPES)), ids=["-".join(map(str, s)) for s in L.BANK_SHAPES])
def test_queue_count_and_class_sums(i):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_bank_count_and_sums(K, dev, i)


@pytest.mark.parametrize("D", L.BANK_WRITE_D)
def test_queue_write_segments(D):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_bank_write_segments(K, dev, D)


@pytest.mark.parametrize("D", L.BANK_WRITE_D)
def test_queue_write_pixels(D):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_bank_write_pixels(K, dev, D)


def test_trainer_enqueue_at_171_classes_matches_oracle():
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    L.run_enqueue_wide(K, dev)
