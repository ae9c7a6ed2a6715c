"""The bilinear exchange kernels at their edges: upsample + concat (csrc/upcat.hip), the fused sum with ReLU and the n-ary sum
(csrc/fuse.hip) and their adjoint (csrc/cseg_bilinear.h) on all five routes -- band kernels with 8, 12, 24, 40 taps and the gather
kernel, each asserted through cseg_bilinear_adjoint_plan -- against float64 on the kernel's own fp32 taps, with a pointwise bound that
admits the two legal roundings of the tap weight and nothing else; pass-through channels, same-resolution gradients, the three routes
of cseg_fuse_sum_bwd and the n-ary sum bit for bit; planted zero stripes and NaNs; refusals. Cases, references and bounds:
tests/exchange_cases.py; the same bodies run on the emulated device in tests/test_emu_exchange_edges.py."""
import pytest
import torch

from tests import exchange_cases as X

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def test_every_route_is_taken_for_its_own_reason():
    _dev()
    from contrastiveseg_amd import kernels as K
    X.check_route_reasons(K)


@pytest.mark.parametrize("name", list(X.UPCAT_CASES))
def test_upsample_concat_edges_match_float64_on_the_kernels_taps(name):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    X.run_upcat(K, dev, name)


@pytest.mark.parametrize("name", list(X.FUSE_CASES))
def test_fuse_sum_relu_edges_match_float64_on_the_kernels_taps(name, monkeypatch):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    X.run_fuse(K, dev, name, monkeypatch)


@pytest.mark.parametrize("w", [8, 7])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_nary_sum_is_the_left_to_right_fp32_sum(n, w):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    X.run_sum(K, dev, n, w)


def test_fan_out_of_five_falls_back_to_torch_adds():
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    X.run_fanout_fallback(K, dev)


@pytest.mark.parametrize("what", list(X.REFUSALS))
def test_exchange_refusals(what):
    dev = _dev()
    from contrastiveseg_amd import kernels as K
    X.run_refusal(K, dev, what)
