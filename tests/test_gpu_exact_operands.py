"""tests/exact_cases.py on the MI355X: every convolution family of contrastiveseg_amd/kernels.py, in every direction it offers, on
operands that leave nothing to round -- dense small integers, wide impulses (both cross terms of the split, an fp16-subnormal lo
piece, a hi piece that rounds into the next binade), power-of-two magnitudes, all-zero and constant operands. Every comparison is
torch.equal against the float64 convolution; the derivation is in the docstring of tests/exact_cases.py and the emulated-device copy
of the same bodies is tests/test_emu_exact_operands.py."""
import pytest
import torch

from tests import exact_cases as X

pytestmark = pytest.mark.gpu


def _K(monkeypatch, arith=X.F16X3, env=None):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from contrastiveseg_amd import kernels as K
    X.setup(K, monkeypatch, arith, env)
    return K, torch.device("cuda:0")


@pytest.mark.parametrize("cfg", X.CONFIGS, ids=X.config_id)
def test_exact_operands(cfg, monkeypatch):
    K, dev = _K(monkeypatch, cfg["arith"], cfg["env"])
    X.run_config(K, dev, cfg, X.EXACT_KINDS)


@pytest.mark.parametrize("i", range(len(X.EPILOGUE_CONFIGS)))
def test_epilogues_on_exact_and_degenerate_operands(i, monkeypatch):
    K, dev = _K(monkeypatch, X.EPILOGUE_CONFIGS[i][2])
    X.run_epilogue(K, dev, X.EPILOGUE_CONFIGS[i])


@pytest.mark.parametrize("i", range(len(X.DEGENERATE_CONFIGS)))
def test_degenerate_operands(i, monkeypatch):
    K, dev = _K(monkeypatch, X.DEGENERATE_CONFIGS[i][2])
    X.run_degenerate(K, dev, X.DEGENERATE_CONFIGS[i])


@pytest.mark.parametrize("arith", [X.F16X3, X.BF16X6])
def test_all_zero_input_and_gradient_through_autograd(arith, monkeypatch):
    K, dev = _K(monkeypatch, arith)
    X.run_autograd_zero_input(K, dev)


@pytest.mark.parametrize("shapes", X.GROUPS, ids=["2-members", "3-members"])
def test_grouped_launches(shapes, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_group(K, dev, shapes, X.EXACT_KINDS + X.DEGENERATE_KINDS)


@pytest.mark.parametrize("case", [(2, 48, 48, 9, 12), (1, 96, 96, 7, 68), (2, 48, 96, 5, 132)])
def test_fp32_conv3x3(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_conv3x3_fp32(K, dev, case)


@pytest.mark.parametrize("case", [(2, 10, 132), (1, 2, 6), (1, 8, 128)])
def test_fp32_rgb_stem(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_rgb_stem(K, dev, case)


@pytest.mark.parametrize("case", X.CLS_CASES)
def test_fp32_classifier(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_classifier(K, dev, case, wide=False)


@pytest.mark.parametrize("case", X.CLS_WIDE_CASES)
def test_fp32_classifier_wide(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_classifier(K, dev, case, wide=True)


# ---- the shape lattices (tests/exact_cases.py: LATTICES): every entry, every evaluation ------------------------------------------------------
@pytest.mark.parametrize("cfg", X.LATTICES, ids=X.lattice_id)
def test_lattice(cfg, monkeypatch):
    K, dev = _K(monkeypatch, cfg["arith"], cfg["env"])
    assert X.run_lattice(K, dev, cfg) == len(X.lattice_points(cfg))


@pytest.mark.parametrize("shapes", X.LATTICE_GROUPS, ids=X.LATTICE_GROUP_IDS)
def test_lattice_grouped_launches(shapes, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_group(K, dev, shapes, X.LATTICE_GROUP_KINDS)


@pytest.mark.parametrize("case", X.FP32_CONV3X3_CORNERS)
def test_lattice_fp32_conv3x3(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_conv3x3_fp32(K, dev, case)


@pytest.mark.parametrize("case", X.RGB_STEM_CORNERS)
def test_lattice_fp32_rgb_stem(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_rgb_stem(K, dev, case)


@pytest.mark.parametrize("case", X.CLS_CORNERS)
def test_lattice_fp32_classifier(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_classifier(K, dev, case, wide=False)


@pytest.mark.parametrize("case", X.CLS_WIDE_CORNERS)
def test_lattice_fp32_classifier_wide(case, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_classifier(K, dev, case, wide=True)


def test_predicates_match_entry_points(monkeypatch):
    K, dev = _K(monkeypatch)
    assert X.run_refusals(K, dev, monkeypatch, X.setup) > 150


@pytest.mark.parametrize("entry", X.AUTOGRAD_LATTICE, ids=[e[0] for e in X.AUTOGRAD_LATTICE])
def test_autograd_lattice(entry, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_autograd_lattice(K, dev, entry)


def test_block_lattice(monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_block_lattice(K, dev, monkeypatch, X.BLOCK_CORNERS, grouped=False)


@pytest.mark.parametrize("i", range(len(X.BLOCK_GROUPS)))
def test_block_group_lattice(i, monkeypatch):
    K, dev = _K(monkeypatch)
    X.run_block_lattice(K, dev, monkeypatch, X.BLOCK_GROUPS[i], grouped=True)
