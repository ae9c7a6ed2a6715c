"""tests/exact_cases.py on the CPU emulation of the execution model (tests/emu): the kernel SOURCES, through the autograd-free entry
points of contrastiveseg_amd/kernels.py, on operands that leave nothing to round -- every result must equal the float64 convolution
bit for bit (torch.equal, no tolerance). The derivation is in the docstring of tests/exact_cases.py; the MI355X copy of the same
bodies is tests/test_gpu_exact_operands.py, which runs every configuration (this file runs the ones marked `emu`)."""
import os

import pytest
import torch

from tests import exact_cases as X
from tests.emu import build_emu

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
CPU = torch.device("cpu")


def _K(monkeypatch, arith=X.F16X3, env=None):
    from tests.emu import inject
    from contrastiveseg_amd import kernels as K
    inject.install(monkeypatch)
    X.setup(K, monkeypatch, arith, env)
    return K


@pytest.mark.parametrize("cfg", [c for c in X.CONFIGS if c["emu"]], ids=X.config_id)
def test_exact_operands(cfg, monkeypatch):
    X.run_config(_K(monkeypatch, cfg["arith"], cfg["env"]), CPU, cfg, X.EXACT_KINDS)


@pytest.mark.parametrize("i", X.EPILOGUE_EMU)
def test_epilogues_on_exact_and_degenerate_operands(i, monkeypatch):
    X.run_epilogue(_K(monkeypatch, X.EPILOGUE_CONFIGS[i][2]), CPU, X.EPILOGUE_CONFIGS[i])


@pytest.mark.parametrize("i", X.DEGENERATE_EMU)
def test_degenerate_operands(i, monkeypatch):
    X.run_degenerate(_K(monkeypatch, X.DEGENERATE_CONFIGS[i][2]), CPU, X.DEGENERATE_CONFIGS[i])


@pytest.mark.parametrize("arith", [X.F16X3, X.BF16X6])
def test_all_zero_input_and_gradient_through_autograd(arith, monkeypatch):
    X.run_autograd_zero_input(_K(monkeypatch, arith), CPU)


def test_grouped_launches(monkeypatch):
    X.run_group(_K(monkeypatch), CPU, X.GROUPS[0], X.EXACT_KINDS + ("zero_a", "zero_b"))


def test_fp32_paths(monkeypatch):
    K = _K(monkeypatch)
    X.run_conv3x3_fp32(K, CPU, (2, 48, 48, 9, 12), ("dense", "zero_a"))
    X.run_rgb_stem(K, CPU, (2, 10, 132), ("dense", "zero_b"))
    X.run_classifier(K, CPU, X.CLS_CASES[0], False, ("dense", "zero_a"))
    X.run_classifier(K, CPU, X.CLS_WIDE_CASES[0], True, ("dense", "zero_b"))
    X.run_classifier(K, CPU, X.CLS_WIDE_CASES[1], True, ("dense",))


# ---- the shape lattices (tests/exact_cases.py: LATTICES): the entries marked `emu`, every grouped case, the autograd corners ------------------
@pytest.mark.parametrize("cfg", [c for c in X.LATTICES if c["emu"]], ids=X.lattice_id)
def test_lattice(cfg, monkeypatch):
    assert X.run_lattice(_K(monkeypatch, cfg["arith"], cfg["env"]), CPU, cfg, every=cfg["emu"]) == len(X.lattice_points(cfg)[::cfg["emu"]])


@pytest.mark.parametrize("kind", X.LATTICE_GROUP_KINDS)          # (one kind per test: a 384-channel member costs the emulator seconds)
@pytest.mark.parametrize("shapes", X.LATTICE_GROUPS, ids=X.LATTICE_GROUP_IDS)
def test_lattice_grouped_launches(shapes, kind, monkeypatch):
    X.run_group(_K(monkeypatch), CPU, shapes, (kind,))


def test_lattice_fp32_corners(monkeypatch):
    K = _K(monkeypatch)
    for case in X.FP32_CONV3X3_CORNERS:
        X.run_conv3x3_fp32(K, CPU, case, ("dense", "const"))
    for case in X.RGB_STEM_CORNERS:
        X.run_rgb_stem(K, CPU, case, ("dense", "const"))
    for case in X.CLS_CORNERS:
        X.run_classifier(K, CPU, case, False, ("dense", "const"))
    for case in X.CLS_WIDE_CORNERS:
        X.run_classifier(K, CPU, case, True, ("dense", "const"))


def test_predicates_match_entry_points(monkeypatch):
    K = _K(monkeypatch)
    assert X.run_refusals(K, CPU, monkeypatch, X.setup) > 150


@pytest.mark.parametrize("entry", X.AUTOGRAD_LATTICE, ids=[e[0] for e in X.AUTOGRAD_LATTICE])
def test_autograd_lattice(entry, monkeypatch):
    X.run_autograd_lattice(_K(monkeypatch), CPU, entry)


@pytest.mark.parametrize("case", X.BLOCK_CORNERS)                  # (one corner per test: a 192-channel block costs the emulator seconds)
def test_block_lattice(case, monkeypatch):
    X.run_block_lattice(_K(monkeypatch), CPU, monkeypatch, [case], grouped=False)


@pytest.mark.parametrize("i", range(len(X.BLOCK_GROUPS)))
def test_block_group_lattice(i, monkeypatch):
    X.run_block_lattice(_K(monkeypatch), CPU, monkeypatch, X.BLOCK_GROUPS[i], grouped=True)
