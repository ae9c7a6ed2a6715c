"""The GPU parity tests (tests/test_gpu_*.py), replayed on CPU with the "device" being the CPU emulation of the execution
model: contrastiveseg_amd._hip is pointed at libcseg_emu.so (tests/emu/inject.py), the test modules' `_dev()` returns the
CPU, and the SAME test bodies run -- autograd wrappers of contrastiveseg_amd/kernels.py, the C-ABI, and the HIP sources
of every kernel family -- against the same oracles: the reference-generated golden vectors (bit-exact mined indices,
losses, gradients), the numpy oracle, torch fp64. Cases are the GPU tests' own parametrisations, minus the shapes that
are too large for an emulation that switches fibers at every wave-level operation.
What this proves: the kernel sources are functionally right under the documented execution model. What it cannot: speed,
and hazards that exist only on the hardware."""
import importlib
import itertools
import os
import sys

import pytest
import torch

from tests.emu import build_emu, inject

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _cases(module, func, keep=lambda kw: True):
    """The parametrisations pytest would generate for tests/<module>.py::<func>, as dicts, filtered by `keep`."""
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    fn = getattr(importlib.import_module(module), func)
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [n.strip() for n in mark.args[0].split(",")]
        rows = []
        for v in mark.args[1]:
            v = getattr(v, "values", v)                  # pytest.param(...)
            if len(names) == 1 and not (isinstance(v, tuple) and len(v) == 1 and False):
                v = (v,) if len(names) == 1 else v
            rows.append(dict(zip(names, v)))
        axes.append(rows)
    out = []
    for combo in itertools.product(*axes) if axes else [()]:
        kw = {}
        for d in combo:
            kw.update(d)
        if keep(kw):
            out.append(kw)
    return out


def _ids(cases):
    return ["-".join(str(v) for v in kw.values()) or "all" for kw in cases]


def _replay(monkeypatch, module, func, kw, fixtures=()):
    inject.install(monkeypatch)
    mod = importlib.import_module(module)
    monkeypatch.setattr(mod, "_dev", lambda: torch.device("cpu"))
    kw = dict(kw)
    if "golden_dir" in fixtures:
        kw["golden_dir"] = GOLDEN
    getattr(mod, func)(**kw)


# ---- loss path: mining, contrast (self / memory bank), fused upsample + CE, against the reference's golden vectors ---------
LOSS = _cases("test_gpu_kernels", "test_criterion_matches_reference_golden", lambda kw: not kw["name"].startswith("cfg2"))


@pytest.mark.parametrize("kw", LOSS, ids=_ids(LOSS))
def test_criterion_matches_reference_golden(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_criterion_matches_reference_golden", kw, ("golden_dir",))


@pytest.mark.slow
def test_criterion_at_the_benched_shapes_matches_reference_golden(monkeypatch):
    """BASELINE configs[1] shapes (8 x 19 x 128 x 256 logits, 256-d embeddings, 512 x 1024 labels): mined indices bit-exact,
    loss, gradient slices -- the HIP sources against the reference's own numbers, on the emulator."""
    _replay(monkeypatch, "test_gpu_kernels", "test_criterion_matches_reference_golden", {"name": "cfg2_full"}, ("golden_dir",))


PART = _cases("test_gpu_kernels", "test_classify_partition_matches_oracle")


@pytest.mark.parametrize("kw", PART, ids=_ids(PART))
def test_classify_partition_matches_oracle(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_classify_partition_matches_oracle", kw)


SELF = _cases("test_gpu_kernels", "test_contrast_self_matches_oracle", lambda kw: kw["T"] * kw["V"] * kw["D"] <= 152 * 6 * 256)
BANK = _cases("test_gpu_kernels", "test_contrast_bank_matches_oracle")


@pytest.mark.parametrize("kw", SELF, ids=_ids(SELF))
def test_contrast_self_matches_oracle(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_contrast_self_matches_oracle", kw)


@pytest.mark.parametrize("kw", BANK, ids=_ids(BANK))
def test_contrast_bank_matches_oracle(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_contrast_bank_matches_oracle", kw)


FUSED = _cases("test_gpu_kernels", "test_contrast_fused_forward_equals_the_three_launches")


@pytest.mark.parametrize("kw", FUSED, ids=_ids(FUSED))
def test_contrast_fused_forward_equals_the_three_launches(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_contrast_fused_forward_equals_the_three_launches", dict(kw, monkeypatch=monkeypatch))


def test_upsample_concat_and_fuse_sum_match_torch(monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_upsample_concat_matches_torch", {})
    _replay(monkeypatch, "test_gpu_kernels", "test_fuse_sum_relu_matches_torch", {"monkeypatch": monkeypatch})


CLS = _cases("test_gpu_cls1x1", "test_classifier_with_folded_dropout_matches_the_reference_modules")


@pytest.mark.parametrize("kw", CLS, ids=_ids(CLS))
def test_classifier_with_folded_dropout_matches_the_reference_modules(kw, monkeypatch):
    """csrc/cls1x1.hip (forward, backward-data, weight gradient) under module_helper.FoldedDropout2d + ClassifierConv1x1"""
    _replay(monkeypatch, "test_gpu_cls1x1", "test_classifier_with_folded_dropout_matches_the_reference_modules", dict(kw, monkeypatch=monkeypatch))


@pytest.mark.parametrize("bn_training", [True, False])
def test_bias_gradient_of_a_convolution_in_front_of_batchnorm(bn_training, monkeypatch):
    _replay(monkeypatch, "test_gpu_cls1x1", "test_bias_gradient_of_a_convolution_in_front_of_batchnorm",
            {"bn_training": bn_training, "monkeypatch": monkeypatch})


def test_bottleneck_skip_gradient_in_the_epilogue_is_bit_identical(monkeypatch):
    _replay(monkeypatch, "test_gpu_cls1x1", "test_bottleneck_skip_gradient_in_the_epilogue_is_bit_identical", {"monkeypatch": monkeypatch})


def test_classifier_eval_mode_and_fallbacks(monkeypatch):
    _replay(monkeypatch, "test_gpu_cls1x1", "test_classifier_eval_mode_and_fallbacks", {"monkeypatch": monkeypatch})


CE = _cases("test_gpu_kernels", "test_upsample_ce_matches_torch_and_oracle", lambda kw: kw["B"] * kw["H"] * kw["W"] <= 2 * 256 * 512)


@pytest.mark.parametrize("kw", CE, ids=_ids(CE))
def test_upsample_ce_matches_torch_and_oracle(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_upsample_ce_matches_torch_and_oracle", kw)


def test_upsample_ce_forward_without_a_status_buffer(monkeypatch):
    """cseg_upsample_ce_fwd through the C ABI with status = NULL and a label equal to K: the bad label is dropped as it is with a status
    buffer (the same loss, bit for bit), it is just not counted; with the buffer the count is 1 (the ignore index is not a bad label)."""
    import ctypes
    from contrastiveseg_amd import _hip
    inject.install(monkeypatch)
    B, K, h, w, H, W, ignore = 1, 3, 2, 2, 4, 4, -1
    g = torch.Generator().manual_seed(17)
    seg = torch.randn(B, K, h, w, generator=g)
    target = torch.randint(0, K, (B, H, W), generator=g)
    target[0, 1, 2] = K
    target[0, 3, 0] = ignore
    nb = _hip.lib().cseg_upsample_ce_blocks(B, H, W)

    def forward(status):
        partial, out, lse = torch.empty(2 * nb), torch.empty(2), torch.empty(B, H, W)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
        _hip.call("cseg_upsample_ce_fwd", ptr(seg), ptr(target), None, ignore, B, K, h, w, H, W, ptr(partial), ptr(out), ptr(status),
                  ptr(lse), None)
        return out

    status = torch.zeros(4, dtype=torch.int32)
    with_status, without = forward(status), forward(None)
    assert torch.isfinite(with_status).all() and float(with_status[1]) == H * W - 2
    assert torch.equal(without.view(torch.int32), with_status.view(torch.int32))
    assert status.tolist() == [0, 1, 0, 0]


ENQ = _cases("test_gpu_kernels", "test_trainer_enqueue_on_gpu_matches_reference_golden")


@pytest.mark.parametrize("kw", ENQ, ids=_ids(ENQ))
def test_queue_update_matches_reference_golden(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_kernels", "test_trainer_enqueue_on_gpu_matches_reference_golden", kw, ("golden_dir",))


# ---- mining, memory bank, contrastive term and upsample-CE at their edges (tests/loss_edge_cases.py), every parametrisation ----------
def _edge(module, func):
    cases = _cases(module, func)
    wants_mp = "monkeypatch" in getattr(importlib.import_module(module), func).__code__.co_varnames

    def decorate(body):
        return pytest.mark.parametrize("kw", cases, ids=_ids(cases))(body)
    return decorate, (lambda kw, monkeypatch: _replay(monkeypatch, module, func, dict(kw, monkeypatch=monkeypatch) if wants_mp else kw))


_P, _R_PART = _edge("test_gpu_mining_edges", "test_classify_partition_edges")
_G, _R_GATHER = _edge("test_gpu_mining_edges", "test_gather_anchors_equals_indexing")
_S, _R_SCATTER = _edge("test_gpu_mining_edges", "test_scatter_anchor_grad_is_bit_exact")
_QS, _R_QSUMS = _edge("test_gpu_queue_edges", "test_queue_count_and_class_sums")
_QW, _R_QSEG = _edge("test_gpu_queue_edges", "test_queue_write_segments")
_QP, _R_QPIX = _edge("test_gpu_queue_edges", "test_queue_write_pixels")
_QE, _R_QENQ = _edge("test_gpu_queue_edges", "test_trainer_enqueue_at_171_classes_matches_oracle")
_CC, _R_CON = _edge("test_gpu_loss_edges", "test_contrast_edges_match_float64_oracle")
_CR, _R_CONREF = _edge("test_gpu_loss_edges", "test_contrast_refusals")
_UC, _R_CE = _edge("test_gpu_loss_edges", "test_upsample_ce_edges_match_torch_float64_and_oracle")
_UR, _R_CEREF = _edge("test_gpu_loss_edges", "test_upsample_ce_refuses_40_pixels_on_one_tap")


@_P
def test_classify_partition_edges(kw, monkeypatch):
    _R_PART(kw, monkeypatch)


@_G
def test_gather_anchors_equals_indexing(kw, monkeypatch):
    _R_GATHER(kw, monkeypatch)


@_S
def test_scatter_anchor_grad_is_bit_exact(kw, monkeypatch):
    _R_SCATTER(kw, monkeypatch)


@_QS
def test_queue_count_and_class_sums(kw, monkeypatch):
    _R_QSUMS(kw, monkeypatch)


@_QW
def test_queue_write_segments(kw, monkeypatch):
    _R_QSEG(kw, monkeypatch)


@_QP
def test_queue_write_pixels(kw, monkeypatch):
    _R_QPIX(kw, monkeypatch)


@_QE
def test_trainer_enqueue_at_171_classes_matches_oracle(kw, monkeypatch):
    _R_QENQ(kw, monkeypatch)


@_CC
def test_contrast_edges_match_float64_oracle(kw, monkeypatch):
    _R_CON(kw, monkeypatch)


@_CR
def test_contrast_refusals(kw, monkeypatch):
    _R_CONREF(kw, monkeypatch)


@_UC
def test_upsample_ce_edges_match_torch_float64_and_oracle(kw, monkeypatch):
    _R_CE(kw, monkeypatch)


@_UR
def test_upsample_ce_refuses_40_pixels_on_one_tap(kw, monkeypatch):
    _R_CEREF(kw, monkeypatch)


# ---- fused BatchNorm (+ residual, + ReLU), forward / backward / running statistics against torch fp64 ---------------------
BN = _cases("test_gpu_bn", "test_fused_bn_matches_torch_fp64", lambda kw: kw["shape"][0] * kw["shape"][1] * kw["shape"][2] * kw["shape"][3] <= 1 << 20)


@pytest.mark.parametrize("kw", BN, ids=_ids(BN))
def test_fused_bn_matches_torch_fp64(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_bn", "test_fused_bn_matches_torch_fp64", kw)


# ---- fp32-MFMA 3x3 convolution (forward, backward-data, weight gradient) ----------------------------------------------------
C33 = _cases("test_gpu_conv3x3", "test_conv3x3_matches_fp64", lambda kw: kw["B"] * kw["H"] * kw["W"] <= 2048)


@pytest.mark.parametrize("kw", C33, ids=_ids(C33))
def test_conv3x3_fp32_mfma_matches_fp64(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_conv3x3", "test_conv3x3_matches_fp64", kw)


# ---- fused augmentation kernel of the data pipeline ------------------------------------------------------------------------
AUG = _cases("test_gpu_aug", "test_augment_kernel_matches_forward_chain", lambda kw: kw["B"] * kw["Ht"] * kw["Wt"] <= 4 * 64 * 128)


@pytest.mark.parametrize("kw", AUG, ids=_ids(AUG))
def test_augment_kernel_matches_forward_chain(kw, monkeypatch):
    _replay(monkeypatch, "test_gpu_aug", "test_augment_kernel_matches_forward_chain", kw)


# ---- split-bf16 convolutions: the GPU tests of tests/test_gpu_conv3x3_sb.py (they call .cuda() directly) -------------------
def _replay_sb(monkeypatch, func, kw, env=()):
    inject.install(monkeypatch)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    for k, v in env:
        monkeypatch.setenv(k, v)
    mod = importlib.import_module("test_gpu_conv3x3_sb")
    fn = getattr(mod, func)
    if "monkeypatch" in fn.__code__.co_varnames[:fn.__code__.co_argcount]:
        kw = dict(kw, monkeypatch=monkeypatch)
    fn(**kw)


_SMALL = lambda kw: kw["case"][1] <= 192          # (the 720-channel case runs in tests/test_emu_sb_kernels.py, marked slow)
SB_AUTO = _cases("test_gpu_conv3x3_sb", "test_autograd_matches_fp64", _SMALL)


@pytest.mark.parametrize("wrw", ["0", "1", "2"])
@pytest.mark.parametrize("kw", SB_AUTO, ids=_ids(SB_AUTO))
def test_sb_autograd_matches_fp64(kw, wrw, monkeypatch):
    """Conv3x3SplitBF16 end to end (forward, backward-data, weight / bias gradient) with the weight gradient on MIOpen's
    stand-in (0), the split-bf16 kernel version 1 and version 2."""
    from contrastiveseg_amd import kernels as K
    monkeypatch.setattr(K, "CONV3X3_SB_WRW", wrw != "0")
    _replay_sb(monkeypatch, "test_autograd_matches_fp64", kw, [("CSEG_CONV3X3_SB_WRW_V", wrw)] if wrw != "0" else [])


SB_HEAD8 = _cases("test_gpu_conv3x3_sb", "test_head_kernel_8_rows_matches_fp64", _SMALL)


@pytest.mark.parametrize("kw", SB_HEAD8, ids=_ids(SB_HEAD8))
def test_head_kernel_8_rows_matches_fp64(kw, monkeypatch):
    _replay_sb(monkeypatch, "test_head_kernel_8_rows_matches_fp64", kw)


SB_FORK = _cases("test_gpu_conv3x3_sb", "test_basic_block_with_fused_identity_gradient", lambda kw: True)


@pytest.mark.parametrize("kw", SB_FORK, ids=_ids(SB_FORK))
def test_basic_block_with_fused_identity_gradient(kw, monkeypatch):
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    _replay_sb(monkeypatch, "test_basic_block_with_fused_identity_gradient", kw)


SB_ONE = _cases("test_gpu_conv3x3_sb", "test_pointwise_matches_fp64", _SMALL)


@pytest.mark.parametrize("wrw", [False, True])
@pytest.mark.parametrize("kw", SB_ONE, ids=_ids(SB_ONE))
def test_sb_pointwise_autograd_matches_fp64(kw, wrw, monkeypatch):
    from contrastiveseg_amd import kernels as K
    monkeypatch.setattr(K, "CONV1X1_SB_WRW", wrw)
    _replay_sb(monkeypatch, "test_pointwise_matches_fp64", kw)


# ---- stride-2 convolutions: the module-level GPU test of tests/test_gpu_conv3x3_s2.py on the emulated device -----------------------
S2_MOD = _cases("test_gpu_conv3x3_s2", "test_stride2_module_matches_fp64", lambda kw: kw["case"][1] * kw["case"][2] <= 96 * 192)


@pytest.mark.parametrize("kw", S2_MOD, ids=_ids(S2_MOD))
def test_stride2_module_matches_fp64(kw, monkeypatch):
    """Conv3x3(cin, cout, 2) end to end: SplitWeights' batched packs in both stride-2 formats, the three kernels, the routing."""
    inject.install(monkeypatch)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    mod = importlib.import_module("test_gpu_conv3x3_s2")
    mod.test_stride2_module_matches_fp64(monkeypatch=monkeypatch, **kw)


def test_transition_256_to_48_module_matches_fp64(monkeypatch):
    inject.install(monkeypatch)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    importlib.import_module("test_gpu_conv3x3_s2").test_transition_256_to_48_module_matches_fp64(monkeypatch=monkeypatch)


# ---- row-sparse projection-head backward with the PRODUCT's deposit path (kernels.PixelContrast / GatherAnchors) ---------
@pytest.mark.parametrize("loss_type", ["contrast_ce_loss", "mem_contrast_ce_loss"])
def test_sparse_embed_route_equals_dense_route(loss_type, monkeypatch):
    """tests/test_gpu_sparse_embed.py at the head's real width (720 -> 720 -> 256, 19 classes, up to 1024 anchors): HIP BN,
    mining, contrast and CE sources on the emulator, torch's CPU GEMMs standing in for rocBLAS."""
    inject.install(monkeypatch)
    mod = importlib.import_module("test_gpu_sparse_embed")
    monkeypatch.setattr(mod, "_dev", lambda: torch.device("cpu"))
    mod.test_sparse_route_equals_dense_route_on_the_gpu(loss_type, monkeypatch)


# ---- whole train steps: Trainer -> registry -> criterion -> backward -> SGD (+ memory-bank update), every model family ------
def _trainer_losses(case, install):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    model, backbone, loss, cfg_file, contrast = case
    install()
    cfg = Configer(configs=os.path.join(os.path.dirname(HERE), "configs", cfg_file))
    cfg.update(["network", "backbone"], backbone)
    cfg.update(["network", "model_name"], model)
    cfg.update(["loss", "loss_type"], loss)
    cfg.update(["data", "num_classes"], 7)
    cfg.get("loss", "params").pop("ce_weight", None)
    cfg.update(["train", "batch_size"], 2)
    cfg.get("train", "data_transformer")["input_size"] = [128, 64]
    cfg.update(["contrast", "warmup_iters"], 0)
    cfg.update(["contrast", "max_views"], 1 if "mem" in loss else 6)
    for k, v in contrast.items():
        cfg.update(["contrast", k], v)
    cfg.update(["solver", "max_iters"], 2)
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    tr.seg_net.train()
    for m in tr.seg_net.modules():
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)):
            m.p = 0.0
    torch.manual_seed(5)
    losses, w = [], None
    for b in SyntheticLoader(cfg, torch.device("cpu"), length=2, seed=3, mode="blocky"):
        losses.append(float(tr.train_step(b)))
        if w is None:                                # after the FIRST update: one backward through the whole network
            w = torch.cat([p.detach().reshape(-1)[:256] for p in list(tr.seg_net.parameters())[::8] if p.dim() > 1])
    return losses, w


TRAIN = list(importlib.import_module("test_gpu_train_step").CASES) if HERE in sys.path or sys.path.insert(0, HERE) is None else []


_EVERY_FAMILY = os.environ.get("CSEG_EMU_ALL") == "1"       # default: two of the six families (20 s each on 8 cores)


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.skipif(
    not _EVERY_FAMILY and c[0] not in ("hrnet_w48_contrast", "deeplab_v3_mem"), reason="set CSEG_EMU_ALL=1 for every family"))
    for c in TRAIN], ids=[c[0] + "-" + c[2] for c in TRAIN])
def test_train_steps_on_the_emulated_device_equal_the_torch_restatement(case, monkeypatch):
    """Two trainer steps of each model family / criterion with the device half = the HIP sources on the emulator, against
    the same two steps with the device half = oracle/cpu_port.py (the torch restatement pinned to the reference goldens):
    same first loss and same weights after the first update (a slice of every 8th tensor); the second loss within the
    sensitivity of the freshly initialised network."""
    from oracle import cpu_port
    from contrastiveseg_amd import kernels as K

    def emulated():
        inject.install(monkeypatch)
        # the launch-size threshold of rounds 2-4: the small convolutions of these toy encoders stay on torch on BOTH sides, as they did
        # when the bound below was set (with the round-5 default of 1 every covered layer runs through the emulator: 12 minutes instead
        # of 40 s for the two families, and 6.0e-3 instead of < 5e-3 for deeplab_v3_mem -- the split kernels have their own emulator
        # tests at every route, tests/test_emu_sb_kernels.py / test_emu_conv_stats.py, and the default routing runs in the GPU suite)
        monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 256)
        monkeypatch.setattr(K, "CONV1X1_SB_MIN_TILES", 256)
    ref_losses, ref_w = _trainer_losses(case, lambda: cpu_port.install(monkeypatch))
    monkeypatch.undo()
    losses, w = _trainer_losses(case, emulated)
    # step 1: the same arithmetic up to summation order. Step 2 sees that difference through a freshly initialised network
    # whose backward amplifies perturbations (the step goldens bound it at 5 % too)
    assert abs(losses[0] - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0])), (losses, ref_losses)
    assert abs(losses[1] - ref_losses[1]) <= 5e-2 * max(1.0, abs(ref_losses[1])), (losses, ref_losses)
    # (gradients of these freshly initialised networks differ by ~1e-2 between two fp32 evaluation orders -- the reference
    # against its own fp64 evaluation included; a wrong adjoint moves this by O(1))
    assert float((w - ref_w).norm() / ref_w.norm()) <= 5e-3


# ---- module-level dispatch of the residual-branch convolutions (module_helper.Conv3x3 / HeadConv3x3) -----------------------
@pytest.mark.parametrize("channels,hw", [(48, (8, 64)), (96, (6, 36)), (192, (5, 64)), (192, (4, 20))])
def test_conv3x3_module_routes_to_the_split_kernels(channels, hw, monkeypatch):
    """nn.Conv2d semantics of the module whatever the route: forward / backward-data on the split-bf16 kernel (192 channels
    through the explicit-tiling entry points, exactly as _hip.SIGNATURES declares them), weight gradient on the split-bf16
    kernel (48 / 96 / 192 at any width), the fp32-MFMA kernel or aten."""
    import torch.nn.functional as F
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.models.tools.module_helper import Conv3x3
    inject.install(monkeypatch)
    monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 1)
    calls = []
    for name in ("conv3x3_sb_run", "conv3x3_sb_wrw", "_conv3x3_wrw"):
        monkeypatch.setattr(K, name, (lambda fn, name: lambda *a, **k: (calls.append((name, k.get("nt", a[4] if len(a) > 4 else 0)
                                                                                      if name == "conv3x3_sb_run" else None)),
                                                                        fn(*a, **k))[1])(getattr(K, name), name))
    g = torch.Generator().manual_seed(channels)
    conv = Conv3x3(channels, channels)
    x = torch.randn(2, channels, *hw, generator=g).requires_grad_(True)
    dy = torch.randn(2, channels, *hw, generator=g)
    y = conv(x)
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    w64 = conv.weight.detach().double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, 1, 1)
    y64.backward(dy.double())
    assert float((y.detach().double() - y64.detach()).abs().max()) <= 4e-6 * float(y64.abs().max()) * max(1.0, (9 * channels) ** 0.5 / 8)
    assert [c[0] for c in calls[:2]] == ["conv3x3_sb_run", "conv3x3_sb_run"]
    if channels in K.CONV3X3_SB_PICK_NT_CHANNELS:
        assert calls[0][1] == calls[1][1] == K.conv3x3_sb_pick_nt(x, channels) and calls[0][1] in (3, 6)
    wrw_route = [c[0] for c in calls[2:]]
    if channels in K.CONV3X3_SB_WRW_CHANNELS:              # (any width since round 5: ragged row segments, f16x3)
        assert K.SPLIT_ARITH == "f16x3" and wrw_route == ["conv3x3_sb_wrw"]
    elif channels in K.CONV3X3_WRW_CHANNELS:
        assert wrw_route == ["_conv3x3_wrw"]
    else:
        assert wrw_route == []
    for got, ref in ((x.grad, x64.grad), (conv.weight.grad, w64.grad)):
        assert float((got.double() - ref).abs().max()) <= 4e-6 * float(ref.abs().max()) * max(1.0, (9 * channels) ** 0.5 / 8)


# ---- two ranks over gloo, device half = the HIP sources on the emulator ---------------------------------------------------
def _spawn(worker, n=2):
    import socket
    import torch.multiprocessing as mp
    try:
        build_emu.build()                        # before the ranks start: they must not race to build it
    except build_emu.EmuBuildError as e:
        pytest.skip(str(e))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, n, port, q)) for r in range(n)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(n)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_two_rank_syncbn_exchange_on_the_emulated_device(monkeypatch):
    """tests/test_gpu_bn.py::test_fused_syncbn_two_ranks_on_one_gpu_equal_single_process with the emulated device: two ranks with
    half the batch each == one process with the whole batch (outputs, input / residual gradients, running statistics; the
    rank-local parameter gradients add up)."""
    import numpy as np
    from tests.emu import workers
    from contrastiveseg_amd.lib.models.tools.fused_bn import FusedBatchNorm2d
    res = _spawn(workers.syncbn_worker)
    inject.install(monkeypatch)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(4, 24, 20, 36, generator=gen) * 2 + 1
    r = torch.randn(4, 24, 20, 36, generator=gen)
    g = torch.randn(4, 24, 20, 36, generator=gen)
    m = FusedBatchNorm2d(24).train()
    with torch.no_grad():
        m.weight.copy_(torch.linspace(0.5, 1.5, 24))
        m.bias.copy_(torch.linspace(-1, 1, 24))
    xd, rd = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    y = m(xd, residual=rd, relu=True)
    y.backward(g)
    assert np.abs(np.concatenate([res[0][1], res[1][1]]) - y.detach().numpy()).max() <= 1e-6
    assert np.abs(np.concatenate([res[0][2], res[1][2]]) - xd.grad.numpy()).max() <= 1e-6
    assert np.array_equal(np.concatenate([res[0][3], res[1][3]]), rd.grad.numpy())
    assert np.abs(res[0][4] + res[1][4] - m.weight.grad.numpy()).max() <= 1e-4
    assert np.abs(res[0][5] + res[1][5] - m.bias.grad.numpy()).max() <= 1e-4
    for k in (0, 1):
        assert np.abs(res[k][6] - m.running_mean.numpy()).max() <= 1e-6
        assert np.abs(res[k][7] - m.running_var.numpy()).max() <= 1e-6


def test_two_rank_cross_rank_contrast_on_the_emulated_device(monkeypatch):
    """tests/test_distributed_gloo.py's oracle (the single-process loss on the concatenated global batch) against two ranks
    whose device half is the HIP sources: same loss, local gradient / world == the single-process gradient slice."""
    import numpy as np
    from tests.emu import workers
    sys.path.insert(0, HERE)
    from test_distributed_gloo import _case, _configer
    res = _spawn(workers.cross_rank_worker)
    inject.install(monkeypatch)
    from contrastiveseg_amd.lib.loss.loss_contrast import PixelContrastLoss
    c, (target, seg, embed, _) = _case()
    crit = PixelContrastLoss(_configer(c, "global", 256))
    e = torch.from_numpy(embed).requires_grad_(True)
    torch.manual_seed(11)
    want = crit(e, torch.from_numpy(target), seg=torch.from_numpy(seg))
    want.backward()
    B = c["B"] // 2
    for rank, loss, grad, n in res:
        assert n == crit.last_selection["plan"].N
        assert abs(loss - float(want.detach())) < 1e-5 * max(1.0, abs(float(want.detach())))
        ref = e.grad.numpy()[rank * B:(rank + 1) * B]
        assert np.allclose(grad / 2, ref, rtol=1e-4, atol=1e-8), np.abs(grad / 2 - ref).max()


# ---- BASELINE.json's headline contrast shape and the reference config's bank size, on the emulator ------------------------
@pytest.mark.slow
def test_contrast_at_the_headline_and_reference_bank_sizes(monkeypatch):
    """1024 anchors x 4104 bank columns x 256-d (BASELINE.json), and the reference's own memory configuration (152 anchors x
    190 000 columns): bank mode read in place == plain mode on the packed copy == the float64 oracle, gradients included."""
    _replay(monkeypatch, "test_gpu_kernels", "test_contrast_headline_shape_properties", {})
    _replay(monkeypatch, "test_gpu_kernels", "test_contrast_bank_reference_config_size", {})


def test_single_rank_process_group_takes_the_multi_rank_paths():
    """tools/rccl_single_rank_check.py on gloo with the emulated device half: with CSEG_DIST_SINGLE_RANK=1 a process group of
    one rank goes through the SyncBN exchange and the cross-rank contrast set (collectives counted) and reproduces the local
    paths. On the GPU box the same script runs on RCCL (tests/test_zz_gpu_default_routes.py)."""
    import json
    import subprocess
    try:
        build_emu.build()
    except build_emu.EmuBuildError as e:
        pytest.skip(str(e))
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "rccl_single_rank_check.py"), "--backend", "gloo", "--emu"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["ok"] and d["syncbn_all_reduces"] == 2 and d["cross_rank_collectives"] >= 2


# ---- round 3: the whole network's weights packed in one launch (kernels.SplitWeights -> cseg_amax_batch / cseg_split_pack_batch) --
@pytest.mark.parametrize("arith", ["f16x3", "bf16x6"])
def test_batched_weight_packs_equal_the_per_layer_packs(arith, monkeypatch):
    """Same bytes as cseg_conv3x3_split_pack / cseg_conv1x1_split_pack layer by layer (all three packed formats, forward and
    backward-data operators), refreshed together after an in-place update of the weights, dropped with the weight."""
    import ctypes
    import gc
    from contrastiveseg_amd import _hip
    from contrastiveseg_amd import kernels as K
    inject.install(monkeypatch)
    monkeypatch.setattr(K, "SPLIT_ARITH", arith)
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    aid = K.split_arith_id()
    g = torch.Generator().manual_seed(3)
    ws = {"c3_main_96": torch.randn(96, 96, 3, 3, generator=g) * 0.05, "c3_sb16_48": torch.randn(48, 48, 3, 3, generator=g) * 3.0,
          "c3_sb16_64": torch.randn(64, 64, 3, 3, generator=g) * 1e-3, "c3_192_nt3": torch.randn(192, 48, 3, 3, generator=g),
          "c1_64_256": torch.randn(256, 64, 1, 1, generator=g) * 0.2, "c1_144_48": torch.randn(48, 144, 1, 1, generator=g)}
    reqs = [("c3_main_96", "c3", False, 0), ("c3_main_96", "c3", True, 0), ("c3_sb16_48", "c3", False, 0), ("c3_sb16_48", "c3", True, 0),
            ("c3_sb16_64", "c3", False, 0), ("c3_192_nt3", "c3", False, 3), ("c1_64_256", "c1", False, 0), ("c1_64_256", "c1", True, 0),
            ("c1_144_48", "c1", False, 0)]

    def single(w, tag, flag, nt):
        co, ci = w.shape[:2]
        conv_in, conv_out = (co, ci) if flag else (ci, co)
        lib = _hip.lib()
        aw = K.tensor_amax(w.contiguous()) if aid else None
        ap = ctypes.c_void_p(aw.data_ptr()) if aid else ctypes.c_void_p(None)
        if tag == "c3":
            wp = torch.full((lib.cseg_conv3x3_split_packed_bytes(aid, conv_in, conv_out),), 0xEE, dtype=torch.uint8)
            _hip.call("cseg_conv3x3_split_pack", ctypes.c_void_p(w.data_ptr()), co, ci, int(flag), nt, aid, ap, wp.data_ptr(), None)
        else:
            wp = torch.full((lib.cseg_conv1x1_split_packed_bytes(aid, conv_in, conv_out),), 0xEE, dtype=torch.uint8)
            _hip.call("cseg_conv1x1_split_pack", ctypes.c_void_p(w.data_ptr()), co, ci, int(flag), aid, ap, wp.data_ptr(), None)
        return wp, aw

    def check():
        for name, tag, flag, nt in reqs:
            wp, aw = K.SPLIT_WEIGHTS.get(ws[name], tag, flag, nt)
            ref, ref_aw = single(ws[name], tag, flag, nt)
            # (the buffer has room for either 3x3 packed format -- the 16-channel-chunk one of the grouped launches is larger; a pack
            # writes `total` groups of NP cells of 16 bytes)
            st = K.SPLIT_WEIGHTS.weights[id(ws[name])]
            used = next(e["total"] for e in st["entries"].values() if e["wp"] is wp) * (2 if aid else 3) * 16
            assert wp.shape == ref.shape and used <= wp.numel() and torch.equal(wp[:used], ref[:used]), (name, tag, flag)
            assert bool((ref[used:] == 0xEE).all()), "the per-layer pack wrote beyond the plan's size"
            if aid:
                assert int(aw.view(32, 32)[:, 0].max()) == int(ref_aw.view(32, 32)[:, 0].max()) == \
                    int(ws[name].abs().max().view(torch.int32))
    check()                                             # registration: every request packs on first use
    launches = []
    orig = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (launches.append(name), orig(name, *a))[1])
    for w in ws.values():
        w.mul_(1.7).add_(0.01)                          # what an optimizer step does: in place, version bumped
    K.SPLIT_WEIGHTS.get(ws["c1_144_48"], "c1", False, 0)          # the first request of the next step refreshes everything
    assert launches == (["cseg_amax_batch", "cseg_split_pack_batch"] if aid else ["cseg_split_pack_batch"]), launches
    launches.clear()
    monkeypatch.setattr(_hip, "call", orig)
    check()
    n = len(K.SPLIT_WEIGHTS.weights)
    del ws["c3_192_nt3"]
    gc.collect()
    assert len(K.SPLIT_WEIGHTS.weights) == n - 1
    reqs = [r for r in reqs if r[0] != "c3_192_nt3"]
    ws["c1_144_48"].mul_(0.5)
    check()                                             # one stale weight among fresh ones


@pytest.mark.parametrize("how", ["fused_sgd", "foreach_sgd", "param_data", "raw_pointer"])
def test_packed_weights_follow_updates_that_skip_the_version_counter(how, monkeypatch):
    """torch._fused_sgd_ updates parameters WITHOUT bumping Tensor._version, and so does every write through
    `param.data` or a raw pointer; SplitWeights used to key staleness on (data_ptr, _version) alone, so the step-0 packs stayed in
    use for the whole run. Now every optimizer step (global post-hook) and an explicit invalidate() advance an epoch. Three steps;
    after each the split kernel's output must equal the convolution with the CURRENT weights."""
    from contrastiveseg_amd import kernels as K
    from contrastiveseg_amd.lib.models.tools.module_helper import Conv3x3
    inject.install(monkeypatch)
    monkeypatch.setattr(K, "SPLIT_ARITH", "f16x3")
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 1)
    torch.manual_seed(11)
    conv = Conv3x3(48, 48)
    x = torch.randn(1, 48, 4, 64)
    opt = None
    if how.endswith("_sgd"):
        try:
            opt = torch.optim.SGD(conv.parameters(), lr=0.5, momentum=0.9, **({"fused": True} if how == "fused_sgd" else {"foreach": True}))
        except (RuntimeError, TypeError) as e:
            pytest.skip("this torch build has no fused SGD on the CPU: %s" % e)
    for step in range(3):
        y = conv(x)
        ref = torch.nn.functional.conv2d(x.double(), conv.weight.detach().double(), None, 1, 1)
        err = float((y.detach().double() - ref).abs().max()) / float(ref.abs().max())
        assert err <= 3e-5, (how, step, err)          # a stale pack is off by the size of the update: O(1)
        v0 = conv.weight._version
        if opt is not None:
            opt.zero_grad()
            y.square().mean().backward()
            conv.weight.grad.add_(0.3)                # a visible update whatever the loss gradient is
            opt.step()
            if how == "fused_sgd" and conv.weight._version != v0:
                pass                                   # (a torch that bumps the version: the epoch is then redundant, not wrong)
        elif how == "param_data":
            conv.weight.data.mul_(1.5).add_(0.02)
            K.SPLIT_WEIGHTS.invalidate()
        else:
            import ctypes
            n = conv.weight.numel()
            buf = (ctypes.c_float * n).from_address(conv.weight.data_ptr())
            for i in range(0, n, 7):
                buf[i] = buf[i] * -2.0 + 0.05
            assert conv.weight._version == v0
            K.SPLIT_WEIGHTS.invalidate()


def test_batched_weight_packs_survive_recycled_layers(monkeypatch):
    """Layers that come and go (every test builds its own): a new weight that lands on a dead weight's Python id AND storage gets a
    fresh max|w| row, so the cached job table of the dead one must not be reused (it was, in the first hardware run: NaN outputs
    from a scale derived from a zero record)."""
    import gc
    from contrastiveseg_amd import kernels as K
    inject.install(monkeypatch)
    monkeypatch.setattr(K, "SPLIT_ARITH", "f16x3")
    monkeypatch.setattr(K, "SPLIT_WEIGHTS", K.SplitWeights())
    monkeypatch.setattr(K, "CONV3X3_SB_MIN_TILES", 1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 48, 4, 64, generator=g)
    seen = set()
    for trial in range(12):
        w = torch.randn(48, 48, 3, 3, generator=g) * (10.0 ** (trial % 6 - 3))   # very different magnitudes: a stale scale shows
        y = K.conv3x3_sb_run(x, w, False)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
        assert torch.isfinite(y).all()
        assert float((y.double() - ref).abs().max()) <= 3e-5 * float(ref.abs().max())
        seen.add((id(w), w.data_ptr()))
        # what the cached job tables are keyed on names pointers and record rows by value
        ident = K.SPLIT_WEIGHTS.table_cache[(("cpu", None), "amax")][0]
        assert ident == tuple((v.data_ptr(), v.numel(), st["row"]) for st in K.SPLIT_WEIGHTS.weights.values() for v in [st["ref"]()])
        del w, y
        gc.collect()
    # (whether an (id, storage) pair really recurs is up to CPython and the allocator: on the GPU box it did)
