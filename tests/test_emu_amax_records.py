"""tests/test_gpu_amax_records.py replayed with the device being the CPU emulation of the execution model (tests/emu): the same test
bodies run the HIP sources of csrc/bn.hip, csrc/fuse.hip (cseg_affine_channels) and the split-operand convolutions through
contrastiveseg_amd/kernels.py -- every producer's max|.| record against the tensor it stored, the consumers with the producer's record
against a fresh pass, forwarded records, the version guard, the arena switch and the projection head's merged record -- once in
ascending and once in descending wave order: a record must not depend on which block publishes first. (The hipGraph test needs the
GPU.)"""
import os

import pytest

from tests.emu import build_emu
from tests.test_emu_cabi import _cases, _ids, _replay

pytestmark = pytest.mark.skipif(not os.path.exists(build_emu.CLANG), reason="host clang++ of the ROCm toolchain not found")
MOD = "test_gpu_amax_records"
ORDERS = ["asc", "desc"]

FWD_TRAIN = _cases(MOD, "test_training_forward_leaves_the_record_of_the_stored_output")
FWD_FROZEN = _cases(MOD, "test_frozen_forward_leaves_the_record_of_the_stored_output")
BWD = _cases(MOD, "test_backward_leaves_the_record_of_the_stored_input_gradient")
BWD_SYNC = _cases(MOD, "test_sync_backward_leaves_the_record_of_the_stored_input_gradient")
MODULE = _cases(MOD, "test_module_attaches_the_records_of_output_and_input_gradient")
AFFINE = _cases(MOD, "test_affine_channels_leaves_the_record_of_the_stored_output")
GROUP_FWD = _cases(MOD, "test_grouped_forward_leaves_every_members_record")
GROUP_BWD = _cases(MOD, "test_grouped_backward_leaves_every_members_record")
CONSUMERS = _cases(MOD, "test_consumers_give_the_same_bits_with_the_producers_record")


def _run(monkeypatch, order, func, kw, mp=False):
    monkeypatch.setenv("CSEG_EMU_WAVE_ORDER", order)
    _replay(monkeypatch, MOD, func, dict(kw, monkeypatch=monkeypatch) if mp else kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", FWD_TRAIN, ids=_ids(FWD_TRAIN))
def test_training_forward_leaves_the_record_of_the_stored_output(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_training_forward_leaves_the_record_of_the_stored_output", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", FWD_FROZEN, ids=_ids(FWD_FROZEN))
def test_frozen_forward_leaves_the_record_of_the_stored_output(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_frozen_forward_leaves_the_record_of_the_stored_output", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", BWD, ids=_ids(BWD))
def test_backward_leaves_the_record_of_the_stored_input_gradient(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_backward_leaves_the_record_of_the_stored_input_gradient", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", BWD_SYNC, ids=_ids(BWD_SYNC))
def test_sync_backward_leaves_the_record_of_the_stored_input_gradient(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_sync_backward_leaves_the_record_of_the_stored_input_gradient", kw)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", MODULE, ids=_ids(MODULE))
def test_module_attaches_the_records_of_output_and_input_gradient(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_module_attaches_the_records_of_output_and_input_gradient", kw, mp=True)


@pytest.mark.parametrize("order", ORDERS)
def test_degenerate_operands_leave_all_zero_records(order, monkeypatch):
    _run(monkeypatch, order, "test_degenerate_operands_leave_all_zero_records", {}, mp=True)


@pytest.mark.parametrize("order", ORDERS)
def test_no_record_under_bf16x6(order, monkeypatch):
    _run(monkeypatch, order, "test_no_record_under_bf16x6", {}, mp=True)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", AFFINE, ids=_ids(AFFINE))
def test_affine_channels_leaves_the_record_of_the_stored_output(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_affine_channels_leaves_the_record_of_the_stored_output", kw)


def test_affine_channels_refuses_planes_that_are_no_multiple_of_four(monkeypatch):
    _run(monkeypatch, "asc", "test_affine_channels_refuses_planes_that_are_no_multiple_of_four", {})


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", GROUP_FWD, ids=_ids(GROUP_FWD))
def test_grouped_forward_leaves_every_members_record(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_grouped_forward_leaves_every_members_record", kw, mp=True)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", GROUP_BWD, ids=_ids(GROUP_BWD))
def test_grouped_backward_leaves_every_members_record(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_grouped_backward_leaves_every_members_record", kw, mp=True)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kw", CONSUMERS, ids=_ids(CONSUMERS))
def test_consumers_give_the_same_bits_with_the_producers_record(kw, order, monkeypatch):
    _run(monkeypatch, order, "test_consumers_give_the_same_bits_with_the_producers_record", kw, mp=True)


@pytest.mark.parametrize("order", ORDERS)
def test_forwarded_records(order, monkeypatch):
    _run(monkeypatch, order, "test_forwarded_records", {}, mp=True)


@pytest.mark.parametrize("order", ORDERS)
def test_an_in_place_edit_drops_the_record(order, monkeypatch):
    _run(monkeypatch, order, "test_an_in_place_edit_drops_the_record", {}, mp=True)


@pytest.mark.parametrize("order", ORDERS)
def test_records_across_an_arena_switch(order, monkeypatch):
    _run(monkeypatch, order, "test_records_across_an_arena_switch", {}, mp=True)


@pytest.mark.parametrize("order", ORDERS)
def test_projection_head_record_of_the_row_sparse_input_gradient(order, monkeypatch):
    _run(monkeypatch, order, "test_projection_head_record_of_the_row_sparse_input_gradient", {}, mp=True)
