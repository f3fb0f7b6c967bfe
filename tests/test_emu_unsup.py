"""Unsupervised SML loss term and the masked on-device median under the fiber emulator (see tests/test_emu_ops.py for what these are and are
not): the same kernel sources, compiled for the host."""
from tests import parity_cases_unsup as U


def test_masked_median_bit_exact(emu):
    U.selection_case(emu)


def test_unsup_loss_reference_fixtures(emu):
    U.fixture_case(emu)


def test_unsup_loss_larger_maps_ties_and_zero_weight(emu):
    U.larger_maps_case(emu)


def test_unsup_backward_after_the_mask_was_dropped(emu):
    U.dropped_mask_case(emu)


def test_unsup_forward_loss_against_restatement(emu):
    U.forward_loss_case(emu, net_hw=(48, 64))
