"""Unsupervised SML loss term and the masked on-device median on a real MI355X (HIP kernels through the C ABI) vs torch.median, the reference's
fixtures and the torch restatement; the term inside a captured step.  Every case runs once."""
import pytest

from tests import parity_cases_unsup as U

pytestmark = pytest.mark.gpu


def test_masked_median_bit_exact(gpu):
    U.selection_case(gpu)


def test_unsup_loss_reference_fixtures(gpu):
    U.fixture_case(gpu)


def test_unsup_loss_larger_maps_ties_and_zero_weight(gpu):
    U.larger_maps_case(gpu)


def test_unsup_graphed_step_matches_eager(gpu):
    U.graphed_step_case(gpu)


def test_unsup_autograph_matches_eager(gpu):
    U.autograph_case(gpu)


def test_unsup_step_is_reproducible(gpu):
    U.reproducible_case(gpu)


def test_unsup_backward_after_the_mask_was_dropped(gpu):
    U.dropped_mask_case(gpu)


def test_unsup_forward_loss_against_restatement(gpu):
    U.forward_loss_case(gpu)                       # resized maps (48 x 64 -> 288 x 384): the mask source is a fresh tensor inside forward_loss
    U.forward_loss_case(gpu, net_hw=(48, 64))
