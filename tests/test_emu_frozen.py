"""Frozen BatchNorm at the engine and module level under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): the cases
of tests/parity_cases_frozen.py the GPU twin runs, except the captured-region one, which needs a GPU."""
import pytest

from tests import parity_cases_frozen as Z


@pytest.mark.parametrize("i", range(len(Z.CONV_CASES)))
def test_conv2d_frozen(emu, i):
    Z.conv_case(emu, Z.CONV_CASES[i])


def test_resnet_block_idiom_and_mark(emu):
    Z.resnet_block_case(emu)


def test_affine_false(emu):
    Z.affine_false_case(emu)
    Z.refuses_untracked_case(emu)


def test_decoder_block_frozen(emu):
    Z.decoder_block_case(emu)


@pytest.mark.parametrize("kind,k", [("ir", 3), ("ir", 5), ("ds", 3), ("ds", 5)])
def test_depthwise_blocks_frozen(emu, kind, k):
    Z.effnet_block_case(emu, kind, k)


@pytest.mark.slow      # (a whole RC-Net step forward and backward: minutes under the emulator, as test_emu_networks)
def test_mixed_mode_rcnet(emu):
    Z.mixed_mode_case(emu)


def test_lazy_on_off_and_head(emu):
    Z.lazy_case(emu)
