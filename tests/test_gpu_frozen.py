"""Frozen BatchNorm at the engine and module level on a real MI355X (tests/parity_cases_frozen.py): backward through running statistics layer by
layer against the oracle with training=False, the bn.eval() idiom, the sticky mark, mixed mode, and the captured-region key."""
import pytest

from tests import parity_cases_frozen as Z

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(Z.CONV_CASES)))
def test_conv2d_frozen(gpu, i):
    Z.conv_case(gpu, Z.CONV_CASES[i])


def test_resnet_block_idiom_and_mark(gpu):
    Z.resnet_block_case(gpu)


def test_affine_false(gpu):
    Z.affine_false_case(gpu)
    Z.refuses_untracked_case(gpu)


def test_decoder_block_frozen(gpu):
    Z.decoder_block_case(gpu)


@pytest.mark.parametrize("kind,k", [("ir", 3), ("ir", 5), ("ds", 3), ("ds", 5)])
def test_depthwise_blocks_frozen(gpu, kind, k):
    Z.effnet_block_case(gpu, kind, k)


def test_mixed_mode_rcnet(gpu):
    Z.mixed_mode_case(gpu)


def test_lazy_on_off_and_head(gpu):
    Z.lazy_case(gpu)


def test_autograph_recaptures_after_freeze(gpu):
    Z.autograph_case(gpu)
