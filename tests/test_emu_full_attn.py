"""Softmax ('full') attention and the token masks under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): the
covering selection of tests/parity_cases_full_attn.py; the GPU twin runs the cross products."""
import pytest

from tests import parity_cases_full_attn as A


@pytest.mark.parametrize("op", A.OPS)
def test_attention(emu, op):
    A.attention_case(emu, op, quick=True)
    A.report()


def test_attention_edges(emu):
    A.edges_case(emu, quick=True)
    A.report()


def test_attention_refusals(emu):
    A.refusals_case(emu, quick=True)


def test_state_dict_keys():
    A.state_dict_case()


def test_default_route_unchanged(emu):
    A.default_route_case(emu, quick=True)


@pytest.mark.slow      # (whole layers through the per-op route, forward and backward)
def test_layer_full(emu):
    A.layer_case(emu, quick=True)
    A.report()


@pytest.mark.slow
@pytest.mark.parametrize("attention", ["full", "linear"])
def test_transformer_with_masks(emu, attention):
    A.transformer_case(emu, attention, quick=True)
    A.report()
