"""The linear-attention and fused LoFTR-layer kernels one by one under the fiber emulator (see tests/test_emu_ops.py for what these are and are
not): the covering selection of tests/parity_cases_attn.py; the GPU twin runs the cross products."""
import pytest

from tests import parity_cases_attn as A


def test_attention(emu):
    A.attention_case(emu, quick=True)
    A.report_attn()


def test_attention_edges(emu):
    A.attention_edges_case(emu, quick=True)
    A.report_attn()


def test_attention_refusals(emu):
    A.attention_refusals_case(emu, quick=True)


def test_fused_layer(emu):
    A.fused_case(emu, quick=True)
    A.report_attn()


def test_fused_layer_refusals(emu):
    A.fused_refusals_case(emu, quick=True)


@pytest.mark.slow      # (whole transformer passes, forward and backward: half a minute each under the emulator)
@pytest.mark.parametrize("route", A.ROUTES)
def test_transformer_routes(emu, route):
    A.routes_case(emu, quick=True, routes=(route,))
    A.report_attn()


def test_transformer_too_long(emu):
    A.too_long_case(emu, quick=True)
