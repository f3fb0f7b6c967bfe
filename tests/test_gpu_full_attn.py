"""Softmax ('full') attention and the token masks on a real MI355X (HIP kernels through the C ABI, and the modules that route to them) against
float64 torch: the cross products of tests/parity_cases_full_attn.py."""
import pytest

from tests import parity_cases_full_attn as A

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in A.DTYPES]


@pytest.mark.parametrize("sweep", A.SWEEPS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", A.OPS)
def test_attention(gpu, op, dtype, sweep):
    A.attention_case(gpu, op, dtypes=(dtype,), sweeps=(sweep,))
    A.report()


def test_attention_edges(gpu):
    A.edges_case(gpu)
    A.report()


def test_attention_refusals(gpu):
    A.refusals_case(gpu)


def test_state_dict_keys(gpu):
    A.state_dict_case()


def test_default_route_unchanged(gpu):
    A.default_route_case(gpu)


def test_layer_full(gpu):
    A.layer_case(gpu)
    A.report()


@pytest.mark.parametrize("attention", ["full", "linear"])
def test_transformer_with_masks(gpu, attention):
    A.transformer_case(gpu, attention)
    A.report()
