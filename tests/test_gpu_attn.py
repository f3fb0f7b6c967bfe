"""The linear-attention and fused LoFTR-layer kernels one by one on a real MI355X (HIP kernels through the C ABI) against float64 torch: the
cross products of tests/parity_cases_attn.py."""
import pytest

from tests import parity_cases_attn as A

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in A.DTYPES]


@pytest.mark.parametrize("sweep", A.SWEEPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention(gpu, dtype, sweep):
    A.attention_case(gpu, dtypes=(dtype,), sweeps=(sweep,))
    A.report_attn()


def test_attention_edges(gpu):
    A.attention_edges_case(gpu)
    A.report_attn()


def test_attention_refusals(gpu):
    A.attention_refusals_case(gpu)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_layer(gpu, dtype, kind):
    A.fused_case(gpu, dtypes=(dtype,), kinds=(kind,))
    A.report_attn()


def test_fused_layer_refusals(gpu):
    A.fused_refusals_case(gpu)


@pytest.mark.parametrize("route", A.ROUTES[1:])
def test_transformer_routes(gpu, route):
    A.routes_case(gpu, routes=("default", route))
    A.report_attn()


def test_transformer_too_long(gpu):
    A.too_long_case(gpu)
