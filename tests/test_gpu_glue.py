"""Layout, LayerNorm, loss and Adam kernels one by one on a real MI355X (HIP kernels through the C ABI) against float64 torch restatements,
including the sizes that reach a second grid-stride iteration."""
import pytest

from tests import parity_cases_glue as G

pytestmark = pytest.mark.gpu


def test_add(gpu):
    G.add_case(gpu)


def test_cast(gpu):
    G.cast_case(gpu)


def test_layouts(gpu):
    G.layout_case(gpu)


def test_upsample_nearest(gpu):
    G.upsample_case(gpu)


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_layernorm(gpu, C):
    G.layernorm_case(gpu, Cs=(C,), extras=C == 128)
    G.report()


def test_colsum(gpu):
    G.colsum_case(gpu)
    G.report()


def test_act_bwd(gpu):
    G.act_bwd_case(gpu)


def test_bce_and_sigmoid(gpu):
    G.bce_case(gpu)
    G.report()


def test_adam(gpu):
    G.adam_case(gpu)
    G.report()
