"""The BatchNorm kernel family one by one on a real MI355X (HIP kernels through the C ABI) against float64 torch restatements: the cross products
of tests/parity_cases_bn.py and, per form, the sizes that reach a second grid-stride iteration."""
import pytest

from tests import parity_cases_bn as B

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in B.DTYPES]


def test_statistics_producers(gpu):
    B.stats_case(gpu)
    B.report_bn()


def test_finalize(gpu):
    B.finalize_case(gpu)
    B.report_bn()


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_affine_act(gpu, dtype, form):
    B.affine_case(gpu, dtypes=(dtype,), forms=(form,))
    B.report_bn()


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward(gpu, dtype, form, act):
    B.backward_case(gpu, dtypes=(dtype,), forms=(form,), acts=(act,))
    B.report_bn()


@pytest.mark.parametrize("dtype", DTYPES)
def test_thresholds(gpu, dtype):
    B.thresholds_case(gpu, dtypes=(dtype,))
    B.report_bn()


def test_phases(gpu):
    B.phases_case(gpu)
    B.report_bn()


def test_conditioning(gpu):
    B.conditioning_case(gpu)
    B.report_bn()
