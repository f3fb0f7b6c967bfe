"""The depthwise, bilinear and SML-head kernels one by one on a real MI355X (HIP kernels through the C ABI) against float64 torch: the cross
products of tests/parity_cases_dw.py and one size past each launcher clamp."""
import pytest

from tests import parity_cases_dw as D

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in D.DTYPES]
HEAD_DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in D.HEAD_DTYPES]


@pytest.mark.parametrize("cls", D.CLASSES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_depthwise(gpu, dtype, cls):
    D.dw_case(gpu, dtypes=(dtype,), classes=(cls,))
    D.report_dw()


def test_depthwise_fp16(gpu):
    D.dw_fp16_case(gpu)
    D.report_dw()


def test_depthwise_misaligned_weights_and_accumulate(gpu):
    D.dw_variants_case(gpu)
    D.report_dw()


def test_wgrad_batch(gpu):
    D.wgrad_batch_case(gpu)
    D.report_dw()


@pytest.mark.parametrize("form", D.BIL_FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear(gpu, dtype, form):
    D.bilinear_case(gpu, dtypes=(dtype,), forms=(form,))
    D.report_dw()


def test_bilinear_fp16(gpu):
    D.bilinear_fp16_case(gpu)
    D.report_dw()


@pytest.mark.parametrize("dtype", HEAD_DTYPES)
def test_sml_head(gpu, dtype):
    D.head_case(gpu, dtypes=(dtype,))
    D.report_dw()


def test_reciprocal(gpu):
    D.reciprocal_case(gpu)
    D.report_dw()


def test_refusals(gpu):
    D.refusals_case(gpu)
