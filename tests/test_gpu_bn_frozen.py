"""rd_bn_act_bwd_frozen on a real MI355X (HIP kernels through the C ABI) against float64 torch autograd through F.batch_norm(training=False):
the cross products of tests/parity_cases_bn_frozen.py and, per form, a size that reaches a second grid-stride iteration."""
import pytest

from tests import parity_cases_bn as B
from tests import parity_cases_bn_frozen as Z

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in B.DTYPES]


@pytest.mark.parametrize("act", B.ACTS)
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_frozen(gpu, dtype, form, act):
    Z.backward_case(gpu, dtypes=(dtype,), forms=(form,), acts=(act,))
    B.report_bn()


@pytest.mark.parametrize("dtype", DTYPES)
def test_thresholds_frozen(gpu, dtype):
    Z.thresholds_case(gpu, dtypes=(dtype,))
    B.report_bn()
