"""The Scale-Map-Learner options 'midas-small-depth' and ground-truth dilation on a real MI355X: the three kernels of rd_sml_depth.hip through
the C ABI, MidasNet_small_depth against the reference's outputs, and the training / validation step with the two new configuration keys."""
import pytest

from tests import parity_cases_sml_depth as D

pytestmark = pytest.mark.gpu

HEAD_DTYPES = [pytest.param(d, id=str(d).split(".")[-1]) for d in D.HEAD_DTYPES]


@pytest.mark.parametrize("dtype", HEAD_DTYPES)
def test_depth_head(gpu, dtype):
    D.head_case(gpu, dtypes=(dtype,))


def test_dilate(gpu):
    D.dilate_case(gpu)


def test_refusals(gpu):
    D.refusals_case(gpu)


@pytest.mark.parametrize("in_channels", [3, 2])
def test_depth_net(gpu, in_channels):
    D.sml_depth_net_case(gpu, in_channels)


def test_train_step(gpu):
    D.train_step_case(gpu)


def test_graphed_step(gpu):
    D.graphed_step_case(gpu)


def test_validate_batch(gpu):
    D.validate_case(gpu)


def test_default_launches(gpu):
    D.default_launches_case(gpu)
