"""Scale-Map-Learner batch augmentation on a real MI355X (HIP kernels through the C ABI and through riders_amd.utv_dataset): the cases of
tests/parity_cases_sml_aug.py, and a captured training step fed through augment(..., out=step.static_batch)."""
import pytest

from tests import parity_cases_sml_aug as A

pytestmark = pytest.mark.gpu


def test_fixture_parity(gpu, tmp_path):
    A.fixture_parity_case(gpu, tmp_path)


def test_geometry_kernel(gpu):
    A.geometry_case(gpu)


def test_host_count_equals_device_mask(gpu):
    A.count_case(gpu)


def test_noise_kernel(gpu):
    A.noise_case(gpu)


def test_static_batch(gpu):
    A.static_batch_case(gpu)


def test_static_batch_feeds_graphed_step(gpu):
    A.graphed_step_case(gpu)
