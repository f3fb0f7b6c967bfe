"""Scale-Map-Learner batch augmentation: the host-side draw order (no kernel library), and the two kernels under the fiber emulator (see
tests/test_emu_ops.py for what these are and are not) -- the cases of tests/parity_cases_sml_aug.py, which the GPU twin runs on the device."""
from tests import parity_cases_sml_aug as A


def test_draw_order_fixture(tmp_path):
    A.draw_order_fixture_case(tmp_path)


def test_draw_order_crop(tmp_path):
    A.draw_order_crop_case(tmp_path)


def test_fixture_parity(emu, tmp_path):
    A.fixture_parity_case(emu, tmp_path)


def test_geometry_kernel(emu):
    A.geometry_case(emu)


def test_host_count_equals_device_mask(emu):
    A.count_case(emu)


def test_noise_kernel(emu):
    A.noise_case(emu)


def test_static_batch(emu):
    A.static_batch_case(emu)
