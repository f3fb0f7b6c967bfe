"""RC-Net inference over frame batches (rd_infer.hip, rcnet_main.fuse_frames / run_frames) under the fiber emulator (see tests/test_emu_ops.py for
what these are and are not) -- the cases of tests/parity_cases_infer.py, which the GPU twin runs on the device."""
import pytest

from tests import parity_cases_infer as I


def test_scatter_frames_equals_scatter_crops(emu):
    I.scatter_frames_exact_case(emu)


def test_scatter_frames_reference_fixture(emu):
    I.scatter_frames_reference_case(emu)


def test_frame_thresholds(emu):
    I.thresholds_case(emu)


def test_entry_refusals(emu):
    I.entry_refusals_case(emu)


@pytest.mark.slow      # (a whole RC-Net forward over three frames: the emulator runs every launch block by block)
def test_run_frames(emu):
    I.run_frames_case(emu)
