"""The Scale-Map-Learner options 'midas-small-depth' and ground-truth dilation under the fiber emulator (see tests/test_emu_ops.py for what these
are and are not): the three kernels of rd_sml_depth.hip one by one, their refusals, and MidasNet_small_depth against the reference's outputs."""
import pytest

from tests import parity_cases_sml_depth as D


def test_depth_head(emu):
    D.head_case(emu)


def test_dilate(emu):
    D.dilate_case(emu)


def test_refusals(emu):
    D.refusals_case(emu)


@pytest.mark.slow      # (a whole SML forward at 2 x 64 x 96: minutes under the emulator; the backward, the eval-mode forward and in_channels = 2 run on the GPU twin)
def test_depth_net(emu):
    D.sml_depth_net_case(emu, 3, forward_only=True)
