"""Whole-module logic checks under the fiber emulator (see tests/test_emu_ops.py for what these are and are not)."""
import pytest

from tests import parity_cases as P

# the longest cases of the CPU suite (minutes under the emulator); they run by default, `-m "not slow"` leaves them out
pytestmark = pytest.mark.slow


def test_decoder_small_golden(emu):
    P.decoder_case(emu, "small")


def test_rcnet_end_to_end_golden(emu):
    P.rcnet_e2e_case(emu)
