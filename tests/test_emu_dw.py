"""The depthwise, bilinear and SML-head kernels one by one under the fiber emulator (see tests/test_emu_ops.py for what these are and are
not): the covering selection of tests/parity_cases_dw.py; the GPU twin runs the cross products and the sizes past the launcher clamps."""
from tests import parity_cases_dw as D


def test_depthwise(emu):
    D.dw_case(emu, quick=True)
    D.report_dw()


def test_depthwise_fp16(emu):
    D.dw_fp16_case(emu, quick=True)
    D.report_dw()


def test_depthwise_misaligned_weights_and_accumulate(emu):
    D.dw_variants_case(emu, quick=True)
    D.report_dw()


def test_wgrad_batch(emu):
    D.wgrad_batch_case(emu, quick=True)
    D.report_dw()


def test_bilinear(emu):
    D.bilinear_case(emu, quick=True)
    D.bilinear_fp16_case(emu, quick=True)
    D.report_dw()


def test_sml_head(emu):
    D.head_case(emu, quick=True)
    D.report_dw()


def test_reciprocal(emu):
    D.reciprocal_case(emu, quick=True)
    D.report_dw()


def test_refusals(emu):
    D.refusals_case(emu, quick=True)
