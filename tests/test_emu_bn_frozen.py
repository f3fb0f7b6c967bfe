"""rd_bn_act_bwd_frozen under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): the covering selection of the
cross products the GPU twin runs in full (tests/parity_cases_bn_frozen.py, parity_cases_bn `_cover` / QUICK_WIDE)."""
from tests import parity_cases_bn as B
from tests import parity_cases_bn_frozen as Z


def test_backward_frozen(emu):
    Z.backward_case(emu, quick=True)
    B.report_bn()


def test_thresholds_frozen(emu):
    Z.thresholds_case(emu, quick=True)
    B.report_bn()
