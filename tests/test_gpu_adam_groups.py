"""Parameter groups of the fused Adam on a real MI355X: rd_adam_step_groups through the C ABI (including a group boundary in the second
grid-stride sweep), FlatAdam built from torch's list of group dictionaries, and one RC-Net fine-tuning step pair, eager and graphed."""
import pytest

from tests import parity_cases_adam_groups as A
from tests import parity_cases_glue as G

pytestmark = pytest.mark.gpu


def test_kernel_groups(gpu):
    A.kernel_multi_case(gpu)
    A.kernel_eight_case(gpu)
    G.report()


def test_kernel_refusals(gpu):
    A.kernel_refusal_case(gpu)


def test_kernel_inactive_group(gpu):
    A.kernel_inactive_case(gpu)


def test_kernel_skip_flag(gpu):
    A.kernel_skip_flag_case(gpu)


def test_kernel_ties_to_adam_step(gpu):
    A.kernel_ties_to_adam_step_case(gpu)


def test_kernel_second_sweep(gpu):
    A.kernel_large_case(gpu)
    G.report()


def test_flat_adam_groups(gpu):
    A.flat_adam_groups_case(gpu)
    A.flat_adam_idle_group_case(gpu)
    G.report()


def test_flat_adamw(gpu):
    A.flat_adamw_case(gpu)


def test_reference_literal_form(gpu):
    A.reference_literal_case(gpu)


def test_state_exchange(gpu):
    A.state_exchange_case(gpu)


def test_bucketing(gpu):
    A.bucketing_case(gpu)


def test_finetune_step_pair_eager_and_graphed(gpu):
    A.finetune_case(gpu)
    G.report()
