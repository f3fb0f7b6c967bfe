"""Dynamic fp16 loss scale on a real MI355X: the update kernel against torch._amp_update_scale_, the scaled Adam launch through the C ABI
(including a group boundary in the second grid-stride sweep), FlatAdam + DynamicLossScale against GradScaler("cpu") + torch.optim.Adam, the
static path's launches, and RC-Net / SML fp16 training steps, eager against graphed."""
import pytest

from tests import parity_cases_glue as G
from tests import parity_cases_loss_scale as S

pytestmark = pytest.mark.gpu


def test_update_matches_torch(gpu):
    S.update_case(gpu)


def test_update_floor(gpu):
    S.update_floor_case(gpu)


def test_update_refusals(gpu):
    S.update_refusal_case(gpu)


def test_scaled_adam(gpu):
    S.scaled_adam_case(gpu)
    G.report()


def test_scaled_adam_first_applied_step(gpu):
    S.first_applied_step_case(gpu)


def test_scaled_adam_found_inf(gpu):
    S.scaled_adam_found_inf_case(gpu)


def test_scaled_adam_refusals(gpu):
    S.scaled_adam_refusal_case(gpu)


def test_scaled_adam_second_sweep(gpu):
    S.scaled_adam_large_case(gpu)
    G.report()


def test_flat_adam_dynamic(gpu):
    S.flat_adam_dynamic_case(gpu)
    G.report()


def test_static_path_unchanged(gpu):
    S.static_path_case(gpu)


def test_step_tape_seed_reads_the_live_tensor(gpu):
    S.seed_case(gpu)


def test_rcnet_fp16_eager_and_graphed(gpu):
    S.rcnet_fp16_case(gpu)
    G.report()


def test_sml_fp16_eager_and_graphed(gpu):
    S.sml_fp16_case(gpu)
