"""Global-norm gradient clipping on a real MI355X: the norm pass and the finalize through the C ABI (including a second grid-stride sweep), the
finite flag, the clipped Adam launch, FlatAdam.set_grad_clip against torch's clip_grad_norm_ + torch.optim.Adam, the launches with clipping off,
the drop-in riders_amd.clip_grad_norm_, and RC-Net / SML training steps with clipping, eager against graphed."""
import pytest

from tests import parity_cases_glue as G
from tests import parity_cases_grad_clip as C

pytestmark = pytest.mark.gpu


def test_norm_and_finalize(gpu):
    C.norm_case(gpu)
    G.report()


def test_norm_accumulate(gpu):
    C.accumulate_case(gpu)


def test_finite_flag(gpu):
    C.finite_flag_case(gpu)


def test_clipped_adam_coef_one_is_bit_identical(gpu):
    C.clipped_adam_identity_case(gpu)


def test_clipped_adam(gpu):
    C.clipped_adam_case(gpu)
    G.report()


def test_clipped_adam_skip(gpu):
    C.clipped_adam_skip_case(gpu)


def test_refusals(gpu):
    C.refusal_case(gpu)


def test_flat_adam_against_torch(gpu):
    C.flat_adam_case(gpu)
    G.report()


def test_off_means_untouched(gpu):
    C.off_case(gpu)


def test_drop_in_function(gpu):
    C.drop_in_case(gpu)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_rcnet_eager_and_graphed(gpu, precision):
    C.rcnet_case(gpu, precision)
    G.report()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_sml_eager_and_graphed(gpu, precision):
    C.sml_case(gpu, precision)
    G.report()
