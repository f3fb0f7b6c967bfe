"""Layout, LayerNorm, loss and Adam kernels one by one under the fiber emulator (see tests/test_emu_ops.py for what these are and are not).
quick=True drops only the sizes above 100 K elements (the grid-stride second iterations), which run on the GPU twin."""
from tests import parity_cases_glue as G


def test_add(emu):
    G.add_case(emu, quick=True)


def test_cast(emu):
    G.cast_case(emu, quick=True)


def test_layouts(emu):
    G.layout_case(emu, quick=True)


def test_upsample_nearest(emu):
    G.upsample_case(emu, quick=True)


def test_layernorm(emu):
    G.layernorm_case(emu, quick=True)


def test_colsum(emu):
    G.colsum_case(emu, quick=True)


def test_act_bwd(emu):
    G.act_bwd_case(emu, quick=True)


def test_bce_and_sigmoid(emu):
    G.bce_case(emu, quick=True)


def test_adam(emu):
    G.adam_case(emu, quick=True)
    G.report()
