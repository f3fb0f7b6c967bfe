"""Global-norm gradient clipping under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): the state's layout, the norm
pass and the finalize through the C ABI, the finite flag, the clipped Adam launch, FlatAdam.set_grad_clip against torch's clip_grad_norm_ +
torch.optim.Adam (plain, under a DynamicLossScale against GradScaler("cpu"), under a static scale), the launches with clipping off, and the
drop-in riders_amd.clip_grad_norm_.  quick=True drops only the 2 M-element arenas; the RC-Net and SML steps, eager against graphed, run on the
GPU twin."""
import ctypes
import re

from riders_amd import _lib
from tests import parity_cases_glue as G
from tests import parity_cases_grad_clip as C


def test_grad_clip_state_matches_c_layout():
    """rd_grad_clip_state: the ctypes mirror has the header's members in the header's order and types, 32 bytes; the constants agree; the four
    entries parse from the header and the two existing group launches keep their argument counts"""
    src = open(_lib.HEADER).read()
    body = re.search(r"typedef struct rd_grad_clip_state\s*\{(.*?)\}\s*rd_grad_clip_state;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for n in rest.split(","):
            m = re.match(r"^(\w+)(?:\[(\d+)\])?$", n.strip())
            assert m, decl
            fields.append((m.group(1), ctype[ty] * int(m.group(2)) if m.group(2) else ctype[ty]))
    assert fields == list(_lib.GradClipState._fields_), (fields, _lib.GradClipState._fields_)
    assert [n for n, _ in fields] == ["total_norm", "coef", "passes", "clipped", "nonfinite", "reserved"]
    assert ctypes.sizeof(_lib.GradClipState) == 32
    assert [getattr(_lib.GradClipState, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20]
    defines = dict((k, int(v)) for k, v in re.findall(r"#define (RD_GRAD_NORM_\w+) (\d+)", src))
    assert defines == dict(RD_GRAD_NORM_ROWS=_lib.RD_GRAD_NORM_ROWS, RD_GRAD_NORM_L2=_lib.GRAD_NORM_L2, RD_GRAD_NORM_INF=_lib.GRAD_NORM_INF), defines
    assert (C.ROWS, C.L2, C.INF) == (_lib.RD_GRAD_NORM_ROWS, _lib.GRAD_NORM_L2, _lib.GRAD_NORM_INF)
    protos = _lib.parse_header()
    i32, f32, i64, vp = ctypes.c_int32, ctypes.c_float, ctypes.c_int64, ctypes.c_void_p
    assert protos["rd_grad_clip_init"] == (ctypes.c_int, [vp, vp])
    assert protos["rd_grad_norm_partial"] == (ctypes.c_int, [vp, i64, f32, vp, i32, vp, i32, i32, vp, vp])
    assert protos["rd_grad_clip_finalize"] == (ctypes.c_int, [vp, i32, f32, i32, vp, vp])
    assert protos["rd_adam_step_groups_clipped"] == (ctypes.c_int, [vp, vp, vp, vp, i64, ctypes.POINTER(_lib.AdamGroups), f32, vp, vp, i32, vp, vp])
    assert len(protos["rd_adam_step_groups"][1]) == 9 and len(protos["rd_adam_step_groups_scaled"][1]) == 10      # no existing signature moved


def test_norm_and_finalize(emu):
    C.norm_case(emu, quick=True)
    G.report()


def test_norm_accumulate(emu):
    C.accumulate_case(emu, quick=True)


def test_finite_flag(emu):
    C.finite_flag_case(emu, quick=True)


def test_clipped_adam_coef_one_is_bit_identical(emu):
    C.clipped_adam_identity_case(emu, quick=True)


def test_clipped_adam(emu):
    C.clipped_adam_case(emu, quick=True)
    G.report()


def test_clipped_adam_skip(emu):
    C.clipped_adam_skip_case(emu, quick=True)


def test_refusals(emu):
    C.refusal_case(emu, quick=True)


def test_flat_adam_against_torch(emu):
    C.flat_adam_case(emu, quick=True)
    G.report()


def test_off_means_untouched(emu):
    C.off_case(emu, quick=True)


def test_drop_in_function(emu):
    C.drop_in_case(emu, quick=True)
