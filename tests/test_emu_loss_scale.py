"""Dynamic fp16 loss scale under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): the state's layout, the update
kernel against torch._amp_update_scale_, the scaled Adam launch through the C ABI, FlatAdam + DynamicLossScale against GradScaler("cpu") +
torch.optim.Adam, and the static path's launches.  quick=True drops only the 2 M-element arena; the RC-Net and SML fp16 steps, eager against
graphed, run on the GPU twin."""
import ctypes
import re

from riders_amd import _lib
from tests import parity_cases_glue as G
from tests import parity_cases_loss_scale as S


def test_loss_scale_state_matches_c_layout():
    """rd_loss_scale_state: the ctypes mirror has the header's members in the header's order and types, 32 bytes, with (found_inf, skipped) the
    int32 pair at byte 8 that rd_grad_finite_check and rd_adam_skip_count know as `flag`; the three entries parse from the header"""
    src = open(_lib.HEADER).read()
    body = re.search(r"typedef struct rd_loss_scale_state\s*\{(.*?)\}\s*rd_loss_scale_state;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for n in rest.split(","):
            assert re.match(r"^\w+$", n.strip()), decl
            fields.append((n.strip(), ctype[ty]))
    assert fields == list(_lib.LossScaleState._fields_), (fields, _lib.LossScaleState._fields_)
    assert [n for n, _ in fields] == ["scale", "inv_scale", "found_inf", "skipped", "growth_tracker", "backoffs", "growths", "reserved"]
    assert ctypes.sizeof(_lib.LossScaleState) == 32
    assert _lib.LossScaleState.found_inf.offset == 8 and _lib.LossScaleState.skipped.offset == 12
    assert _lib.LossScaleState.scale.offset == 0 and _lib.LossScaleState.inv_scale.offset == 4
    protos = _lib.parse_header()
    i32, f32, i64, vp = ctypes.c_int32, ctypes.c_float, ctypes.c_int64, ctypes.c_void_p
    assert protos["rd_loss_scale_init"] == (ctypes.c_int, [vp, f32, i32, vp])
    assert protos["rd_loss_scale_update"] == (ctypes.c_int, [vp, f32, f32, i32, vp])
    assert protos["rd_adam_step_groups_scaled"] == (ctypes.c_int, [vp, vp, vp, vp, i64, ctypes.POINTER(_lib.AdamGroups), f32, vp, i32, vp])
    assert len(protos["rd_adam_step_groups"][1]) == 9      # no existing signature moved


def test_update_matches_torch(emu):
    S.update_case(emu, quick=True)


def test_update_floor(emu):
    S.update_floor_case(emu, quick=True)


def test_update_refusals(emu):
    S.update_refusal_case(emu, quick=True)


def test_scaled_adam(emu):
    S.scaled_adam_case(emu, quick=True)
    G.report()


def test_scaled_adam_first_applied_step(emu):
    S.first_applied_step_case(emu, quick=True)


def test_scaled_adam_found_inf(emu):
    S.scaled_adam_found_inf_case(emu, quick=True)


def test_scaled_adam_refusals(emu):
    S.scaled_adam_refusal_case(emu, quick=True)


def test_flat_adam_dynamic(emu):
    S.flat_adam_dynamic_case(emu, quick=True)
    G.report()


def test_static_path_unchanged(emu):
    S.static_path_case(emu, quick=True)


def test_step_tape_seed_reads_the_live_tensor(emu):
    S.seed_case(emu, quick=True)
