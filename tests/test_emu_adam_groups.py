"""Parameter groups of the fused Adam under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): the kernel through the
C ABI, FlatAdam built from torch's list of group dictionaries, the state exchange with torch.optim.Adam and the bucketing.  quick=True drops only
the 2 M-element arena (a group boundary in the second grid-stride sweep), which runs on the GPU twin."""
import ctypes
import re

from riders_amd import _lib
from tests import parity_cases_adam_groups as A
from tests import parity_cases_glue as G


def test_adam_groups_matches_c_layout():
    """rd_adam_groups: the ctypes mirror has the header's members in the header's order, types and array lengths"""
    src = open(_lib.HEADER).read()
    assert int(re.search(r"#define\s+RD_ADAM_MAX_GROUPS\s+(\d+)", src).group(1)) == _lib.RD_ADAM_MAX_GROUPS == 8
    for name, val in (("RD_ADAM_DECOUPLED", _lib.ADAM_DECOUPLED), ("RD_ADAM_INACTIVE", _lib.ADAM_INACTIVE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == val
    body = re.search(r"typedef struct rd_adam_groups\s*\{(.*?)\}\s*rd_adam_groups;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for n in rest.split(","):
            m = re.match(r"^(\w+)(?:\[RD_ADAM_MAX_GROUPS\])?$", n.strip())
            assert m, decl
            fields.append((m.group(1), ctype[ty] * 8 if "[" in n else ctype[ty]))
    assert fields == list(_lib.AdamGroups._fields_), (fields, _lib.AdamGroups._fields_)
    # int32 count + 8 int32 flags, 4 bytes of padding in front of the int64 arrays, 2 x 8 int64, 5 x 8 float
    assert _lib.AdamGroups.end.offset == 40 and ctypes.sizeof(_lib.AdamGroups) == 40 + 2 * 64 + 5 * 32
    restype, argtypes = _lib.parse_header()["rd_adam_step_groups"]
    assert restype is ctypes.c_int and argtypes[5] is ctypes.POINTER(_lib.AdamGroups) and len(argtypes) == 9


def test_kernel_groups(emu):
    A.kernel_multi_case(emu, quick=True)
    A.kernel_eight_case(emu, quick=True)
    G.report()


def test_kernel_refusals(emu):
    A.kernel_refusal_case(emu, quick=True)


def test_kernel_inactive_group(emu):
    A.kernel_inactive_case(emu, quick=True)


def test_kernel_skip_flag(emu):
    A.kernel_skip_flag_case(emu, quick=True)


def test_kernel_ties_to_adam_step(emu):
    A.kernel_ties_to_adam_step_case(emu, quick=True)


def test_flat_adam_groups(emu):
    A.flat_adam_groups_case(emu, quick=True)
    A.flat_adam_idle_group_case(emu, quick=True)
    G.report()


def test_flat_adamw(emu):
    A.flat_adamw_case(emu, quick=True)


def test_reference_literal_form(emu):
    A.reference_literal_case(emu, quick=True)


def test_constructor_refusals(emu):
    A.constructor_refusals_case(emu, quick=True)


def test_state_exchange(emu):
    A.state_exchange_case(emu, quick=True)


def test_bucketing(emu):
    A.bucketing_case(emu, quick=True)
