"""The kernel-level routes, pinned: every routing query of the C ABI must answer exactly what tests/route_table.jsonl records (see
tests/route_table.py for what is recorded and at which commit).  Host code only -- no launch, no allocation."""
import ctypes
import re

import pytest

from tests import route_table as R


def _check(lib):
    table = R.load_table()
    want = R.entries()
    assert len(table) == len(want), "route_table.jsonl does not match the descriptor list: re-record it (python -m tests.route_table)"
    for row, (fields, opts) in zip(table, want):
        assert row["d"] == [fields[k] for k in R.FIELDS] and [o for o, _ in row["runs"]] == opts
        for o, a in row["runs"]:
            assert R.answers(lib, fields, o) == a, (fields, o)


def test_route_table_reaches_every_route():
    """every route's kernel family appears among the recorded names, in every dtype it exists in"""
    table = R.load_table()
    for dt in R.DTYPES:
        part = [a for r in table if r["d"][0] == dt for _, a in r["runs"]]
        fwd = [a[k] for a in part for k in ("fwd", "fused_in", "fused_bn", "fused_both")]
        wg = [a[k] for a in part for k in ("wgrad", "wgrad_fused_in")]
        for fam in R.FWD_ALL + (R.FWD_16 if dt else ()):
            assert any(re.search(fam, n) for n in fwd), (dt, fam)
        for fam in R.WG_ALL + (R.WG_16 if dt else R.WG_32):
            assert any(re.search(fam, n) for n in wg), (dt, fam)


def test_kernel_route_table(emu_lib_path):
    from riders_amd import _lib
    _check(_lib._bind(ctypes.CDLL(emu_lib_path)))


@pytest.mark.gpu
def test_kernel_route_table_gpu(gpu):
    from riders_amd import engine
    _check(engine.L())
