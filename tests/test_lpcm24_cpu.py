"""No GPU: the indexed route listing (iamf_hip_route_tables, _table_instances, _table_tally) and its table 2, the
instances of the 24-bit LPCM form of the headline kernel."""
import ctypes as C
import os
import subprocess

import pytest

import iac_amd as A
import route_cases as R


def test_the_symbols_are_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("iamf_hip_route_tables", "iamf_hip_route_table_instances", "iamf_hip_route_table_tally"):
        assert name in names, name
        assert hasattr(A.lib(), name)
    assert "iamf_hip_fast_lpcm24_launch" not in names and "iamf_hip_route_count_table" not in names   # internal entries
    assert callable(A.route_table_instances) and callable(A.route_table_tally) and callable(A.route_tables)
    assert A.ROUTE["LPCM24"] == 16
    with open(os.path.join(os.path.dirname(A.__file__), "..", "include", "iamf_hip.h")) as f:
        header = f.read()
    assert "IAMF_HIP_ROUTE_LPCM24 = 16" in header
    for name in ("iamf_hip_route_tables(void)", "iamf_hip_route_table_instances(int table", "iamf_hip_route_table_tally(int table"):
        assert name in header, name


def test_three_tables_and_the_first_two_are_the_existing_listings():
    assert A.route_tables() == 3
    assert A.route_table_instances(0) == A.route_instances()
    assert A.route_table_instances(1) == A.route_instances_ext()
    for t, n in ((0, len(A.route_instances())), (1, len(A.route_instances_ext())), (2, 16)):
        assert A.lib().iamf_hip_route_table_instances(t, None, 0) == n
    # the same counters, not copies: nothing launched, and reading through either symbol agrees
    assert A.route_table_tally(0) == A.route_tally(reset=False) == {}
    assert A.route_table_tally(1) == A.route_tally_ext(reset=False) == {}


def test_table_2_is_the_lpcm24_instances_and_nothing_else():
    rows = A.route_table_instances(2)
    want = {("LPCM24", early, m, oc, 0) for m in R.LPCM_M for oc in (1, 2) for early in (0, 1)}
    assert len(rows) == len(set(rows)) == 16 and set(rows) == want
    assert not set(rows) & set(A.route_instances()) and not set(rows) & set(A.route_instances_ext())
    assert not [r for r in A.route_instances() + A.route_instances_ext() if r[0] == "LPCM24"]
    # the rows pair off with the 16-bit family's
    assert {("LPCM",) + r[1:] for r in rows} == {r for r in A.route_instances() if r[0] == "LPCM"}
    assert A.route_table_tally(2) == {} and A.route_table_tally(2, reset=True) == {}   # no launch without a device


def test_a_table_outside_the_range_is_a_bad_argument():
    L = A.lib()
    for t in (-1, 3, 100):
        assert L.iamf_hip_route_table_instances(t, None, 0) == -1
        assert L.iamf_hip_route_table_tally(t, None, 0, 0) == -1
        with pytest.raises(A.IamfHipError):
            A.route_table_instances(t)
        with pytest.raises(A.IamfHipError):
            A.route_table_tally(t)
    row = (A.RouteRow * 1)()
    assert L.iamf_hip_route_table_instances(2, row, 1) == 16 and A.hipabi.ROUTE_NAME[row[0].family] == "LPCM24"
    assert row[0].launches == 0
