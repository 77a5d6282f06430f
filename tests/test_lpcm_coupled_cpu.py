"""No GPU: the route listing by family (iamf_hip_route_family_instances, _family_tally) and the family it was added for, the
instances of the coupled 16-bit LPCM form of the headline kernel (LPCM_COUPLED), which no numbered table lists."""
import os
import subprocess

import pytest

import iac_amd as A

COUPLED_M = [2, 6, 8, 10, 12]


def test_the_symbols_are_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("iamf_hip_route_family_instances", "iamf_hip_route_family_tally"):
        assert name in names, name
        assert hasattr(A.lib(), name)
    assert "iamf_hip_fast_lpcm_coupled_launch" not in names and "iamf_hip_route_count_family" not in names   # internal entries
    assert callable(A.route_family_instances) and callable(A.route_family_tally)
    assert A.ROUTE["LPCM_COUPLED"] == 17 and A.hipabi.ROUTE_NAME[17] == "LPCM_COUPLED"
    with open(os.path.join(os.path.dirname(A.__file__), "..", "include", "iamf_hip.h")) as f:
        header = f.read()
    assert "IAMF_HIP_ROUTE_LPCM_COUPLED = 17" in header
    for name in ("iamf_hip_route_family_instances(int family, iamf_hip_route_row *rows, int cap)",
                 "iamf_hip_route_family_tally(int family, iamf_hip_route_row *rows, int cap, int reset)"):
        assert name in header, name


def test_the_coupled_family_has_20_rows_and_shares_none_with_a_table():
    rows = A.route_family_instances("LPCM_COUPLED")
    want = {("LPCM_COUPLED", early, m, oc, 0) for m in COUPLED_M for oc in (1, 2) for early in (0, 1)}
    assert len(rows) == len(set(rows)) == 20 and set(rows) == want
    assert A.route_family_instances(17) == rows
    assert A.lib().iamf_hip_route_family_instances(17, None, 0) == 20
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == "LPCM_COUPLED"], t
    row = (A.RouteRow * 3)()
    assert A.lib().iamf_hip_route_family_instances(17, row, 3) == 20     # cap rows filled, the count returned
    assert all(A.hipabi.ROUTE_NAME[r.family] == "LPCM_COUPLED" and r.launches == 0 for r in row)


def test_the_tables_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9


@pytest.mark.parametrize("family,table", [("LPCM", 0), ("FANOUT_LPCM", 1), ("LPCM24", 2)])
def test_a_family_of_a_table_is_that_tables_rows(family, table):
    want = [r for r in A.route_table_instances(table) if r[0] == family]
    assert want and A.route_family_instances(family) == want
    assert A.route_family_tally(family) == {}


def test_every_family_of_table_0_is_listed_in_table_order():
    base = A.route_instances()
    for family in sorted({r[0] for r in base}):
        assert A.route_family_instances(family) == [r for r in base if r[0] == family], family


def test_an_unknown_family_is_minus_1():
    L = A.lib()
    for fam in (-1, 0, 18, 19, 24, 1000):
        assert L.iamf_hip_route_family_instances(fam, None, 0) == -1, fam
        assert L.iamf_hip_route_family_tally(fam, None, 0, 0) == -1, fam
        assert L.iamf_hip_route_family_tally(fam, None, 0, 1) == -1, fam
        with pytest.raises(A.IamfHipError):
            A.route_family_instances(fam)
        with pytest.raises(A.IamfHipError):
            A.route_family_tally(fam)


def test_empty_tallies():
    # no launch without a device: every family's tally is empty, with and without a reset
    for family in ("LPCM_COUPLED", "LPCM", "FANOUT_LPCM", "LPCM24", "FAST", "GENERIC"):
        assert A.route_family_tally(family) == {} and A.route_family_tally(family, reset=True) == {}, family
    assert A.lib().iamf_hip_route_family_tally(17, None, 0, 0) == 0
