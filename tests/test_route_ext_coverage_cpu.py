"""No GPU: tests/route_cases_ext.py declares one case for every kernel instance of the library's extension table
(iamf_hip_route_instances_ext walks the lists of render_route.hpp its launcher dispatches over), the extension table and the
base table share no row, and the base listing holds no row of an extension family."""
import iac_amd as A
import route_cases_ext as RX


def test_ext_listing_needs_no_device_and_is_disjoint_from_the_base_listing():
    rows = A.route_instances_ext()
    assert rows and len(rows) == len(set(rows))
    assert A.lib().iamf_hip_route_instances_ext(None, 0) == len(rows)
    assert all(r[0] == "FANOUT_LPCM" and r[1] == 0 and r[3] == 0 for r in rows), rows
    assert A.ROUTE["FANOUT_LPCM"] == 15
    base = A.route_instances()
    assert not set(rows) & set(base)
    assert not [r for r in base if r[0] == "FANOUT_LPCM"]
    assert A.route_tally_ext(reset=False) == {}        # no launch without a GPU


def test_every_ext_instance_has_a_case_and_every_case_an_instance():
    listed = set(A.route_instances_ext())
    declared = {c.inst for c in RX.CASES}
    missing = sorted(listed - declared)
    assert not missing, "extension instances without a case in tests/route_cases_ext.py: %s" % missing
    stale = sorted(declared - listed)
    assert not stale, "cases for instances the build does not hold: %s" % stale
    ids = [c.id for c in RX.CASES]
    assert len(ids) == len(set(ids))


def test_the_instances_lie_inside_the_lists_they_intersect():
    import route_cases as R
    for _, _, m, _, k in A.route_instances_ext():
        assert m in R.LPCM_M and m in R.FAN_M and ("FANOUT", 0, m, 0, k) in set(A.route_instances())
