"""No GPU: tests/route_cases.py declares one case for every kernel instance the library lists (iamf_hip_route_instances
walks the lists of render_route.hpp and resample_route.hpp that the launchers dispatch over).  An instance added to a list
without a case fails here, by name; so does a case whose instance the build no longer holds."""
import iac_amd as A
import route_cases as R

# the edges tests/test_gpu_route_coverage.py must keep running: they repeat an instance another case declares, so the
# set comparison below would not miss them
EDGES = ["wide4_lfe_m4_c6_512_streams", "wide4_lfe_m4_c6_511_streams", "lpcm_m1_oc2_1025_streams", "wide_m12_c11_s24",
         "wide_m12_c11_s32", "wide_m1_c24", "wide_m14_c24", "wide_m24_c24", "rs_block_c2_r2_255_streams",
         "rs_block_c6_r2_256_streams", "rs_direct_c2_n64_63_streams", "rs_direct_c2_n64_256_streams",
         "rs_direct_c2_n96_64_streams", "rs_direct_c2_n128_255_streams", "rs_direct_c6_n192_64_streams"]
# families whose every instance a call through the public ABI reaches (custom matrices, the projection and environment
# switches): none of them may be declared unreachable
ALL_REACHABLE = {"GENERIC", "NOLIM", "FAST", "WIDE", "WIDE4", "WIDE4_LFE", "LPCM", "FANOUT", "RS_PLAIN", "RS_TILE", "RS_BLOCK"}


def test_listing_is_a_set_of_known_families():
    rows = A.route_instances()
    assert len(rows) == len(set(rows)) and len(rows) > 400
    assert all(r[0] in A.ROUTE and r[0] != "NONE" for r in rows)
    assert A.lib().iamf_hip_route_instances(None, 0) == len(rows)   # nothing was dropped for want of room
    assert A.route_tally(reset=False) == {}                        # no launch without a GPU


def test_every_instance_has_a_case_and_every_case_an_instance():
    listed = set(A.route_instances())
    declared = {c.inst for c in R.CASES}
    unreachable = {u.inst for u in R.UNREACHABLE}
    assert not (declared & unreachable), sorted(declared & unreachable)
    missing = sorted(listed - declared - unreachable)
    assert not missing, "instances without a case in tests/route_cases.py: %s" % missing
    stale = sorted((declared | unreachable) - listed)
    assert not stale, "cases for instances the build does not hold: %s" % stale


def test_case_ids_are_unique_and_the_edges_are_there():
    ids = [c.id for c in R.CASES] + [u.id for u in R.UNREACHABLE]
    assert len(ids) == len(set(ids))
    assert not [e for e in EDGES if e not in ids]


def test_unreachable_entries_name_their_rule_and_stay_out_of_the_reachable_families():
    for u in R.UNREACHABLE:
        assert u.inst[0] not in ALL_REACHABLE, u.id
        assert len(u.rule) > 40 and u.kw.get("routed") and u.kw["routed"] != u.inst, u.id
    # the resampler's three: the direct kernel's 192-tap instances for the channel counts its launcher leaves to the tiled kernel
    assert sorted(u.inst for u in R.UNREACHABLE) == [("RS_DIRECT", 3, 192, 1, 4), ("RS_DIRECT", 3, 192, 2, 4), ("RS_DIRECT", 3, 192, 8, 2)]
