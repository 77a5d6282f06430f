"""The cases of tests/test_gpu_handover.py, without a GPU (tests/handover_util.py has the table and the programmes).

 * the table and the exclusion list together name every render family of the library's listings
   (iamf_hip_route_instances, _ext, table 2 and the by-family listings), and every row's tally key is a listed instance;
 * every ordered pair of families of a class, A = B included, occurs at one boundary or more; the expected route of both
   calls follows the rules of pick_route() restated in handover_util.takes; 490 cases in all (N 185, NC 103, N2 31, N2P 31,
   ND 15, NI 17, W 28, WM 28, WX 13, WD 13, WS 13, WL 13), in 38 groups by (class, A);
 * every stream of every class is, at every boundary b and for every length of call 2, in the limiter phase its name says
   at the gain steps b - 1 and b, and triggers where the table of phases says — from oracle_lib.limiter_trace alone.  (Step
   k is the one input sample k enters at; it sees the peaks of the 240 samples in front of it, so a peak on input p
   triggers at step p + 1.)

Not in the table, by EXCLUDED: NOLIM (keeps no state), FIR_SPLIT / FIR_FUSED (no bit-exact reference, d_fir_hist is not
exportable), the resampler's kernels; and the façade's and the groups' internal batches, which no call-by-call entry reaches."""
import numpy as np
import pytest

import handover_util as H
import oracle_lib as O


def test_table_and_exclusions_name_every_family():
    import iac_amd as A
    listed = set(A.route_instances()) | set(A.route_instances_ext())
    for t in range(A.route_tables()):
        listed |= set(A.route_table_instances(t))
    for fam in ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED"):
        listed |= set(A.route_family_instances(fam))
    families = {k[0] for k in listed}
    assert families == set(A.ROUTE) - {"NONE"}, sorted(families ^ (set(A.ROUTE) - {"NONE"}))
    in_table = {H.listed_family(r) for r in H.ROWS}
    assert in_table.isdisjoint(H.EXCLUDED), sorted(in_table & set(H.EXCLUDED))
    assert in_table | set(H.EXCLUDED) == families, sorted((in_table | set(H.EXCLUDED)) ^ families)
    for r in H.ROWS:       # every row names an instance of the build
        assert H.key_of(r, H.CLASSES[r.cls]) in listed, r
    assert H.key_of(H.row("N", "FANOUT"), H.CLASSES["N.sib"]) in listed
    # the variants the issue names: both prefetch variants of the packet forms, both LP2, both projections
    keys = {H.key_of(r, H.CLASSES[r.cls]) for r in H.ROWS}
    for k in [("LPCM", 0, 16, 2, 0), ("LPCM", 1, 16, 2, 0), ("LPCM_COUPLED", 0, 6, 2, 0), ("LPCM_COUPLED", 1, 6, 2, 0),
              ("LPCM_MIX", 0, 16, 2, 1), ("LPCM_MIX", 0, 16, 2, 2), ("FAST", 1, 16, 2, 0), ("WIDE4", 1, 12, 12, 0), ("WIDE", 1, 12, 0, 0),
              ("WIDE4_LFE", 0, 16, 6, 0), ("WIDE4_DEMIX", 0, 12, 12, 0), ("WIDE4_DOWN", 0, 12, 10, 0), ("FAST_DOWN", 0, 8, 2, 0), ("WIDE4_MIX", 0, 12, 12, 0)]:
        assert k in keys, k


def test_every_ordered_pair_and_the_case_count():
    cases = H.all_cases()
    assert len(cases) == H.N_CASES == 490
    per = {}
    for c in cases:
        per[c.cls] = per.get(c.cls, 0) + 1
    assert per == H.CASES_PER_CLASS and sorted(per) == sorted(H.CLASS_NAMES)
    assert len({H.case_id(c) for c in cases}) == len(cases)
    assert len(H.groups()) == len(H.ROWS) == 38 and sum(len(v) for v in H.groups().values()) == 490
    for cls in H.CLASS_NAMES:
        rows = H.rows_of(cls)
        assert [r.fam for r in rows].count("GENERIC") == 1
        have = {(c.a.fam, c.b_row.fam) for c in H.cases_of(cls) if c.fam_b is c.b_row}
        for a in rows:
            for b in rows:
                assert (a.fam, b.fam) in have, (cls, a.fam, b.fam)
        assert [c for c in H.cases_of(cls) if c.b == 100 and c.fam_b.fam == "GENERIC"], cls
        assert {c.b for c in H.cases_of(cls)} == set(H.BOUNDARIES), cls


def test_expected_routes_follow_the_rules():
    for c in H.all_cases():
        what = H.case_id(c)
        # call 1 at position 0, call 2 at b: the frames the ABI can form
        for n in (c.b, c.n2):
            assert n % c.fs == 0 or n < c.fs, what
        assert H.takes(c.a, c.b, 0) == c.env_a and c.fam_a is c.a, what
        took = H.takes(c.b_row, c.n2, c.b)
        if c.fam_b is c.b_row:
            assert took == c.env_b, what
        else:      # the position shuts B's family out
            assert took is None and c.fam_b.fam == "GENERIC" and (c.b % 16 != 0), what
            assert c.b < 240 or c.b_row.kind in ("wide", "wide4_16"), what
        # who can leave a stream off the 16-grid
        if c.b in (1000, 100):
            assert c.a.kind in ("ragged", "generic", "generic1", "any"), what
        if c.b == 1088 and c.a.kind.startswith("wide4"):
            raise AssertionError(what)
    # the boundaries the routing rules branch on
    assert 1088 & 1023 == 64 and 1280 & 1023 == 256 and 1000 % 16 and 1000 >= 240 and 100 % 16 and 100 < 240
    w, g = H.row("W", "WIDE"), H.row("W", "GENERIC")
    assert H.takes(w, 1088, 0) == {} and H.takes(w, 1024, 0) == {"IAMF_HIP_NO_WIDE4": "1"} and H.takes(w, 2048, 1000) is None
    assert H.takes(g, 1000, 1024) == {} and H.takes(g, 2048, 1024) == H.FORCE
    assert [c for c in H.cases_of("W") if c.b_row.fam == "WIDE" and c.b == 1000 and c.fam_b.fam == "GENERIC"]
    assert [c for c in H.cases_of("WL") if c.b_row.fam == "WIDE4_LFE" and c.b == 1000 and c.fam_b.fam == "GENERIC"]


def _shapes():
    out = []
    for cls in H.CLASS_NAMES:
        for (b, n2, fs) in H.shapes(cls):
            out.append((cls, b, n2, fs))
            if cls == "N" and n2 == H.N2 or cls == "N" and b == 1000:
                out.append((cls + ".sib", b, n2, fs))
    return out


@pytest.mark.parametrize("cname,b,n2,fs", _shapes(), ids=lambda v: str(v))
def test_every_stream_is_in_its_phase_at_the_boundary(cname, b, n2, fs):
    z = H.limiter_input(cname, b, n2, fs)
    ints, ints2 = H.programme(cname, b, n2, fs)
    assert np.abs(ints).max() < 32768 and (ints2 is None or np.abs(ints2).max() < 32768)
    assert len({(H.EGS[s % 3], H.OGS[s % 3]) for s in range(H.S)}) == 3
    IDLE, ATT, REL, TRIG = O.LIM_IDLE, O.LIM_ATTACK, O.LIM_RELEASE, O.LIM_TRIGGER
    for s, phase in enumerate(H.PHASES):
        what = (cname, b, n2, fs, phase)
        y, t = O.limiter_trace(np.ascontiguousarray(z[s]), [b, n2])
        trig = np.flatnonzero(t & TRIG)
        ph = t & 3
        assert trig.size, what
        # a trigger only where a peak is in the look-ahead window: steps p + 1 .. p + 240
        allowed = np.zeros(t.size, dtype=bool)
        for p, _ in H.peaks(phase, b):
            allowed[p + 1:p + 241] = True
            assert (t[p + 1] & TRIG), (what, "the peak on input %d does not trigger at step %d" % (p, p + 1))
        assert allowed[trig].all(), (what, "a trigger outside the peaks' windows", trig[~allowed[trig]][:4])
        if phase == "idle":
            assert (ph[:b + 301] == IDLE).all() and trig[0] == b + 301 and trig[0] - b >= 300, what
        elif phase == "look-ahead":
            assert (ph[:b + 11] == IDLE).all() and trig[0] == b + 11, what
            # B attenuates samples that A put into the ring: outputs b + 11 - 240 .. b - 1 leave in call 2 with a gain below 1
            k = np.arange(b + 11 - 240, b)
            k = k[k >= 0]
            loud = np.abs(z[s][:, k]).max(axis=0) > 0
            assert loud.any() and (np.abs(y[:, k[loud]]) < np.abs(z[s][:, k[loud]])).any(), what
        elif phase == "mid-attack":
            assert (ph[:b - 19] == IDLE).all() and trig[0] == b - 19, what
            assert ph[b - 1] == ATT and ph[b] == ATT and ph[b + 20] == ATT, what          # under way across the boundary
        elif phase in ("release", "re-trigger"):
            p0 = max(b - 400, 0)
            assert trig[0] == p0 + 1, what
            if b >= 400 + 241:
                assert ph[b - 1] == REL and ph[b] == REL and not (t[b - 100:b + 1] & TRIG).any(), what
            else:      # b = 100: the peak is still in the window
                assert b == 100 and ph[b - 1] != IDLE and ph[b] != IDLE and (t[b - 1] & TRIG) and (t[b] & TRIG), what
            if phase == "re-trigger":
                assert (t[b + 6] & TRIG) and ph[b + 6] == (REL if b >= 641 else ph[b + 6]) and ph[b + 7] == ATT, what
                if b >= 641:
                    assert not (t[b - 100:b + 6] & TRIG).any(), what
            elif b >= 641:
                assert not (trig > b - 100).any() and (ph[b:b + n2] == REL).all(), what
        elif phase == "edge":
            assert (ph[:b] == IDLE).all() and not (t[:b] & TRIG).any(), what
            assert t[b] == (IDLE | TRIG) and (t[b + 1] & TRIG), what         # input b - 1 at B's first step, input b at the second
        # the limiter's gain shows in what is emitted around the boundary
        k = np.arange(max(b - 240, 0), b + 240)
        assert (np.abs(y[:, k]) < np.abs(z[s][:, k])).any() or phase == "idle", what
