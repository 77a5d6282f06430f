"""What tests/test_gpu_demix_stacks.py will ask of the device, checked where there is none: its cases and its restatement
of the routing rules."""
import demix_cases as D
import test_gpu_demix_stacks as T


def test_the_cases_reach_the_wide4_demixer_in_every_class_it_serves():
    """every (target layout, step mask) class of six channels or
    more has a stack whose case the routed run sends to render_wide4_kernel<.., DMX>, and one it does not"""
    classes = {}
    for i in range(len(T.STACKS)):
        c = D.stack_case(i)
        t = T.expected_tally(c, [4, 6])
        classes.setdefault((c["layout"], c["steps"]), []).append(t[0][0][0])
    assert len(classes) == 46
    for k, v in classes.items():
        if len(D.PLAYBACK[k[0]]) >= 6:
            assert "WIDE4_DEMIX" in v, k
            assert len(v) == 1 or "GENERIC" in v, k
        else:
            assert set(v) == {"GENERIC"}, k


def test_trimmed_cases_name_the_kernels_the_rules_give():
    """the trimmed call is the wide4 kernel's only at a length that kernel takes (whole 64-sample groups, at least 256) and
    a start that is a multiple of 4; the whole-frame calls around it keep theirs"""
    w = ("WIDE4_DEMIX", 0, 12, 12, 0)
    for fs, s0, n in T._TRIMS:
        c = D.stack_case(T.STACKS.index([1, 3, 7]), fs=fs, offset=8)
        got = [k for k, _ in T.expected_tally(c, T._trim_calls(fs, s0, n))]
        assert got[:2] == [w, w] and got[3:5] == [w, w] and got[5] == ("GENERIC", 0, 12, 0, 0), (fs, s0, n, got)
        assert (got[2] == w) == (fs == 1024 and s0 % 4 == 0), (fs, s0, n, got)


def test_the_target_groups_hold_every_stack_once():
    """the GPU test runs the stacks in nine groups, by target layout"""
    assert sorted(i for t in range(9) for i, st in enumerate(T.STACKS) if st[-1] == t) == list(range(175))
    assert [sum(st[-1] == t for st in T.STACKS) for t in range(9)] == [1, 2, 4, 12, 24, 8, 32, 88, 4]
