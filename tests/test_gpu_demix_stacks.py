"""-m gpu: scalable channel audio at stage level on EVERY layer stack the format allows (demix_cases.all_stacks: the 175
chains of the nine layouts, 46 classes of (target layout, de-mix step mask)), on the frame geometries that decide the
route, and on frames whose start was trimmed (iamf_hip_render_args::demix_sample0).

decoded layers -> iamf_hip_batch_set_demixer's stage -> identity -> limiter -> s16, once as routed and once with
IAMF_HIP_NO_WIDE4=1 (the general kernel's demixer): both equal, bit for bit, (oracle demixer, pinned to the reference's
demixer.c on the same 175 cases by tests/test_oracle_golden.py) -> O.limiter_run -> O.pack, for both streams (stream 1
lands in another lane column).  The launch tally of the routed run is asserted, so a silent fall-back cannot pass."""
import numpy as np
import pytest

import demix_cases as D
import oracle_lib as O
import route_cases as R
import synth

pytestmark = pytest.mark.gpu

S = 2
STACKS = D.all_stacks()


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available()
    import iac_amd as A
    import gpu_util as G
    return A, G


def _samples(call, fs):
    return call[1] if isinstance(call, tuple) else call * fs


def expected_tally(c, calls):
    """render_route.hpp (pick_route, wide_shape_ok, wide4_shape_ok) and iamf_hip_batch_set_demixer restated for these runs
    (identity, s16, limiter on, dense 16-byte aligned buffers, no decoded channel gained twice): a call takes
    render_wide4_kernel<m, m, DMX> exactly when
      the batch allows it      m in {6, 8, 10, 12}, fs >= 256, pre % 4 == 0 and pre + fs / 16 <= 192 (demix_w4: the kernel
                               keeps the first 192 window entries and reads them four at a time);
      the call's shape does    whole 64-sample groups, whole 1024-sample chunks or a last one of at least 256; the stream at
                               a multiple of 16 or 240 samples on;
      a trimmed start does     demix_sample0 % 4 == 0;
    else the general kernel, as does the flush and every target of one or two channels."""
    m, fs, pre = len(c["order"]), c["fs"], c["offset"] % c["fs"]
    batch = m in R.WIDE4_DEMIX_M and fs >= 256 and pre % 4 == 0 and pre + fs // 16 <= 192
    out, pos = [], 0
    for call in calls:
        if isinstance(call, tuple) and call[0] == "refuse":
            continue
        n = _samples(call, fs)
        s0 = call[0] if isinstance(call, tuple) else 0
        shape = n % 64 == 0 and (n % 1024 == 0 or n % 1024 >= 256) and (pos % 16 == 0 or pos >= 240)
        out.append((("WIDE4_DEMIX", 0, m, m, 0) if batch and shape and s0 % 4 == 0 else R.gen(m), 1))
        pos += n
    return out + [(R.gen(m), 1)]


def check(hip, c, calls, what):
    A, G = hip
    fs, F, ch = c["fs"], len(c["schedule"]), len(c["order"])
    x = np.stack([np.stack([synth.uniform(c["seed"] + 100 * s + f, ch, fs, 0.9) for f in range(F)]) for s in range(S)])
    made = [call for call in calls if not (isinstance(call, tuple) and call[0] == "refuse")]
    assert sum(1 if isinstance(call, tuple) else call for call in made) == F
    want = []
    for s in range(S):
        dem = D.drive_demixer(O.lib(), "orc_demixer_", c, x[s])    # [F][ch][fs]: whole frames, as the reference demixes
        parts, f0 = [], 0                                          # them before iamf_frame_trim cuts
        for call in made:
            if isinstance(call, tuple):
                parts.append(dem[f0][:, call[0]:call[0] + call[1]])
                f0 += 1
            else:
                parts += [dem[f] for f in range(f0, f0 + call)]
                f0 += call
        z, _ = O.limiter_run(np.ascontiguousarray(np.concatenate(parts, axis=1)), [_samples(call, fs) for call in made])
        want.append(O.pack(z, 16))
    mx = G.identity_matrix(ch)
    A.route_reset()
    got = R.demix_render(A, c, mx, ch, x, calls)
    tally = A.route_tally()
    with R.environment({"IAMF_HIP_NO_WIDE4": "1"}):
        ref = R.demix_render(A, c, mx, ch, x, calls)
    for s in range(S):
        R.compare(ref[s], want[s], 0, (what, s, "general kernel"))
        R.compare(got[s], want[s], 0, (what, s, "as routed"))
    R.check_tally(tally, expected_tally(c, calls))
    return tally


def check_all(hip, items):
    """check() for every (label, case, calls) of a group: the group fails with the list of ITS failing members, each
    with what differed, so one stack that is wrong does not hide the state of the others"""
    failed = []
    for label, c, calls in items:
        try:
            check(hip, c, calls, label)
        except AssertionError as e:
            failed.append((label, str(e).splitlines()[0][:300] if str(e) else "assert"))
    assert not failed, "%d of %d failed: %s" % (len(failed), len(items), failed)


_TARGETS = ["mono", "stereo", "5.1", "5.1.2", "5.1.4", "7.1", "7.1.2", "7.1.4", "3.1.2"]   # IAChannelLayoutType 0..8


@pytest.mark.parametrize("target", range(9), ids=lambda t: _TARGETS[t])
def test_every_stack_exact_on_both_demixers(hip, target):
    """every stack of all_stacks() that ends in this target layout (1 + 2 + 4 + 12 + 24 + 8 + 32 + 88 + 4 = 175 over the
    nine groups), each with the gains, defaults, offset and schedule of demix_cases.stack_case(i): 256-sample frames in
    calls of 4 and 6, so that a 1024-sample chunk holds the records of four frames.  One test per target, not per stack:
    a stack takes some 15 ms, and the failure message names every stack of the group that differs."""
    items = [((i, st), D.stack_case(i), [4, 6]) for i, st in enumerate(STACKS) if st[-1] == target]
    check_all(hip, items)


_GEOMETRY_STACKS = [[0, 1, 8, 3, 4, 7], [2, 3], [5, 6, 7]]   # the full mask 63; mask 0 into 5.1.2; mask 32 into 7.1.4


@pytest.mark.parametrize("offset", [128, 132, 1000])
def test_frame_geometry_decides_the_route(hip, offset):
    """1024-sample frames (cross-fade of 64) on three stacks: offset 128 ends the cross-fade at 192 exactly (wide4), 132
    behind it (general kernel), 1000 leaves no room for a cross-fade at all (pre + ov > fs: windows of 1 and 0 throughout)"""
    for layers in _GEOMETRY_STACKS:
        c = D.stack_case(STACKS.index(layers), fs=1024, offset=offset)
        tally = check(hip, c, [4, 6], (layers, offset))
        assert (("WIDE4_DEMIX", 0, len(c["order"]), len(c["order"]), 0) in tally) == (offset == 128), (layers, tally)


_TRIM_STACKS = [[1, 3, 7], [8, 3, 6], [0, 1, 2]]
# (frame size, demix_sample0, samples).  256-sample frames, offset 8: the previous mode's prefix is [0, 8), the cross-fade
# [8, 24).  Calls of fewer than 256 samples, or not of whole 64-sample groups, are the general kernel's whatever their
# start; the 1024-sample rows (prefix [0, 8), cross-fade [8, 72)) are calls the wide4 kernel takes with a start inside
# the prefix, inside the cross-fade and behind it, and gives up for a start that is no multiple of 4.
_TRIMS = [(256, 4, 252), (256, 12, 244), (256, 24, 232), (256, 200, 40), (256, 12, 100), (256, 5, 251), (256, 13, 50),
          (1024, 4, 960), (1024, 64, 960), (1024, 200, 768), (1024, 5, 960)]


def _trim_calls(fs, s0, n, refusals=()):
    head, rest = ([2, 2], [3, 2]) if fs == 256 else ([1, 1], [2, 1])
    return head + list(refusals) + [(s0, n)] + rest


def _trim_case(layers, fs):
    c = D.stack_case(STACKS.index(layers), fs=fs, offset=8)
    if fs == 1024:
        c["schedule"] = c["schedule"][:6]
    return c


@pytest.mark.parametrize("layers", _TRIM_STACKS, ids=lambda l: "_".join(str(v) for v in l))
def test_frame_with_a_trimmed_start(hip, layers):
    """A frame whose first s0 samples were cut before the call, the way the decoder facade's render_tu makes the call
    (include/iamf_hip.h): the channel rows START AT SAMPLE s0 of the frame (moved to the front of rows that stay
    frame_size apart), the record is that frame's own record, n_frames = 1, demix_sample0 = s0, n_samples = n.  The
    expectation demixes the WHOLE frame, as the reference does before iamf_frame_trim, and cuts [s0, s0 + n) out of it;
    limiter and pack run over the call lengths actually made.  Whole-frame calls in front of and behind the trimmed one keep
    their kernel; the trimmed call itself is the wide4 kernel's only where its length is one that kernel takes (the tally
    check() asserts; tests/test_demix_stacks_cpu.py spells it out per row).  Every
    (frame size, s0, n) of _TRIMS on this stack; the failure message names the ones that differ."""
    check_all(hip, [((layers, fs, s0, n), _trim_case(layers, fs), _trim_calls(fs, s0, n)) for fs, s0, n in _TRIMS])


def test_trimmed_start_outside_the_frame_is_refused_and_changes_nothing(hip):
    """demix_sample0 + n_samples > frame_size and demix_sample0 < 0: IAMF_HIP_ERR_BAD_ARG, nothing emitted, no state moved —
    the calls behind the refusals still match (on each of the three stacks)"""
    refusals = [("refuse", 200, 100), ("refuse", -4, 16), ("refuse", 256, 0)]
    check_all(hip, [((layers, "refused"), _trim_case(layers, 256), _trim_calls(256, 12, 100, refusals)) for layers in _TRIM_STACKS])
