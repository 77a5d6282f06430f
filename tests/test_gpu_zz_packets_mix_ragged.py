"""-m gpu: both elements of a two-element mix as LPCM packets in calls of any length (iamf_hip_batch_render_packets_mix_ragged;
render_fast_kernel<.., IN2, LP, true, LPB, LPC, LP2, IL = false, RAG = true>, iac_amd/csrc/iamf_render_packets_mix_ragged*.hip).

Every case runs the new entry on one batch and iamf_hip_batch_render_packets_mix on a twin (packets_mix_ragged_util.check) and
asserts, after every call: the launch tally of every listing on both sides (the new family's row on the first, the general
kernel's in its place on the twin); byte-equal PCM and return values; the exported stream state equal bit for bit; every byte of
the PCM rows outside the emitted runs still 0xA5 (gpu_util.rows_and_rest); and the oracle with a second element, stream by
stream.  Tolerance 0.  Three streams per batch, frames of 64 to 1024 samples, tiny launches.

The name sorts the file behind the existing GPU files, whose order in a run stays as it was."""
import ctypes as C

import numpy as np
import pytest

import packets_mix_ragged_util as U
import route_cases as R
import route_cases_lpcm_mix as RM

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_NO_WIDE4", "IAMF_HIP_DENSE", "IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED")
SHAPE_IDS = sorted(U.SHAPES)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def shape(name, calls, fs, **kw):
    bps, m, oc, k = U.SHAPES[name]
    return U.Mix(bps, m, oc, k, calls, fs, **kw)


# ---- 1. every instance ----

@pytest.mark.parametrize("bps,m,oc,k", U.INSTANCES, ids=["b%d_m%d_oc%d_k%d" % i for i in U.INSTANCES])
def test_every_instance(bps, m, oc, k):
    import iac_amd as A
    assert U.inst(bps, m, oc, k) in A.route_family_instances(U.FAM)
    mix = U.Mix(bps, m, oc, k, [(1, 0)], 1000)
    got, _ = U.check(mix, routes=[U.RAG], what="instance %s" % (U.inst(bps, m, oc, k),))
    assert got[0]["fam"] == {U.inst(bps, m, oc, k): 1}
    z, y0, y1 = mix.pre_limiter(0)
    mix.assert_drives_the_limiter(0, z, y0, y1)


# ---- 2. lengths ----

@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 65, 145, 240, 480, 1000, 1023])
def test_a_single_call_of_any_length(name, n):
    """one frame of 1024 trimmed to n samples, behind a whole frame (the streams stand at 1024: past the look-ahead)"""
    mix = shape(name, [(1, 0), (1, n)], 1024)
    U.check(mix, routes=[U.WHOLE_ROW, U.RAG], what="%d samples" % n)


@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("what,fs,calls", [
    ("one chunk plus one sample", 1025 * 4, [(1, 1025)]),
    ("two chunks plus one sample", 2052, [(1, 2049)]),
    ("three frames of 1000", 1000, [(3, 0)]),
    ("five frames of 120", 120, [(5, 0), (5, 0)]),
], ids=["n1025", "n2049", "frames_3x1000", "frames_5x120"])
def test_calls_that_span_chunks_and_frames(name, what, fs, calls):
    mix = shape(name, calls, fs)
    U.check(mix, routes=[U.RAG] * len(calls), what=what)


@pytest.mark.parametrize("name", SHAPE_IDS)
def test_whole_blocks_take_the_whole_block_family_through_either_entry(name):
    mix = shape(name, [(1, 0), (1, 0)], 1024)
    U.check(mix, routes=[U.WHOLE_ROW, U.WHOLE_ROW], what="1024 samples")


# ---- 3. trimmed frames ----

TRIMS = [(first, n) for first in (0, 4, 212) for n in (1, 25, 145, 300, 354)]


@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("first,n", TRIMS, ids=["f%d_n%d" % t for t in TRIMS])
def test_a_trimmed_frame(name, first, n):
    """frames of 576 samples, nine blocks: first + ((n + 3) & ~3) <= 576 holds for every pair (212 + 356 = 568)"""
    fs = 576
    assert first + ((n + 3) & ~3) <= fs
    mix = shape(name, [(1, 0), (1, n, first)], fs)
    U.check(mix, routes=[U.WHOLE_ROW, U.RAG], what="first %d, %d samples" % (first, n))


@pytest.mark.parametrize("bps", [2, 3])
@pytest.mark.parametrize("n,holds", [(994, True), (997, False)])
def test_a_trimmed_frame_whose_last_quad_would_leave_the_run_is_left_to_the_general_path(bps, n, holds):
    """With the frame size and first_sample multiples of 4 the inequality follows from first + n <= frame_size.  It can fail where
    the forms' grid admits other first samples: a coupled stereo bed with a coupled stereo second element, whose pairs are on
    their grid at every EVEN first sample.  From sample 2 of a frame of 1000: 994 samples end inside the runs (2 + 996 = 998), the
    last quad of 997 would not (2 + 1000 = 1002, though 2 + 997 = 999 is a valid call)"""
    fs, first = 1000, 2
    assert (first + ((n + 3) & ~3) <= fs) == holds and first + n <= fs
    mix = U.Mix(bps, 2, 2, 2, [(1, 0), (1, n, first)], fs)
    U.check(mix, routes=[U.RAG, U.RAG if holds else U.GENERIC], what="first 2, %d samples" % n)


@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("first", [3, 951])
def test_a_first_sample_off_the_grid_is_left_to_the_general_path(name, first):
    mix = shape(name, [(1, 0), (1, 41, first)], 1000)
    U.check(mix, routes=[U.RAG, U.GENERIC], what="first %d" % first)


# ---- 4. garbage behind n_samples and between the runs ----

@pytest.mark.parametrize("name", SHAPE_IDS)
def test_garbage_behind_n_samples_and_between_the_runs_changes_nothing(name):
    """a quiet programme (the limiter stays idle: the exported LimState is a fresh stream's); every sample of the trimmed frame's
    runs outside the call, in both elements, at + or - full scale, and every byte between the runs 0x7F / 0x80.  Two sets of
    garbage: the same PCM and the same state, the oracle's"""
    import lpcm_util as LP
    bps, m, oc, k = U.SHAPES[name]
    fs, S, first, n = 512, 3, 4, 145
    m2, _ = U.second(m, k)
    full = 1 << (8 * bps - 1)
    runs = []
    for sign in (1, -1):
        rng = np.random.default_rng(99)
        i0, i1 = LP.ints(rng, S, 2, m, fs, bps, level=0.02), LP.ints(rng, S, 2, m2, fs, bps, level=0.02)
        for v in (i0, i1):
            g = np.where(np.arange(fs) % 2 == 0, full - 1, -full) * sign
            v[:, 1, :, :first] = g[None, None, :first]
            v[:, 1, :, first + n:] = g[None, None, first + n:]
        mix = U.Mix(bps, m, oc, k, [(1, 0), (1, n, first)], fs, S=S, ints=(i0, i1), fill=True)
        got, _ = U.check(mix, routes=[U.WHOLE_ROW, U.RAG], what="garbage %d" % sign)
        runs.append(got)
    U.assert_same(runs[0], runs[1], "two sets of garbage")
    for r in runs[0][:2]:
        f, steps = U.lim_states(r["state"])
        assert (f[:, 0] == 1.0).all() and (f[:, 1] == -1.0).all() and (f[:, 2] == -1.0).all(), ("the limiter engaged", f)
        assert len(set(int(v) for v in steps)) == 1 and int(steps[0]) > 1088, steps      # idle: n == n_end


# ---- 5. ramps ----

RAMPS = {"none": (), "element2_const": ("e1c",), "all": ("e0", "e1", "out")}


def with_ramps(mix, which):
    for j, w in enumerate(which):
        if w == "e1c":
            mix.const_ramp("e1", [0.8, 1.0, 0.55])
        else:
            mix.ramp(w, j + 1)
    return mix


@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("ramps", sorted(RAMPS))
@pytest.mark.parametrize("n", [145, 1000, 1025])
def test_ramps_are_fused_and_read_up_to_the_calls_end_only(name, ramps, n):
    """the ramp rows hold NaN from index `total` on, and the last stream's rows end with the allocation
    (packets_mix_ragged_util.ramp_rows): a float read at or behind `total` shows in the PCM or leaves the buffer"""
    fs = 1028 if n > 1024 else 1024
    mix = with_ramps(shape(name, [(1, 0), (1, n)], fs), RAMPS[ramps])
    U.check(mix, routes=[U.RAG if fs % 64 else U.WHOLE_ROW, U.RAG], what="ramps %s, %d samples" % (ramps, n))


@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("how", ["row_off_16_bytes", "stride_not_a_multiple_of_4"])
def test_ramp_rows_off_the_grid_are_left_to_the_general_path(name, how):
    mix = with_ramps(shape(name, [(1, 0), (1, 145)], 1024), ("e0", "e1", "out"))
    kw = dict(ramp_shift={"e1": 1}) if how == "row_off_16_bytes" else dict(ramp_stride_extra=1)
    U.check(mix, routes=[U.GENERIC, U.GENERIC], what=how, **kw)


# ---- 6. the limiter ----

@pytest.mark.parametrize("bps", [2, 3])
@pytest.mark.parametrize("name", sorted(U.LIM_CASES))
def test_the_limiter_across_ragged_calls_and_the_other_entries(name, bps):
    """tests/test_packets_mix_ragged_cpu.py proves from the oracle's limiter trace where each case triggers and that its release
    runs across the calls behind it; here: the ragged calls, then a ragged call, a whole-block mix call, an f32 call with d_in2
    and a flush on the same batch, against the twin and the oracle"""
    mix = U.lim_mix(name, bps=bps)
    n = len(mix.calls3)
    entries = ["new"] * (n - 1) + ["f32"]
    routes = [U.RAG] * (n - 2) + [U.WHOLE_ROW, U.GENERIC]
    got, _ = U.check(mix, routes=routes, what=name, entries=entries)
    _, idle = U.lim_states(got[0]["state"])          # (the first call is quiet: LimState::n of an idle stream)
    for j in range(2, n):                            # behind the call that follows the peak, and from there on: not idle
        _, steps = U.lim_states(got[j]["state"])
        assert (steps < idle).all(), (name, "the limiter is idle behind call %d" % j, steps, idle)


# ---- 7. positions ----

@pytest.mark.parametrize("name", SHAPE_IDS)
def test_a_position_below_the_look_ahead_and_off_16_goes_to_the_general_kernel(name):
    """behind a call of 100 the streams stand at 100: below 240 and no multiple of 16.  Behind 1000 more: fused"""
    mix = shape(name, [(1, 100), (1, 900), (1, 0), (1, 0)], 1000)
    U.check(mix, routes=[U.RAG, U.GENERIC, U.RAG, U.RAG], what="positions")


# ---- 8. the switches ----

@pytest.mark.parametrize("name", SHAPE_IDS)
@pytest.mark.parametrize("switch", ["IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_FORCE_GENERIC"])
def test_each_switch_empties_the_familys_tally_and_leaves_the_pcm(name, switch):
    mix = shape(name, [(1, 0), (1, 0)], 1000)
    ref = U.render(mix)
    U.assert_tallies(mix, ref, [U.RAG, U.RAG], "no switch")
    with R.environment({switch: "1"}):
        got = U.render(mix)
    for r in got:
        assert r["fam"] == {} and r["other"] == {} and r["base"] == {R.gen(mix.m): 1}, (switch, r["fam"], r["base"], r["other"])
    U.assert_same(got, ref, switch)


# ---- 9. refusals ----

def test_refusals_are_the_twins_and_change_nothing():
    import torch
    import iac_amd as A
    mix = U.Mix(2, 4, 2, 1, [(1, 0)], 1000)
    d0, d1 = torch.from_numpy(mix.raw0).cuda(), torch.from_numpy(mix.raw1).cuda()
    pcm = torch.full((3, 1024 * 2 * 2), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def ins(first=(0, 0)):
        out = []
        for d, row, L, f in ((d0, mix.row0, mix.L0, first[0]), (d1, mix.row1, mix.L1, first[1])):
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.first_sample, inp.layout = d.data_ptr(), row, row, f, L
            out.append(inp)
        return out

    def args(**kw):
        a = A.RenderArgs()
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 1, pcm.data_ptr(), 1024 * 2 * 2, st
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def both(b, i, a, s0=0, n=3, reserved=None):
        """-> the two entries' return values on the same call"""
        out = []
        for name in ("iamf_hip_batch_render_packets_mix_ragged", "iamf_hip_batch_render_packets_mix"):
            call = A.PacketMixCall()
            call.in_[0], call.in_[1], call.args = i[0], i[1], a
            if reserved is not None:
                call.reserved[reserved] = 1
            out.append(getattr(A.lib(), name)(b.h if b is not None else None, C.byref(call), s0, n))
        torch.cuda.synchronize()
        assert bool((pcm == 0xA5).all())
        return out

    plain = A.Batch(3, mix.mx, 2, frame_size=1000)
    try:
        r = both(plain, ins(), args())                                   # a batch without a second element
        assert r[0] == r[1] == -1, r
    finally:
        plain.close()
    b = A.Batch(3, mix.mx, 2, frame_size=1000)
    b.set_second_element(mix.mx2, mix.eg2)
    try:
        sb = b.stream_state_bytes()

        def export():
            d_state = torch.zeros((3, sb), dtype=torch.uint8, device="cuda")
            b.export_range(0, 3, d_state.data_ptr(), sb, st)
            torch.cuda.synchronize()
            return d_state.cpu().numpy()

        before = export()
        for lib_name in ("iamf_hip_batch_render_packets_mix_ragged", "iamf_hip_batch_render_packets_mix"):
            assert getattr(A.lib(), lib_name)(b.h, None, 0, 3) == -1                      # a NULL call
        for w in range(4):
            r = both(b, ins(), args(), reserved=w)
            assert r[0] == r[1] == -1, (w, r)
        for i, a, rng in ((ins(), args(d_in=d0.data_ptr()), (0, 3)), (ins(), args(d_in2=d1.data_ptr()), (0, 3)),
                          (ins(first=(0, 4)), args(n_samples=100), (0, 3)), (ins(first=(4, 0)), args(n_samples=100), (0, 3)),
                          (ins(), args(), (0, 4)), (ins(), args(), (-1, 2)), (ins(), args(), (2, 0)),
                          (ins(), args(d_pcm=None), (0, 3)), (ins(), args(n_frames=-1), (0, 3)),
                          (ins(), args(n_samples=2000), (0, 3)), (ins(), args(pcm_stream_stride_bytes=64), (0, 3))):
            r = both(b, i, a, rng[0], rng[1])
            assert r[0] == r[1] and r[0] < 0, r
        assert np.array_equal(export(), before)
        U.reset_tallies(A)
        assert b.render_packets_mix_ragged(*ins(), args()) == 1000 - 240    # the batch stands where it stood: a first call
        fam, base, other = U.tallies(A)
        assert fam == {U.inst(2, 4, 2, 1): 1} and base == {} and other == {}, (fam, base, other)
    finally:
        b.close()
