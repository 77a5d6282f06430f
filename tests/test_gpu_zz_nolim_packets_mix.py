"""iamf_hip_batch_render_packets_mix_nolim on the GPU: every case runs the new entry on one batch and
iamf_hip_batch_render_packets_mix_ragged on a twin (nolim_packets_mix_util.check) and requires, call by call, equal return values
and refusal codes, byte-equal PCM rows with every byte outside the emitted run still the fill pattern, equal exported stream
state, the family's tally exactly {instance: 1} per fused call with every other table empty (for a call that falls through: the
family's tally empty and the twin's rows in every other table) and the family's tally empty on the twin; then every stream equal,
bit for bit, to the oracle of a limiter-less two-element stream on the packets' integer grid.  Three streams, per-stream gains
(1.0, 0.8, 0 / -1) and an element-2 gain per stream (1.0, 0.8, 0.0).

Two lists of the issue cannot be had as it words them, because a call is whole frames or ONE trimmed frame: "one call of 1028
samples as 1 frame + a trimmed frame of 4" and the lengths 1028 and 2052 at frame sizes of 8 to 1024.  The instances therefore
run a frame of 1024, a trimmed frame of 4 and a call of two frames (two chunks, the chunk boundary on a frame boundary); the
lengths 4, 1020, 1024, 1028 and 2052 run as calls of whole frames of 4 samples (a frame boundary between any two quads), and the
frame sizes 8, 240, 1000 and 1024 with calls that cross a chunk boundary in one call."""
import numpy as np
import pytest

import nolim_packets_mix_util as U

pytestmark = pytest.mark.gpu

EVERY_INSTANCE = list(U.INSTANCES)       # (tests/test_nolim_packets_mix_cpu.py: exactly the family's listing)
TWO = [(1, 0), (1, 0)]
# the shapes of the length, trim, ramp and switch tests: 3rd order + coupled stereo in 16 bit, 5.1 coupled + mono in 24
SHAPES = {"toa_stereo_16": (2, 16, 2), "l51_mono_24": (3, 6, 1)}


def each_case(cases, fn):
    """fn(*case) for every case; an assertion that fails is kept and the next case runs; at the end the test fails with all of
    them.  (Any other exception — a HIP error — ends the test at once.)"""
    failed = []
    for case in cases:
        try:
            fn(*case)
        except AssertionError as e:
            failed.append("%r: %s" % (case[0], e))
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(cases), "\n".join(failed))


# ---- instances and formats ----

@pytest.mark.parametrize("bps", (2, 3))
def test_every_instance(bps):
    """a frame of 1024, a trimmed frame of 4 and two frames in one call (two chunks), into stereo f32: the instance's row once per call"""
    def one(what, m, k):
        U.check(U.Mix(bps, m, 2, k, [(1, 0), (1, 4), (2, 0)], 1024), what=what)
    each_case([("%d bit, m %d, LP2 %d" % (8 * b, m, k), m, k) for b, m, k in EVERY_INSTANCE if b == bps], one)


def test_pcm_formats():
    """s16, s24, s32 and f32 on both shapes, four output channels (8, 12, 16, 16 bytes per sample-frame)"""
    def one(what, shape, bd):
        bps, m, k = SHAPES[shape]
        U.check(U.Mix(bps, m, 4, k, TWO, 1000), bd=bd, what=what)
    each_case([("%s -> 4 x %d" % (sh, bd), sh, bd) for sh in sorted(SHAPES) for bd in (16, 24, 32, -32)], one)


def test_output_widths():
    """1 channel f32, stereo s16, 5.1 s16 and 15 channels f32 (60 bytes) fused; mono s16 (2 bytes: no whole dword) and 16 channels
    of f32 (64 bytes: past the tile) take the twin's route"""
    def one(what, oc, bd, fused):
        U.check(U.Mix(2, 4, oc, 2, TWO, 1000), bd=bd, fused=fused, what=what)
    each_case([("mono f32", 1, -32, True), ("stereo s16", 2, 16, True), ("5.1 s16", 6, 16, True), ("15 x f32", 15, -32, True),
               ("mono s16", 1, 16, False), ("16 x f32", 16, -32, False)], one)


def test_a_silent_slot_and_a_slot_only_element_1_feeds():
    """element 0 through an ambisonics matrix whose slot 3 is the LFE (no generator on the batch: src_feed[3] < 0), element 1
    through a dense matrix that feeds every slot, slot 3 included; and element 1 through such a matrix too (slot 3 silent)"""
    import iac_amd as A
    import route_cases as R
    import test_gpu_programmes as TP

    def one(what, second_lfe):
        h2m = TP.selection(4, 6, kind=A.KIND_H2M, channels=6, lfe1=3)
        m2 = TP.selection(4, 6, kind=A.KIND_H2M, channels=6, lfe1=3) if second_lfe else R.matrices(4, 6, table=False, salt=1)
        mix = U.Mix(2, 4, 6, 1, TWO, 1000, mats=(h2m, m2))
        got, _ = U.check(mix, what=what)
        for s in range(U.S):
            slot3 = U.stream_pcm(got, s, 6, -32)[:, 3]
            assert bool(np.any(slot3 != 0)) == (not second_lfe), (what, s)      # (a gain of 0 is skipped, as in the reference: element 1 sounds)
    each_case([("slot 3: element 1 alone", False), ("slot 3: silent", True)], one)


# ---- gains, ramps, loudness ----

def test_loudness():
    """loudness on (1.0, 0.7, 1.3) into s16 and f32, both shapes"""
    def one(what, shape, bd):
        bps, m, k = SHAPES[shape]
        U.check(U.Mix(bps, m, 2, k, TWO, 1000), bd=bd, lg=U.LG, what=what)
    each_case([("%s, bd %d" % (sh, bd), sh, bd) for sh in sorted(SHAPES) for bd in (16, -32)], one)


def test_ramps():
    """each of the three ramps alone and all three, rows from ramp_rows(): NaN between the rows, the allocation ending at the last
    row's last float.  Lengths 1000 and 1028 / 4 (a last chunk and a call of one quad: the last float4 ends the allocation)"""
    def one(what, shape, which, calls, fs):
        bps, m, k = SHAPES[shape]
        mix = U.Mix(bps, m, 2, k, calls, fs)
        for seed, w in enumerate(which):
            mix.ramp(w, seed + 1)
        U.check(mix, what=what)
    sets = (("e0",), ("e1",), ("out",), ("e0", "e1", "out"))
    cases = [("%s, ramps %s" % (sh, "+".join(w)), sh, w, TWO, 1000) for sh in sorted(SHAPES) for w in sets]
    cases += [("%s, all ramps, 257 / 1 frames of 4" % sh, sh, sets[3], [(257, 0), (1, 0)], 4) for sh in sorted(SHAPES)]
    each_case(cases, one)


def test_a_ramp_the_form_does_not_take_is_the_twins():
    """a ramp row shifted by 1 float (off the 16-byte grid) and a stride of 4k + 1"""
    def one(what, which, kw):
        mix = U.Mix(2, 16, 2, 2, TWO, 1000)
        mix.ramp(which, 3)
        U.check(mix, fused=False, what=what, **kw)
    each_case([("%s shifted by 1 float" % w, w, dict(ramp_shift={w: 1})) for w in ("e0", "e1", "out")] +
              [("%s, stride 4k + 1" % w, w, dict(ramp_stride_extra=1)) for w in ("e0", "e1", "out")], one)


# ---- lengths ----

def test_lengths():
    """calls of 4, 1020, 1024, 1028 and 2052 samples (one quad; the chunk boundary on both sides; a last chunk of one quad; two
    chunks and a quad) as whole frames of 4 samples"""
    def one(what, shape):
        bps, m, k = SHAPES[shape]
        U.check(U.Mix(bps, m, 2, k, [(n // 4, 0) for n in (4, 1020, 1024, 1028, 2052)], 4), what=what)
    each_case([(sh, sh) for sh in sorted(SHAPES)], one)


def test_frame_sizes():
    """frame sizes 8, 240, 1000 and 1024: a call of one frame, and one that crosses the chunk boundary (129 x 8 = 1032, 5 x 240 =
    1200, 2 x 1000, 2 x 1024: lanes of one chunk in several frames, chunk 2 beginning mid-frame)"""
    def one(what, shape, fs, calls):
        bps, m, k = SHAPES[shape]
        U.check(U.Mix(bps, m, 2, k, calls, fs), what=what)
    each_case([("%s, fs %d" % (sh, fs), sh, fs, [(1, 0), (nf, 0)]) for sh in sorted(SHAPES) for fs, nf in ((8, 129), (240, 5), (1000, 2), (1024, 2))], one)


# ---- trimmed starts ----

def test_trimmed_starts():
    """first_sample 4 and fs - 4 (n_samples = fs - first: 1020 and 4), every byte of the packets that belongs to no run filled
    with 0x7F / 0x80"""
    def one(what, shape, first):
        bps, m, k = SHAPES[shape]
        U.check(U.Mix(bps, m, 2, k, [(1, 1024 - first, first), (1, 0)], 1024, fill=True), what=what)
    each_case([("%s, first %d" % (sh, first), sh, first) for sh in sorted(SHAPES) for first in (4, 1020)], one)


def test_a_trim_the_form_does_not_take_is_the_twins():
    """first_sample 2 (n_samples 1020: the runs start off the grid, and the f32 path takes the call)"""
    def one(what, shape):
        bps, m, k = SHAPES[shape]
        U.check(U.Mix(bps, m, 2, k, [(1, 1020, 2)], 1024), fused=False, what=what)
    each_case([(sh, sh) for sh in sorted(SHAPES)], one)


# ---- fall-through ----

def test_fall_through():
    """a limiter-on batch, a 16-bit bed beside a 24-bit second element, big-endian samples (either element), a stereo second
    element held as two mono runs, and each off-switch: bit-equal PCM and codes, the family's tally empty, the twin's rows
    everywhere else"""
    import route_cases as R

    def one(what, mixkw, kw, env):
        args = dict(bps=2, m=16, oc=2, k=2)
        args.update(mixkw.pop("shape", {}))
        with R.environment(env):
            U.check(U.Mix(args["bps"], args["m"], args["oc"], args["k"], TWO, 1000, **mixkw), fused=False, what=what, **kw)

    each_case([("limiter on", {}, dict(limiter=True, bd=16), {}),
               ("16-bit bed + 24-bit second", dict(bps1=3), {}, {}),
               ("big-endian bed", dict(le0=False), {}, {}),
               ("big-endian second", dict(le1=False), {}, {}),
               ("big-endian, 24 bit, both", dict(shape=dict(bps=3, m=6, k=1), le0=False, le1=False), {}, {}),
               ("a stereo second as two mono runs", dict(two_mono=True), {}, {}),
               ("IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED", {}, {}, {"IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED": "1"}),
               ("IAMF_HIP_LPCM_UNFUSED", {}, {}, {"IAMF_HIP_LPCM_UNFUSED": "1"}),
               ("IAMF_HIP_FORCE_GENERIC", dict(shape=dict(bps=3, m=6, k=1)), {}, {"IAMF_HIP_FORCE_GENERIC": "1"})], one)


def test_the_fall_through_of_a_plain_call_is_two_unpackers_and_the_general_kernel():
    """what the switch sends a fused call to: one GENERIC row in the base table, no packet-fed row anywhere"""
    import route_cases as R
    with R.environment({"IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED": "1"}):
        got, ref = U.check(U.Mix(2, 16, 2, 2, [(1, 0)], 1000), fused=False)
    assert got[0]["base"] == ref[0]["base"] == {R.gen(16): 1} and got[0]["rest"] == {}


def test_a_batch_without_a_second_element_is_refused_with_the_twins_code():
    got, ref = U.check(U.Mix(2, 16, 2, 2, [(1, 0)], 1000), fused=False, second=False)
    assert got[0]["err"] == ref[0]["err"] == -1 and got[0]["ret"] == 0 and got[0]["base"] == {} and got[0]["rest"] == {}


# ---- placements ----

def test_placements():
    """gpu_util.place_packets on each element separately: PK_PAD16 and PK_GRID fused, PK_OFF_BASE (the buffer 8 bytes off the
    16-byte grid) the twin's route; PK_FAR_STREAMS (streams 2^31 + 16 bytes apart: the kernel's 64-bit addresses) once, on element 1"""
    import gpu_util as G

    def one(what, shape, el, pk):
        bps, m, k = SHAPES[shape]
        packets = (pk, None) if el == 0 else (None, pk)
        U.check(U.Mix(bps, m, 2, k, TWO, 1000), fused=pk != G.PK_OFF_BASE, packets=packets, what=what)
    cases = [("%s, element %d, %s" % (sh, el, pk), sh, el, pk) for sh in sorted(SHAPES) for el in (0, 1)
             for pk in (G.PK_PAD16, G.PK_GRID, G.PK_OFF_BASE)]
    each_case(cases + [("toa_stereo_16, element 1, far streams", "toa_stereo_16", 1, G.PK_FAR_STREAMS)], one)


# ---- ranges and streams ----

def test_a_range_call_leaves_the_other_streams_rows_alone():
    """stream0 = 1, one of three streams (rows_and_rest asserts the rows outside the range untouched)"""
    for sh in sorted(SHAPES):
        bps, m, k = SHAPES[sh]
        got, _ = U.check(U.Mix(bps, m, 2, k, TWO, 1000), rng=(1, 1), what="range, " + sh)
        assert all(len(r["pcm"][s]) == 0 for r in got for s in (0, 2)) and all(len(r["pcm"][1]) == 1000 * 2 * 4 for r in got)


def test_on_a_stalled_non_blocking_stream():
    """the entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call on the call's own
    stream: the call returns while the stall still runs, and renders the same"""
    import stream_util as SU
    import test_gpu_programmes as TP
    mix = U.Mix(2, 6, 2, 2, TWO, 1000).ramp("e1", 2)
    with SU.side_stream() as side:
        h = side.cuda_stream

        def before_call(k, st):
            assert st == h
            SU.assert_non_blocking(st)
            ev = SU.stall(SU.torch_stream(st))
            assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
            return lambda: not ev.query()

        U.drive("nolim", mix, out_stream=h, export=False)      # (the kernels are loaded)
        got = U.drive("nolim", mix, out_stream=h, before_call=before_call, export=False)
        ref = U.drive("ragged", mix, out_stream=h, export=False)
    assert [r["note"] for r in got] == [True, True], [r["note"] for r in got]
    assert all(r["fam"] == {mix.nl_inst: 1} and r["base"] == {} and r["rest"] == {} for r in got) and all(r["fam"] == {} for r in ref)
    U.assert_same(got, ref, "stalled")
    for s in range(U.S):
        assert TP.mismatch(U.stream_pcm(got, s, 2, -32), U.want(mix, s)) is None, "stream %d against the oracle" % s


# ---- refusals ----

def test_refusals_are_the_twins():
    """a NULL call, a non-zero reserved word, a non-NULL d_in and d_in2, first samples that differ: the twin's codes, nothing
    written, nothing launched, the stream state as it was"""
    def null(call):
        return None

    def reserved(call):
        call.reserved[2] = 7
        return call

    def d_in(call):
        call.args.d_in = call.in_[0].d_raw
        return call

    def d_in2(call):
        call.args.d_in2 = call.in_[1].d_raw
        return call

    def firsts(call):
        call.in_[1].first_sample = 4
        return call

    mix = U.Mix(2, 4, 2, 1, [(1, 0)], 1000)
    for what, edit in (("NULL call", null), ("reserved", reserved), ("d_in", d_in), ("d_in2", d_in2), ("first samples differ", firsts)):
        got = U.drive("nolim", mix, raw_call=edit)
        ref = U.drive("ragged", mix, raw_call=edit)
        assert got[0]["err"] == ref[0]["err"] == -1 and got[0]["ret"] == 0, (what, got[0]["err"], ref[0]["err"])
        assert got[0]["fam"] == {} and got[0]["base"] == {} and got[0]["rest"] == {}, what
        U.assert_same(got, ref, what)
    plain = U.drive("nolim", mix)
    assert plain[0]["err"] is None and plain[0]["ret"] == 1000
    assert plain[0]["state"][1] != got[0]["state"][1] or not np.array_equal(plain[0]["state"][0], got[0]["state"][0])      # (a call that ran moves the stream)
