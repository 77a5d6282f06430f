"""iamf_hip_batch_render_packets_nolim on the GPU: every case runs the new entry on one batch and
iamf_hip_batch_render_packets_ragged on a twin (nolim_packets_util.check) and requires byte-equal PCM rows with every byte
outside the emitted run still the fill pattern, equal return values and refusal codes, equal exported stream state, the
family's tally exactly {instance: 1} per fused call with every other table empty (for a call that falls through: the family's
tally empty and the twin's rows in every other table), the family's tally empty on the twin, and every stream equal to the
oracle of a limiter-less stream on the packets' integer grid."""
import numpy as np
import pytest

import nolim_packets_util as U
import packets_ragged_util as PU

pytestmark = pytest.mark.gpu

EVERY_INSTANCE = list(U.INSTANCES)       # (tests/test_nolim_packets_cpu.py: exactly the family's listing)
TWO = [(1, 0), (1, 0)]


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

@pytest.mark.parametrize("form", sorted(U.FORMS))
def test_every_instance(form):
    """two calls of one frame of 1000, three streams, stereo f32: the instance's row once per call"""
    def one(what, m):
        U.check(form, m, 2, 1000, PU.hot_ints(form, m, 2000), TWO, what=what)
    each_case([("%s %d" % (f, m), m) for f, m in EVERY_INSTANCE if f == form], one)


def test_pcm_formats():
    """s16, s24, s32 and f32 on a mono-coded and a coupled instance, four output channels (8, 12, 16, 16 bytes per sample-frame);
    stereo s24 is 6 bytes, no whole dwords: the twin's route"""
    def one(what, form, m, oc, bd, fused):
        U.check(form, m, oc, 1000, PU.hot_ints(form, m, 2000), TWO, bd=bd, fused=fused, what=what)
    cases = [("%s %d -> 4 x %d" % (f, m, bd), f, m, 4, bd, True) for f, m in (("s24", 9), ("s16c", 6)) for bd in (16, 24, 32, -32)]
    each_case(cases + [("s16c 6 -> stereo s24", "s16c", 6, 2, 24, False)], one)


# ---- gains ----

def test_gains_and_loudness():
    """per stream the gains 1.0, 0.8 and (element gain 0, output gain -1: the branches a non-positive gain skips); loudness off
    and on (1.0, 0.7, 1.3), into s16 and f32"""
    assert U.EG == [1.0, 0.8, 0.0] and U.OG == [1.0, 0.8, -1.0]

    def one(what, form, m, bd, lg):
        U.check(form, m, 2, 1000, PU.hot_ints(form, m, 2000), TWO, bd=bd, lg=lg, what=what)
    each_case([("%s %d, bd %d, loudness %s" % (f, m, bd, lg), f, m, bd, lg) for f, m in (("s16", 16), ("s24c", 12)) for bd in (16, -32)
               for lg in (None, U.LG)], one)


# ---- lengths ----

def test_lengths():
    """frame size 2048: calls of 4 (one quad), 8, 1020 / 1024 / 1028 (the chunk boundary on both sides; 1028 leaves a last
    chunk of one quad) and 2044; three frames of 100 per call (lanes of one chunk in three frames); eleven and twelve frames of
    100 (chunk 2 begins mid-frame, at sample 24 of frame 10)"""
    def one(what, form, m, fs, calls):
        U.check(form, m, 2, fs, PU.hot_ints(form, m, sum(PU.samples(fs, c[:2]) for c in calls)), calls, what=what)
    lengths = [(1, n) for n in (4, 8, 1020, 1024, 1028, 2044)]
    each_case([("lengths s16", "s16", 4, 2048, lengths), ("lengths s24c", "s24c", 6, 2048, lengths), ("3 x 100, s24", "s24", 9, 100, [(3, 0)] * 2),
               ("3 x 100, s16c", "s16c", 8, 100, [(3, 0)] * 2), ("11 x 100, s16", "s16", 16, 100, [(11, 0)]), ("11 x 100, s24c", "s24c", 2, 100, [(11, 0)]),
               ("12 x 100, s16c: 1200 = 1024 + 176", "s16c", 10, 100, [(12, 0)])], one)


# ---- trimmed starts ----

def test_trimmed_starts():
    """first_sample 4, 100 and 240 with n_samples = fs - first, and first_sample 2 on a coupled stereo pair (996 samples); every
    byte that is no sample of the call filled with 0xFF and then with 0x00: the PCM is the same, and the oracle's"""
    def one(what, form, m, first, n):
        ints = PU.hot_ints(form, m, n + 1000)
        calls = [(1, n, first), (1, 0)]
        a, _ = U.check(form, m, 2, 1000, ints, calls, fill=0xFF, what=what + ", fill 0xFF")
        b, _ = U.check(form, m, 2, 1000, ints, calls, fill=0x00, what=what + ", fill 0x00", oracle=False)
        U.assert_same(a, b, what + ": the two fills")
    cases = [("%s %d, first %d" % (f, m, first), f, m, first, 1000 - first) for f, m in (("s16", 4), ("s24", 16), ("s16c", 6), ("s24c", 12))
             for first in (4, 100, 240)]
    cases += [("%s stereo pair, first 2" % f, f, 2, 2, 996) for f in ("s16c", "s24c")]
    each_case(cases, one)


def test_a_trim_the_form_does_not_take_is_the_twins():
    """first_sample 2 on mono runs (4 bytes off the 16-bit grid; 6 bytes, off the dword grid, for 24 bit) and an odd first sample
    on a coupled pair"""
    def one(what, form, m, first, n):
        U.check(form, m, 2, 1000, PU.hot_ints(form, m, n), [(1, n, first)], fused=False, what=what)
    each_case([("s16 4, first 2", "s16", 4, 2, 996), ("s24 4, first 2", "s24", 4, 2, 996), ("s16c 2, first 1", "s16c", 2, 1, 996)], one)


# ---- output widths ----

def test_output_widths():
    """1 (f32), 2, 6, 12 and 15 channels fused; 16 channels of f32 (64 bytes: past the tile) and mono s16 (2 bytes: no whole
    dword) take the twin's route"""
    def one(what, oc, bd, fused):
        U.check("s16", 4, oc, 1000, PU.hot_ints("s16", 4, 2000), TWO, bd=bd, fused=fused, what=what)
    each_case([("mono f32", 1, -32, True), ("stereo s16", 2, 16, True), ("6 x s16", 6, 16, True), ("12 x s32", 12, 32, True), ("15 x f32", 15, -32, True),
               ("12 x s24", 12, 24, True), ("16 x f32", 16, -32, False), ("mono s16", 1, 16, False)], one)


# ---- fall-through ----

def test_fall_through():
    """a limiter-on batch, a batch with a second element, n_samples 1001 / 1002 / 1003, frame size 6, big-endian samples,
    mono-coded 6 channels (16 and 24 bit), IAMF_HIP_NOLIM_PACKETS_UNFUSED=1: bit-equal PCM and codes, the family's tally empty,
    the twin's rows everywhere else"""
    import route_cases as R

    def one(what, form, m, fs, calls, kw, env):
        n = sum(PU.samples(fs, c[:2]) for c in calls)
        with R.environment(env):
            got, ref = U.check(form, m, 2, fs, PU.hot_ints(form, m, n), calls, fused=False, what=what, **kw)
        return got, ref

    each_case([("limiter on", "s16", 4, 1000, TWO, dict(limiter=True, bd=16), {}),
               ("a second element", "s16", 4, 1000, TWO, dict(second=R.matrices(2, 2, table=False)[0]), {}),
               ("1001 / 1002 / 1003", "s24", 9, 2048, [(1, 1001), (1, 1002), (1, 1003)], {}, {}),
               ("frame size 6", "s16", 4, 6, [(2, 0)], dict(oracle=False), {}),      # (no multiple of 4: both entries refuse it, with one code)
               ("big-endian", "s16", 4, 1000, TWO, dict(le=False), {}),
               ("big-endian 24 bit coupled", "s24c", 6, 1000, TWO, dict(le=False), {}),
               ("mono-coded 6 channels, 16 bit", "s16", 6, 1000, TWO, {}, {}),
               ("mono-coded 6 channels, 24 bit", "s24", 6, 1000, TWO, {}, {}),
               ("IAMF_HIP_NOLIM_PACKETS_UNFUSED", "s16c", 12, 1000, TWO, {}, {"IAMF_HIP_NOLIM_PACKETS_UNFUSED": "1"}),
               ("IAMF_HIP_LPCM_UNFUSED", "s16", 16, 1000, TWO, {}, {"IAMF_HIP_LPCM_UNFUSED": "1"}),
               ("IAMF_HIP_FORCE_GENERIC", "s24", 4, 1000, TWO, {}, {"IAMF_HIP_FORCE_GENERIC": "1"})], one)


def test_the_fall_through_of_a_plain_call_is_the_f32_limiterless_kernel():
    """what the switch sends a fused call to: the unpacker, then render_nolim_kernel<M> — one NOLIM row in the base table"""
    import route_cases as R
    with R.environment({"IAMF_HIP_NOLIM_PACKETS_UNFUSED": "1"}):
        got, ref = U.check("s16", 16, 2, 1000, PU.hot_ints("s16", 16, 1000), [(1, 0)], fused=False)
    assert got[0]["base"] == ref[0]["base"] == {U.nolim_f32(16): 1} and got[0]["rest"] == {}


# ---- placements ----

def test_placements():
    """gpu_util.place_packets: PK_PAD16, PK_GRID (fused), PK_OFF_BASE, PK_OFF_STRIDE (the unfused path) and PK_FAR_STREAMS
    (streams 2^31 + 16 bytes apart: the kernel's 64-bit addresses) on one instance of each form"""
    import gpu_util as G

    def one(what, form, m, pk):
        bps = U.FORMS[form][0]
        off, fst, sst = G.packet_geometry(pk, U.S, 1, 16, bps)
        g = G.pk_grid(bps)
        fused = off % 16 == 0 and (fst - 16) % g == 0 and sst % g == 0      # (fst = the row + what the placement adds: rows are multiples of 16)
        assert fused == (pk in (G.PK_PAD16, G.PK_GRID, G.PK_FAR_STREAMS)), (pk, off, fst, sst)
        U.check(form, m, 2, 1000, PU.hot_ints(form, m, 2000), TWO, fused=fused, packets=pk, what=what)
    each_case([("%s %d, %s" % (f, m, pk), f, m, pk) for f, m in PU.PLACED
               for pk in (G.PK_PAD16, G.PK_GRID, G.PK_OFF_BASE, G.PK_OFF_STRIDE, G.PK_FAR_STREAMS)], one)


# ---- ranges and streams ----

def test_a_range_call_leaves_the_other_streams_rows_alone():
    """stream0 = 1, two of four streams (rows_and_rest asserts the rows outside the range untouched)"""
    for form, m in (("s16", 9), ("s24c", 8)):
        ints = PU.hot_ints(form, m, 2000, streams=4)
        got, _ = U.check(form, m, 2, 1000, ints, TWO, rng=(1, 2), what="range, " + form)
        assert all(len(r["pcm"][s]) == 0 for r in got for s in (0, 3)) and all(len(r["pcm"][s]) == 1000 * 2 * 4 for r in got for s in (1, 2))


def test_on_a_stalled_non_blocking_stream():
    """the entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call on the call's own
    stream: the call returns while the stall still runs, and renders the same"""
    import interleaved_util as IU
    import stream_util as SU
    import test_gpu_programmes as TP
    form, m, oc, fs = "s16c", 6, 2, 1000
    amx, omx = IU.dense_matrices(m, oc)
    ints = PU.hot_ints(form, m, 2000)
    with SU.side_stream() as side:
        h = side.cuda_stream

        def before_call(k, st):
            assert st == h
            SU.assert_non_blocking(st)
            ev = SU.stall(SU.torch_stream(st))
            assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
            return lambda: not ev.query()

        U.drive("nolim", amx, form, oc, fs, ints, TWO, out_stream=h, export=False)      # (the kernels are loaded)
        got = U.drive("nolim", amx, form, oc, fs, ints, TWO, out_stream=h, before_call=before_call, export=False)
        ref = U.drive("ragged", amx, form, oc, fs, ints, TWO, out_stream=h, export=False)
    assert [r["note"] for r in got] == [True, True], [r["note"] for r in got]
    assert all(r["fam"] == {U.inst(form, m): 1} and r["base"] == {} and r["rest"] == {} for r in got) and all(r["fam"] == {} for r in ref)
    U.assert_same(got, ref, "stalled")
    for s in range(U.S):
        w = U.want(omx, oc, ints[s], 2, -32, U.EG[s], U.OG[s])
        assert TP.mismatch(U.stream_pcm(got, s, oc, -32), w) is None, "stream %d against the oracle" % s


# ---- refusals ----

def test_refusals_are_the_siblings():
    """a NULL call, a non-zero reserved word and a non-NULL d_in: the sibling's codes, nothing written, nothing launched, the
    stream state as it was"""
    import interleaved_util as IU

    def null(call):
        return None

    def reserved(call):
        call.reserved[2] = 7
        return call

    def d_in(call):
        call.args.d_in = call.in_.d_raw
        return call

    amx, _ = IU.dense_matrices(4, 2)
    ints = PU.hot_ints("s16", 4, 1000)
    for what, edit in (("NULL call", null), ("reserved", reserved), ("d_in", d_in)):
        got = U.drive("nolim", amx, "s16", 2, 1000, ints, [(1, 0)], raw_call=edit)
        ref = U.drive("ragged", amx, "s16", 2, 1000, ints, [(1, 0)], raw_call=edit)
        assert got[0]["err"] == ref[0]["err"] == -1 and got[0]["ret"] == 0, (what, got[0]["err"], ref[0]["err"])
        assert got[0]["fam"] == {} and got[0]["base"] == {} and got[0]["rest"] == {}, what
        U.assert_same(got, ref, what)
    plain = U.drive("nolim", amx, "s16", 2, 1000, ints, [(1, 0)])
    assert plain[0]["err"] is None and plain[0]["ret"] == 1000
    assert plain[0]["state"][1] != got[0]["state"][1] or not np.array_equal(plain[0]["state"][0], got[0]["state"][0])      # (a call that ran moves the stream)
