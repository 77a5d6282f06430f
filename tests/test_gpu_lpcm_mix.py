"""-m gpu: both elements of a two-element mix as 16-bit LPCM packets (iamf_hip_batch_render_lpcm_mix; render_fast_kernel<..,
LP2>, iac_amd/csrc/iamf_render_lpcm_mix.hip and iamf_render_lpcm_mix_coupled.hip).

Every fused case asserts: the listing by family (iamf_hip_route_family_tally) names the instance, once per call; no table
and no other family shows a packet-fed row, and the base tally holds the flush's GENERIC row alone; every stream is bit for
bit the oracle's (route_cases_lpcm_mix.Mix.want: oracle_lib.render of each element from ints / 2^15, the frame gains, (0 +
y0) + y1, the output gain, limiter_run, pack), with PCM, n_emitted and the exported stream state equal to a twin batch run
through the same entry under IAMF_HIP_LPCM_UNFUSED=1 (two unpacks, then the f32 kernels).  Every case asserts from the
oracle that the programme drives the limiter: the mix above the threshold, bursts on both elements at different phases.
Tolerance 0 everywhere.  Shapes: 3-4 streams, frames of 1024 samples, calls of [1, 3, 2] frames.

The shapes that must stay unfused assert the family's tally empty and the same PCM."""
import numpy as np
import pytest

import route_cases as R
import route_cases_lpcm_mix as RM

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_NO_WIDE4", "IAMF_HIP_DENSE")
BAD_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


# ---- 1. every instance ----

@pytest.mark.parametrize("case", RM.CASES, ids=[c.id for c in RM.CASES])
def test_every_instance(case):
    case.build(case)


def test_the_second_elements_matrix_tells_its_channels_apart():
    """a second element whose L and R (or W, X, Y, Z) were swapped by the kernel must show: the seeded matrices give every
    (channel, slot) a weight of its own"""
    for m2 in (2, 4):
        for oc in (1, 2):
            mx2, _ = R.matrices(m2, oc, table=False, salt=1)
            w = np.ctypeslib.as_array(mx2.mat, shape=(m2 * oc,))
            assert len(set(np.abs(w).tolist())) == m2 * oc, (m2, oc)


# ---- 2. per-stream gains ----

@pytest.mark.parametrize("m,k", [(16, 2), (6, 1)])
def test_per_stream_gains_including_the_ones_the_reference_skips(m, k):
    """element, element-2 and output gain per stream: 1.0 (skipped), non-positive (skipped by the reference:
    IAMF_decoder.c:1383-1408 applies a gain only if it is positive and not 1) and ordinary ones, in every position"""
    mix = RM.Mix(m, 2, 2 if k == 2 else 4, "pair" if k == 2 else "mono", S=4,
                 eg=[1.0, -0.5, 0.9, 1.1], eg2=[0.0, 1.0, 1.3, 0.7], og=[0.85, 1.0, -1.0, 1.05])
    RM.check(mix, True, what="gains")


# ---- 3. ramps ----

@pytest.mark.parametrize("which", [("e0",), ("e1",), ("out",), ("e0", "e1", "out")], ids=["element", "element2", "output", "all"])
@pytest.mark.parametrize("m,k", [(9, 2), (12, 1)])
def test_a_ramp_on_each_gain_is_fused(m, k, which):
    mix = RM.Mix(m, 2, 2 if k == 2 else 1, "pair" if k == 2 else "mono")
    for j, w in enumerate(which):
        mix.ramp(w, j + 1)
    RM.check(mix, True, what="ramps %s" % (which,))      # (the family's tally, once per call: the ramped calls were fused)


# ---- 4. packet placement ----

@pytest.mark.parametrize("placement", ["own", "shared"])
@pytest.mark.parametrize("m,k,m2", [(16, 2, 2), (16, 1, 4), (12, 2, 2), (6, 1, 1)])
def test_packet_placement(m, k, m2, placement):
    """runs that are only 8-byte aligned (head 8, pad 8: the runs start at 8, 16 mod 16 in turn) with every byte between them
    0x7F / 0x80; element 1 in a buffer of its own, or in the same packet rows as element 0 (its runs behind element 0's, the
    same strides); the first and the last sample of every run at the extremes"""
    mix = RM.Mix(m, 2, m2, "pair" if k == 2 else "mono", head=(8, 24), pad=(8, 8), fill=True)
    offs = [mix.L1.src_offset[c] for c in range(m2)] + [mix.L0.src_offset[c] for c in range(m)]
    assert all(o % 2 == 0 for o in offs) and any(o % 16 == 8 for o in offs)
    RM.check(mix, True, what=placement, placement=placement)


def test_padded_strides_on_the_8_byte_grid():
    """element 1's rows 8 bytes longer than a multiple of 16: its frame stride is on the 8-byte grid only.  (Calls of two
    frames each: a call that began at an odd frame would find its packets 8 bytes off the 16-byte grid the buffer has to be
    on, and be unpacked.)"""
    mix = RM.Mix(4, 2, 2, "pair", calls=(2, 2, 2))
    mix.raw1 = np.concatenate([mix.raw1, np.full(mix.raw1.shape[:2] + (8,), 0x7F, dtype=np.uint8)], axis=2)
    mix.row1 += 8
    assert mix.row1 % 16 == 8
    RM.check(mix, True, what="stride 8 mod 16")


# ---- 5. trimmed starts ----

def test_a_trimmed_start_the_forms_take_is_fused():
    for m, k, m2 in ((16, 2, 2), (6, 1, 4)):
        mix = RM.Mix(m, 2, m2, "pair" if k == 2 else "mono", S=3, calls=(1,))
        RM.check(mix, True, what="first 64", first=64, n_samples=512)


@pytest.mark.parametrize("first,n_samples", [(3, 512), (64, 500)], ids=["odd_first", "n_not_64"])
def test_a_trimmed_start_the_forms_do_not_take_is_unpacked(first, n_samples):
    mix = RM.Mix(16, 2, 2, "pair", S=3, calls=(1,))
    general = {R.gen(16): 2} if n_samples % 64 else None        # no call of the vector kernels: the general one, and the flush
    RM.check(mix, False, what="first %d, %d samples" % (first, n_samples), first=first, n_samples=n_samples, unfused_base=general)


# ---- 6. shapes that stay unfused ----

@pytest.mark.parametrize("what,kw", [
    ("24-bit second element", dict(m=16, oc=2, m2=1, bps1=3)),
    ("big-endian second element", dict(m=16, oc=2, m2=1, le1=False)),
    ("stereo second element as two mono runs", dict(m=16, oc=2, m2=2, two_mono=True)),
    ("24-bit element 0", dict(m=16, oc=2, m2=2, form2="pair", bps0=3)),
    ("coupled 24-bit element 0", dict(m=6, oc=2, m2=1, bps0=3)),
], ids=["e1_24bit", "e1_big_endian", "e1_two_mono", "e0_24bit", "e0_coupled_24bit"])
def test_forms_that_are_unpacked(what, kw):
    RM.check(RM.Mix(**kw), False, what=what)


def test_six_output_channels_take_wide4_mix_behind_the_two_unpacks():
    mix = RM.Mix(12, 6, 2, "pair")
    RM.check(mix, False, what="six outputs", unfused_base={("WIDE4_MIX", 0, 12, 6, 0): 3, R.gen(12): 1})


def test_limiter_off_is_unpacked():
    mix = RM.Mix(16, 2, 2, "pair")
    RM.check(mix, False, what="limiter off", limiter=False, unfused_base={R.gen(16): 3})


# ---- 7. a range of streams ----

def test_a_range_of_streams_leaves_its_neighbours_alone():
    """[1, 3) of four streams: the neighbours' PCM rows keep their 0xA5 (gpu_util.rows_and_rest, in every call) and their
    exported state is what it was before the first call"""
    mix = RM.Mix(9, 2, 2, "pair", S=4)
    got, twin = RM.check(mix, True, what="range", rng_streams=(1, 2), prefill_state=True)
    for r in (got, twin):
        for s in (0, 3):
            assert r["pcm"][s].size == 0
            assert np.array_equal(r["state"][s], r["state0"][s]), ("stream %d was touched" % s)
        for s in (1, 2):
            assert not np.array_equal(r["state"][s], r["state0"][s])


# ---- 8. PCM formats ----

@pytest.mark.parametrize("bd,m,k", [(16, 1, 1), (24, 16, 2), (32, 10, 1), (-32, 4, 2)], ids=["s16", "s24", "s32", "f32"])
def test_pcm_formats(bd, m, k):
    mix = RM.Mix(m, 2, 2 if k == 2 else 4, "pair" if k == 2 else "mono")
    RM.check(mix, True, bd=bd, what="bd %d" % bd)


# ---- 9. fused, f32 and fused calls on one batch ----

@pytest.mark.parametrize("m,k", [(16, 2), (8, 1)])
def test_fused_and_f32_calls_interleave_on_one_batch(m, k):
    import iac_amd as A
    import test_gpu_programmes as TP
    mix = RM.Mix(m, 2, 2 if k == 2 else 1, "pair" if k == 2 else "mono")
    RM.reset_tallies(A)
    got = mix.render(steps=["mix", "f32", "mix"])
    fam, base, other = RM.tallies(A)
    assert fam == {mix.inst: 2} and other == {}, (fam, other)
    assert base == {("FAST", 1, m, 2, 0): 1, R.gen(m): 1}, base
    ref = mix.render(steps=["f32", "f32", "f32"])
    fam, base, other = RM.tallies(A)
    assert fam == {} and other == {} and base == {("FAST", 1, m, 2, 0): 3, R.gen(m): 1}, (fam, base, other)
    assert got["emitted"] == ref["emitted"] and np.array_equal(got["state"], ref["state"])
    for s in range(mix.S):
        want, pre, y0, y1 = mix.want(s)
        mix.assert_drives_the_limiter(s, pre, y0, y1)
        assert np.array_equal(got["pcm"][s], ref["pcm"][s]), "stream %d against the all-f32 run" % s
        assert TP.mismatch(RM.view(got["pcm"][s], 2, got["fmt"]), want) is None, "stream %d against the oracle" % s


# ---- 10. a caller-owned non-blocking stream ----

@pytest.mark.parametrize("where", ["NULL", "SAME"])
@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "grows_the_unpack_buffers"])
def test_on_a_stalled_non_blocking_stream(where, unfused):
    """The entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call: on the legacy null
    stream (the call must neither wait for it nor leave work there that its own stream needs) and on the call's own stream (the
    device cannot have started the call's work when it returns).  unfused: under IAMF_HIP_LPCM_UNFUSED=1 the first call
    allocates both unpack buffers and the second (three frames) grows both — the header's one exception to "asynchronous":
    such a call waits for its stream before it re-allocates, and zeroes the new buffer on that stream.  Whether a call had
    returned while the stall still ran is asserted for the call's own stream only, and in the steady state (the same calls
    have run once on another batch: no kernel is loaded in the call that is observed); under the null stream's stall it is
    printed — what is asserted there is the PCM."""
    import torch
    import iac_amd as A
    import stream_util as SU
    import test_gpu_programmes as TP
    mix = RM.Mix(16, 2, 2, "pair", calls=(1, 3, 2))
    with SU.side_stream() as side:
        h = side.cuda_stream

        def before_call(k, st):
            assert st == h
            SU.assert_non_blocking(st)
            ev = SU.stall(SU.torch_stream(0 if where == "NULL" else st))
            assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
            return lambda: not ev.query()

        with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"} if unfused else {}):
            mix.render(out_stream=h)
            RM.reset_tallies(A)
            got = mix.render(out_stream=h, before_call=before_call)
        fam, base, other = RM.tallies(A)
    running_after = got["notes"]
    print("still stalled on return (%s, %s): %s" % (where, "unfused" if unfused else "fused", running_after))
    assert fam == ({} if unfused else {mix.inst: 3}) and other == {}, (fam, other)
    if where == "SAME":   # the calls in which the buffers grow wait for their stream; every other call has returned before its work began
        assert running_after == ([False, False, True] if unfused else [True, True, True]), running_after
    for s in range(mix.S):
        want, pre, y0, y1 = mix.want(s)
        mix.assert_drives_the_limiter(s, pre, y0, y1)
        g = RM.view(got["pcm"][s], 2, got["fmt"])
        assert TP.mismatch(g, want) is None, ("stream %d against the oracle" % s, TP.mismatch(g, want))


# ---- refusals (a batch needs a device) ----

def test_refusals_leave_the_batch_and_the_pcm_untouched():
    """with a device, since a batch cannot be created without one: every refusal the entry documents, each with a sentinel in
    the PCM rows, and the stream position as it was (a whole-frame call behind them emits what a first call emits)"""
    import torch
    import iac_amd as A
    mix = RM.Mix(4, 2, 1, S=3, calls=(1,))
    d0, d1 = torch.from_numpy(mix.raw0).cuda(), torch.from_numpy(mix.raw1).cuda()
    pcm = torch.full((3, 1024 * 2 * 2), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def ins(first=(0, 0), raw=(True, True)):
        out = []
        for d, row, L, f, r in ((d0, mix.row0, mix.L0, first[0], raw[0]), (d1, mix.row1, mix.L1, first[1], raw[1])):
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.first_sample, inp.layout = (d.data_ptr() if r else None), row, row, f, L
            out.append(inp)
        return out

    def args(**kw):
        a = A.RenderArgs()
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 1, pcm.data_ptr(), 1024 * 2 * 2, st
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(b, i, a, s0=None, n=None, code=BAD_ARG):
        with pytest.raises(A.IamfHipError) as e:
            b.render_lpcm_mix(i[0], i[1], a, s0, n)
        assert e.value.code == code, e.value.code
        torch.cuda.synchronize()
        assert bool((pcm == 0xA5).all())

    plain = A.Batch(3, mix.mx, 2, frame_size=1024)
    refused(plain, ins(), args())                                    # a batch without a second element
    plain.close()
    b = A.Batch(3, mix.mx, 2, frame_size=1024)
    b.set_second_element(mix.mx2, mix.eg2)
    try:
        refused(b, ins(), args(d_in=d0.data_ptr()))
        refused(b, ins(), args(d_in2=d1.data_ptr()))
        refused(b, ins(raw=(False, True)), args())
        refused(b, ins(raw=(True, False)), args())
        refused(b, ins(first=(0, 64)), args(n_samples=512))
        refused(b, ins(first=(64, 0)), args(n_samples=512))
        refused(b, ins(), args(), 0, 4)                              # a bad range
        refused(b, ins(), args(), -1, 2)
        refused(b, ins(), args(), 2, 0)
        refused(b, ins(), args(d_pcm=None))
        refused(b, ins(), args(n_frames=-1))
        refused(b, ins(), args(n_frames=1, n_samples=2048))          # what range_args_check refuses: before the first unpack launch
        refused(b, ins(), args(d_element_ramp=d0.data_ptr(), ramp_stream_stride=8))
        refused(b, ins(), args(pcm_stream_stride_bytes=64), code=-2)   # IAMF_HIP_ERR_BUFFER_TOO_SMALL
        assert A.route_family_tally("LPCM_MIX", reset=True) == {}
        assert b.render_lpcm_mix(*ins(), args()) == 1024 - 240       # the batch stands where it stood: a first call
    finally:
        b.close()
