"""-m gpu: both elements of a two-element mix as 24-bit LPCM packets (iamf_hip_batch_render_packets_mix; render_fast_kernel<..,
LP, true, 3, LPC, LP2>, iac_amd/csrc/iamf_render_lpcm24_mix.hip and iamf_render_lpcm24_mix_coupled.hip).

The programme, the packet rows and the oracle are route_cases_lpcm_mix.Mix's with bps0 = bps1 = 3 (24-bit rows, low bytes
populated; oracle_lib.render of each element from ints / 2^23, the frame gains, (0 + y0) + y1, the output gain, limiter_run,
pack); the render loop and the checks are this file's, since Mix.render calls the 16-bit entry.

Every fused case asserts: the listing by family names the instance (LPCM24_MIX, 0, m, oc, LP2), once per call; no table and
no other packet-fed family shows a row, and the base tally holds the flush's GENERIC row alone; every stream is bit for bit
the oracle's, with PCM, n_emitted and the exported stream state equal to a twin batch run through the same entry under
IAMF_HIP_LPCM_UNFUSED=1 (two unpacks, then the f32 kernels); every byte of the PCM rows outside the emitted runs is still 0xA5
(gpu_util.rows_and_rest).  Every case asserts from the oracle that the programme drives the limiter.  Tolerance 0.
Shapes: 3-4 streams, frames of 1024 samples, calls of [1, 3, 2] frames — a first chunk without a predecessor, chunk-to-chunk
prefetch and a flush.  The shapes that must stay unfused assert the family's tally empty and the same PCM.

The name sorts the file behind the existing GPU files, whose order in a run stays as it was."""
import numpy as np
import pytest

import route_cases as R
import route_cases_lpcm_mix as RM

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_NO_WIDE4", "IAMF_HIP_DENSE")
FAM = "LPCM24_MIX"
OTHER_FAMILIES = ("LPCM_COUPLED", "LPCM_MIX", "LPCM24_COUPLED")     # the packet-fed families listed by family only
PACKET_FED = ("LPCM", "LPCM24", "LPCM_COUPLED", "LPCM24_COUPLED", "FANOUT_LPCM", "LPCM_MIX", FAM)
INSTANCES = [(m, oc, k) for m in RM.LPCM_M + RM.COUPLED_M for oc in RM.MIX_OC for k in RM.MIX_K]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def inst(m, oc, k):
    return (FAM, 0, m, oc, k)


def mix24(m, oc, m2, form2="mono", **kw):
    """route_cases_lpcm_mix.Mix with 24-bit samples on both elements unless the case says otherwise"""
    kw.setdefault("bps0", 3)
    kw.setdefault("bps1", 3)
    mix = RM.Mix(m, oc, m2, form2, **kw)
    mix.inst24 = inst(m, oc, mix.k)
    return mix


def second(m, k):
    """the second element of instance (m, .., k): a coupled stereo pair for k == 2, else mono for odd m, first order for even"""
    return (2, "pair") if k == 2 else ((1 if m & 1 else 4), "mono")


def reset_tallies(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    for f in OTHER_FAMILIES + (FAM,):
        A.route_family_tally(f, reset=True)


def tallies(A):
    """-> (the family's tally, the base tally, every other packet-fed row that was launched), all reset"""
    fam, base = A.route_family_tally(FAM, reset=True), A.route_tally()
    other = dict(A.route_tally_ext())
    other.update(A.route_table_tally(2, reset=True))
    for f in OTHER_FAMILIES:
        other.update(A.route_family_tally(f, reset=True))
    A.route_reset()
    A.route_tally_ext(reset=True)
    return fam, base, other


def render(mix, fmt=None, placement="own", first=0, n_samples=0, rng_streams=None, limiter=True, out_stream=None, steps=None,
           before_call=None, prefill_state=False):
    """Renders mix.calls and flushes.  steps: per call "new" (default: iamf_hip_batch_render_packets_mix), "old"
    (iamf_hip_batch_render_lpcm_mix on the same packets) or "f32" (iamf_hip_batch_render_range with d_in / d_in2 on f32 copies
    of the same frames).  placement: "own" — each element in a buffer of its own; "shared" — element 1's runs in element 0's
    packet rows, behind them.  rng_streams: (s0, cnt) — every call and the flush over that range only.  before_call(k, stream)
    runs in front of call k and may return a function to run right behind it.
    -> dict(pcm=[per stream uint8], emitted=[..], state=exported in front of the flush, states=[exported behind every call],
            state0=exported in front of the first call (prefill_state), notes=[..], fmt=..)"""
    import torch
    import iac_amd as A
    import gpu_util as G
    S, fs, oc, F = mix.S, mix.fs, mix.oc, mix.F
    fmt = A.FMT_S16 if fmt is None else fmt
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
    s0, cnt = rng_streams or (0, S)
    if placement == "shared":
        d_both = torch.from_numpy(np.concatenate([mix.raw0, mix.raw1], axis=2)).cuda()
        row = mix.row0 + mix.row1
        places = [(d_both.data_ptr(), row), (d_both.data_ptr() + mix.row0, row)]
    else:
        d0, d1 = torch.from_numpy(mix.raw0).cuda(), torch.from_numpy(mix.raw1).cuda()
        places = [(d0.data_ptr(), mix.row0), (d1.data_ptr(), mix.row1)]
    d_x0 = d_x1 = None
    if steps and "f32" in steps:     # [S][F][ch][fs] planar f32 copies of both elements
        def frames(x, ch):
            return torch.from_numpy(np.ascontiguousarray(x.reshape(S, ch, F, fs).transpose(0, 2, 1, 3))).cuda()
        d_x0, d_x1 = frames(mix.x0, mix.m), frames(mix.x1, mix.m2)
    d_ramps = {k: torch.from_numpy(v).cuda() for k, v in mix.ramps.items()}
    b = A.Batch(S, mix.mx, oc, frame_size=fs, out_format=fmt, limiter=limiter, projection=A.PROJ_EXACT,
                sample_rate=mix.sample_rate, threshold_db=mix.threshold_db)
    outs, emitted, notes, states = [[] for _ in range(S)], [], [], []
    try:
        b.set_gains(element=mix.eg, output=mix.og)
        b.set_second_element(mix.mx2, mix.eg2)
        sb = b.stream_state_bytes()

        def export():
            d_state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
            b.export_range(0, S, d_state.data_ptr(), sb, st)
            torch.cuda.synchronize()
            return d_state.cpu().numpy()

        def take(rows, n):
            torch.cuda.synchronize()
            h = G.rows_and_rest(rows, G.DENSE, n * oc * bps, only=(s0, cnt))   # (every byte outside the emitted runs: 0xA5)
            for s in range(s0, s0 + cnt):
                outs[s].append(h[s])
            emitted.append(n)

        state0 = export() if prefill_state else None
        f0 = 0
        for k, nf in enumerate(mix.calls):
            total = n_samples if n_samples else nf * fs
            rows, d_pcm, stride = G.pcm_rows(S, max(total, 240) * oc * bps, G.DENSE, bps)
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n_samples, d_pcm, stride, st
            for which, field in (("e0", "d_element_ramp"), ("e1", "d_element2_ramp"), ("out", "d_output_ramp")):
                if which in d_ramps:   # the call's samples of every stream's ramp: stream stride = the whole programme
                    setattr(a, field, d_ramps[which].data_ptr() + 4 * (f0 * fs + first))
                    a.ramp_stream_stride = F * fs
            after = before_call(k, st) if before_call else None
            step = steps[k] if steps else "new"
            if step == "f32":
                a.d_in, a.in_stream_stride, a.in_frame_stride = d_x0.data_ptr() + 4 * f0 * mix.m * fs, F * mix.m * fs, mix.m * fs
                a.d_in2, a.in2_stream_stride, a.in2_frame_stride = d_x1.data_ptr() + 4 * f0 * mix.m2 * fs, F * mix.m2 * fs, mix.m2 * fs
                n = b.render_range(a, s0, cnt)
            else:
                ins = []
                for (ptr, row), L in zip(places, (mix.L0, mix.L1)):
                    inp = A.LpcmInput()
                    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = ptr + f0 * row, F * row, row
                    inp.first_sample, inp.layout = first, L
                    ins.append(inp)
                n = (b.render_lpcm_mix if step == "old" else b.render_packets_mix)(ins[0], ins[1], a, s0, cnt)
            if after:
                notes.append(after())
            take(rows, n)
            states.append(export())
            f0 += nf
        state = states[-1]
        if limiter:
            rows, d_pcm, stride = G.pcm_rows(S, 240 * oc * bps, G.DENSE, bps)
            take(rows, b.flush_range(d_pcm, stride, st, s0, cnt))
    finally:
        b.close()
    pcm = [np.concatenate(o) if o else np.zeros(0, dtype=np.uint8) for o in outs]
    return dict(pcm=pcm, emitted=emitted, state=state, states=states, state0=state0, notes=notes, fmt=fmt)


def check(mix, fused, bd=16, what="", unfused_base=None, fused_family=None, **kw):
    """Renders `mix` through the new entry, and a twin batch through the same entry under IAMF_HIP_LPCM_UNFUSED=1.  fused: the
    family's tally names mix.inst24 once per call and the base tally holds the flush's GENERIC row alone; else the family's
    tally is empty and the base tally is unfused_base (default: the f32 mixing variant per call + the flush).  fused_family:
    {family: {row: launches}} another packet-fed family is to show instead (16-bit packets on both sides).  Either way: no
    other packet-fed row, PCM bit for bit the oracle's, and PCM, n_emitted and the exported stream state equal to the twin's."""
    import iac_amd as A
    import test_gpu_programmes as TP
    fmt = getattr(A, RM.BD_FMT[bd])
    n_calls = len(mix.calls)
    reset_tallies(A)
    got = render(mix, fmt=fmt, **kw)
    fam, base, other = tallies(A)
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        twin = render(mix, fmt=fmt, **kw)
        fam_twin, base_twin, other_twin = tallies(A)
    f32 = unfused_base if unfused_base is not None else {("FAST", 1, mix.m, mix.oc, 0): n_calls, R.gen(mix.m): 1}
    if fused:
        assert fam == {mix.inst24: n_calls}, (what, "the family's tally", fam)
        assert base == {R.gen(mix.m): 1}, (what, "the base tally: the flush's GENERIC row alone", base)
        assert other == {}, (what, other)
    elif fused_family is not None:
        assert fam == {} and other == fused_family and base == {R.gen(mix.m): 1}, (what, fam, other, base)
    else:
        assert fam == {} and base == f32 and other == {}, (what, fam, base, other)
    assert not [k for k in base if k[0] in PACKET_FED or k[0] == "NONE"], (what, base)
    assert fam_twin == {} and other_twin == {} and base_twin == f32, (what, fam_twin, other_twin, base_twin)
    assert got["emitted"] == twin["emitted"], (what, got["emitted"], twin["emitted"])
    for k, (g, t) in enumerate(zip(got["states"], twin["states"])):
        assert np.array_equal(g, t), (what, "the stream state exported behind call %d against the unfused twin's" % k)
    first, n_samples = kw.get("first", 0), kw.get("n_samples", 0)
    cut, sizes = ((first, first + n_samples), [n_samples]) if n_samples else (None, None)
    s0, cnt = kw.get("rng_streams") or (0, mix.S)
    for s in range(s0, s0 + cnt):
        want, pre, y0, y1 = mix.want(s, bd, sizes=sizes, cut=cut, limiter=kw.get("limiter", True))
        if mix.hot:
            mix.assert_drives_the_limiter(s, pre, y0, y1, what)
        g, t = RM.view(got["pcm"][s], mix.oc, fmt), RM.view(twin["pcm"][s], mix.oc, fmt)
        assert TP.mismatch(g, want) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, want))
        assert TP.mismatch(g, t) is None, (what, "stream %d against the unfused twin" % s, TP.mismatch(g, t))
    return got, twin


# ---- 1. every instance ----

@pytest.mark.parametrize("m,oc,k", INSTANCES, ids=["m%d_oc%d_k%d" % i for i in INSTANCES])
def test_every_instance(m, oc, k):
    import iac_amd as A
    assert inst(m, oc, k) in A.route_family_instances(FAM)
    m2, form2 = second(m, k)
    mix = mix24(m, oc, m2, form2)
    assert mix.L0.sample_bytes == 3 and mix.L1.sample_bytes == 3
    for x in (mix.x0, mix.x1):      # (exact in f32) the low byte of the 24-bit samples is populated
        assert len(np.unique(np.rint(x.astype(np.float64) * (1 << 23)).astype(np.int64) & 0xFF)) > 64
    check(mix, True, what="m%d oc%d k%d" % (m, oc, k))


# ---- 2. per-stream gains ----

@pytest.mark.parametrize("m,k", [(16, 2), (6, 1)])
def test_per_stream_gains_including_the_ones_the_reference_skips(m, k):
    """element, element-2 and output gain per stream: 1.0 (skipped), non-positive (skipped by the reference:
    IAMF_decoder.c:1383-1408 applies a gain only if it is positive and not 1) and ordinary ones, in every position"""
    mix = mix24(m, 2, 2 if k == 2 else 4, "pair" if k == 2 else "mono", S=4,
                eg=[1.0, -0.5, 0.9, 1.1], eg2=[0.0, 1.0, 1.3, 0.7], og=[0.85, 1.0, -1.0, 1.05])
    check(mix, True, what="gains")


# ---- 3. ramps ----

@pytest.mark.parametrize("which", [("e0",), ("e1",), ("out",), ("e0", "e1", "out")], ids=["element", "element2", "output", "all"])
@pytest.mark.parametrize("m,k", [(9, 2), (12, 1)])
def test_a_ramp_on_each_gain_is_fused(m, k, which):
    mix = mix24(m, 2, 2 if k == 2 else 1, "pair" if k == 2 else "mono")
    for j, w in enumerate(which):
        mix.ramp(w, j + 1)
    check(mix, True, what="ramps %s" % (which,))      # (the family's tally, once per call: the ramped calls were fused)


# ---- 4. packet placement ----

@pytest.mark.parametrize("placement", ["own", "shared"])
@pytest.mark.parametrize("m,k,m2", [(16, 2, 2), (16, 1, 4), (12, 2, 2), (6, 1, 1)])
def test_packet_placement(m, k, m2, placement):
    """runs that are only dword-aligned (head 4, pad 4: a run of 3072 or 6144 bytes and its pad keep the next start 4 mod 8)
    with every byte between them 0x7F / 0x80; element 1 in a buffer of its own, or in the same packet rows as element 0 (its
    runs behind element 0's, the same strides)"""
    mix = mix24(m, 2, m2, "pair" if k == 2 else "mono", head=(4, 4), pad=(4, 4), fill=True)
    offs = [mix.L1.src_offset[c] for c in range(m2)] + [mix.L0.src_offset[c] for c in range(m)]
    starts = [o for o in offs if o % 4 == 0]       # (a pair's partner lies 3 bytes behind its first channel)
    assert all(o % 4 in (0, 3) for o in offs) and any(o % 8 == 4 for o in starts), offs
    check(mix, True, what=placement, placement=placement)


# ---- 5. frames that are no whole chunks ----

def test_frames_of_192_samples_sixteen_per_call():
    """a chunk of 1024 samples spans five to six frames: every lane divides its sample index by the frame size"""
    for m, k, m2 in ((16, 2, 2), (6, 1, 4)):
        mix = mix24(m, 2, m2, "pair" if k == 2 else "mono", fs=192, calls=(16, 16))
        check(mix, True, what="frames of 192, m = %d" % m)


# ---- 6. trimmed starts ----

def test_a_trimmed_start_the_forms_take_is_fused():
    for m, k, m2 in ((16, 2, 2), (6, 1, 4)):
        mix = mix24(m, 2, m2, "pair" if k == 2 else "mono", S=3, calls=(1,))
        check(mix, True, what="first 64", first=64, n_samples=512)


@pytest.mark.parametrize("first,n_samples", [(2, 512), (64, 500)], ids=["first_2", "n_500"])
def test_a_trimmed_start_the_forms_do_not_take_is_unpacked(first, n_samples):
    """first_sample = 2: a pair's 12 bytes stay on the dword grid, a mono run's 6 do not; 500 samples are no whole blocks"""
    mix = mix24(16, 2, 2, "pair", S=3, calls=(1,))
    general = {R.gen(16): 2} if n_samples % 64 else None        # no call of the vector kernels: the general one, and the flush
    check(mix, False, what="first %d, %d samples" % (first, n_samples), first=first, n_samples=n_samples, unfused_base=general)


# ---- 7. shapes that stay unfused ----

@pytest.mark.parametrize("what,kw", [
    ("16-bit element 0, 24-bit second element", dict(m=16, oc=2, m2=1, bps0=2, bps1=3)),
    ("24-bit element 0, 16-bit second element", dict(m=16, oc=2, m2=2, form2="pair", bps0=3, bps1=2)),
    ("coupled 24-bit element 0, 16-bit second element", dict(m=6, oc=2, m2=1, bps0=3, bps1=2)),
    ("big-endian second element", dict(m=16, oc=2, m2=1, le1=False)),
    ("big-endian element 0", dict(m=6, oc=2, m2=2, form2="pair", le0=False)),
    ("stereo second element as two mono runs", dict(m=16, oc=2, m2=2, two_mono=True)),
], ids=["e0_16_e1_24", "e0_24_e1_16", "e0_coupled_24_e1_16", "e1_big_endian", "e0_big_endian", "e1_two_mono"])
def test_forms_that_are_unpacked(what, kw):
    kw = dict(kw)
    m, oc, m2, form2 = kw.pop("m"), kw.pop("oc"), kw.pop("m2"), kw.pop("form2", "mono")
    check(mix24(m, oc, m2, form2, **kw), False, what=what)


def test_six_output_channels_take_wide4_mix_behind_the_two_unpacks():
    mix = mix24(12, 6, 2, "pair")
    check(mix, False, what="six outputs", unfused_base={("WIDE4_MIX", 0, 12, 6, 0): 3, R.gen(12): 1})


def test_limiter_off_is_unpacked():
    mix = mix24(16, 2, 2, "pair")
    check(mix, False, what="limiter off", limiter=False, unfused_base={R.gen(16): 3})


# ---- 8. 16-bit packets on both sides ----

@pytest.mark.parametrize("m,k", [(16, 2), (6, 1)])
def test_16_bit_packets_take_the_16_bit_mix_as_through_the_old_entry(m, k):
    import iac_amd as A
    m2, form2 = second(m, k)
    mix = mix24(m, 2, m2, form2, bps0=2, bps1=2)
    row = {("LPCM_MIX", 0, m, 2, k): 3}
    got, _ = check(mix, False, what="16 bit on both sides", fused_family=row)
    reset_tallies(A)
    old = render(mix, steps=["old"] * 3)
    fam, base, other = tallies(A)
    assert fam == {} and other == row and base == {R.gen(m): 1}, (fam, other, base)
    assert got["emitted"] == old["emitted"]
    for s in range(mix.S):
        assert np.array_equal(got["pcm"][s], old["pcm"][s]), s
    for g, o in zip(got["states"], old["states"]):
        assert np.array_equal(g, o)


# ---- 9. a range of streams ----

def test_a_range_of_streams_leaves_its_neighbours_alone():
    """[1, 3) of four streams: the neighbours' PCM rows keep their 0xA5 (gpu_util.rows_and_rest, in every call) and their
    exported state is what it was before the first call"""
    mix = mix24(9, 2, 2, "pair", S=4)
    got, twin = check(mix, True, what="range", rng_streams=(1, 2), prefill_state=True)
    for r in (got, twin):
        for s in (0, 3):
            assert r["pcm"][s].size == 0
            assert np.array_equal(r["state"][s], r["state0"][s]), ("stream %d was touched" % s)
        for s in (1, 2):
            assert not np.array_equal(r["state"][s], r["state0"][s])


# ---- 10. PCM formats ----

@pytest.mark.parametrize("bd,m,k", [(16, 1, 1), (24, 16, 2), (32, 10, 1), (-32, 4, 2)], ids=["s16", "s24", "s32", "f32"])
def test_pcm_formats(bd, m, k):
    mix = mix24(m, 2, 2 if k == 2 else 4, "pair" if k == 2 else "mono")
    check(mix, True, bd=bd, what="bd %d" % bd)


# ---- 11. hand-over ----

@pytest.mark.parametrize("steps", [("new", "f32", "new"), ("f32", "new", "f32"), ("new", "old", "new")],
                         ids=["fused_f32_fused", "f32_fused_f32", "fused_old_fused"])
@pytest.mark.parametrize("m,k", [(16, 2), (8, 1)])
def test_handover_between_the_fused_form_the_f32_calls_and_the_old_entry(m, k, steps):
    """calls of the new entry, iamf_hip_batch_render_range with d_in / d_in2 and the old entry follow one another on one
    batch; behind every call the exported stream state equals that of a control batch that ran the same frames as f32 on the
    general kernel (IAMF_HIP_FORCE_GENERIC=1), and the PCM is the oracle's"""
    import iac_amd as A
    import test_gpu_programmes as TP
    mix = mix24(m, 2, 2 if k == 2 else 1, "pair" if k == 2 else "mono")
    reset_tallies(A)
    got = render(mix, steps=list(steps))
    fam, base, other = tallies(A)
    n_new = steps.count("new")
    assert fam == {mix.inst24: n_new} and other == {}, (fam, other)      # (the old entry unpacks 24-bit packets)
    assert base == {("FAST", 1, m, 2, 0): 3 - n_new, R.gen(m): 1}, base
    with R.environment({"IAMF_HIP_FORCE_GENERIC": "1"}):
        ref = render(mix, steps=["f32"] * 3)
    fam, base, other = tallies(A)
    assert fam == {} and other == {} and base == {R.gen(m): 4}, (fam, base, other)
    assert got["emitted"] == ref["emitted"]
    for j, (g, r) in enumerate(zip(got["states"], ref["states"])):
        assert np.array_equal(g, r), "the stream state behind call %d (%s) against the general kernel's" % (j, steps[j])
    for s in range(mix.S):
        want, pre, y0, y1 = mix.want(s)
        mix.assert_drives_the_limiter(s, pre, y0, y1)
        assert np.array_equal(got["pcm"][s], ref["pcm"][s]), "stream %d against the general kernel's run" % s
        assert TP.mismatch(RM.view(got["pcm"][s], 2, got["fmt"]), want) is None, "stream %d against the oracle" % s


# ---- 12. a caller-owned non-blocking stream ----

def test_on_a_stalled_non_blocking_stream():
    """The entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call on that stream: the
    device cannot have started the call's work when it returns, so a call that had waited for its stream shows.  Asserted
    in the steady state (the same calls have run once on another batch: no kernel is loaded in the call that is observed)."""
    import iac_amd as A
    import stream_util as SU
    import test_gpu_programmes as TP
    mix = mix24(16, 2, 2, "pair", calls=(1, 3, 2))
    with SU.side_stream() as side:
        h = side.cuda_stream

        def before_call(k, st):
            assert st == h
            SU.assert_non_blocking(st)
            ev = SU.stall(SU.torch_stream(st))
            assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
            return lambda: not ev.query()

        render(mix, out_stream=h)
        reset_tallies(A)
        got = render(mix, out_stream=h, before_call=before_call)
        fam, base, other = tallies(A)
    assert fam == {mix.inst24: 3} and other == {}, (fam, other)
    assert got["notes"] == [True, True, True], got["notes"]      # every call had returned while the stall in front of it still ran
    for s in range(mix.S):
        want, pre, y0, y1 = mix.want(s)
        mix.assert_drives_the_limiter(s, pre, y0, y1)
        g = RM.view(got["pcm"][s], 2, got["fmt"])
        assert TP.mismatch(g, want) is None, ("stream %d against the oracle" % s, TP.mismatch(g, want))


# ---- refusals (a batch needs a device) ----

def test_refusals_leave_the_batch_and_the_pcm_untouched():
    """every refusal the entry documents, each with a sentinel in the PCM rows, and the stream position as it was (a whole-frame
    call behind them emits what a first call emits, fused)"""
    import ctypes as C
    import torch
    import iac_amd as A
    mix = mix24(4, 2, 1, S=3, calls=(1,))
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

    def refused(b, i, a, s0=0, n=None, code=-1):
        with pytest.raises(A.IamfHipError) as e:
            b.render_packets_mix(i[0], i[1], a, s0, n)
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
        for w in range(4):                                           # a reserved word, on a live batch
            call = A.PacketMixCall()
            i = ins()
            call.in_[0], call.in_[1], call.args = i[0], i[1], args()
            call.reserved[w] = 1
            assert A.lib().iamf_hip_batch_render_packets_mix(b.h, C.byref(call), 0, 3) == -1
        torch.cuda.synchronize()
        assert bool((pcm == 0xA5).all())
        assert A.route_family_tally(FAM, reset=True) == {}
        assert b.render_packets_mix(*ins(), args()) == 1024 - 240    # the batch stands where it stood: a first call
        assert A.route_family_tally(FAM, reset=True) == {inst(4, 2, 1): 1}
    finally:
        b.close()
