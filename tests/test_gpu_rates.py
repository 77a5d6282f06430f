"""-m gpu: every limiter kernel at sample rates from 5.4 kHz to 384 kHz.

iamf_hip_batch_create derives the limiter's step counts from the sample rate — n_atk attack steps, n_end attack plus release
steps, the length of the coefficient table — and those two integers steer the per-chunk hypothesis gains and the chain-wave
walk, which exist in five separately written copies (render_fast.hpp, render_wide4.hpp, render_wide.hpp,
render_fanout.hpp, render_generic.hpp) and two template forms of the first (RAG: interleaved, ragged calls; !kTab: the fused
HRTF variant, which reads the table from global memory).  tests/test_gpu_programmes.py holds them at 48 kHz, where the
attack (48 steps) is shorter than a 64-sample block and a multiple of 4.  Here the same structured programmes run at the
rates of programmes.RATE_STEPS (tests/test_programmes_cpu.py asserts what each is for and that the re-trigger sweep still
hits the limiter's four phase boundaries there; tests/golden/programmes.json pins the reference on them):

    rate      n_atk  n_end
    5408      6      1088    n_end == kFWin: the release ends on the last word of the staged window
    8000      8      1608    a release shorter than two chunks
    22050     23     4433    n_atk % 4 == 3
    44100     45     8864    n_atk % 4 == 1
    96000     97     19298   an attack longer than one 64-sample block
    192000    193    38574   ... than three
    384000    385    77114   ... than the 240-sample look-ahead and a 256-sample block

and on the refused side of the two staged windows: 5407 Hz (n_end = 1087 = kFWin - 1: the general kernel for mono and stereo,
render_wide.hpp's for the wide layouts) and 1587 Hz (n_end = 319 = kWWin - 1: the general kernel).  Every test asserts the
launch tally of the instance it names and compares EVERY stream with the oracle, bit for bit (the two MFMA projections
within 1 LSB, as everywhere); one programme per stream.  The five copies also get programmes.attack_across_chunks (1024-chunks
that start one to four steps into the attack: the hypothesis changes formula inside a lane's quad), and FAST, GENERIC and the
interleaved form run once more with f32 output, where a gain that is off by an ulp shows by its bits.

Why no index leaves its array at n_atk = 385 (read before the first run at that rate).  n_atk enters every copy in
comparisons only (gain_at, the per-round and per-sample choice of formula); no index is computed from it.  The indices:
  * p.ctab[...]: every read is clamped to n_end (`i < n_end ? i : n_end`, `ci` <= n_end in limiter_wave and in the !kTab
    form's look), and the table has n_end + 1 entries (iamf_hip_batch_create).
  * win[...], round 0: win[o0 .. o0 + 3] with o0 = 4 * t <= 1020 (render_wide.hpp: win[t + 1], t <= 255): inside kFWin = 1088
    (kWWin = 320) whatever the rate.
  * head + (n0 + 1) + o0 .. + 3 in a later round (fast, wide4, fan-out): a walk has just ended at block bs, n0 is the number
    of steps since the walk's last trigger, which lies in the chunk, so n0 + 1 + o0 + 3 <= (samples from that trigger to the
    chunk's end) <= 1023 < kFWin.  The walk's "one more block" adds at most 64 to n0 and removes 64 from o0.
  * look(ci) in the walk: win[d] only for 0 <= d < kFWin, else head[min(ci, kFWin - 1)].
  * render_generic.hpp: head[ci] only for ci < kHead, else p.ctab[ci] with ci <= n_end.
So the rule n_end >= kFWin (kWWin) of pick_route() is the only one the rates touch, and it needs no companion for n_atk."""
import numpy as np
import pytest

import programmes as P
import route_cases as R
import test_gpu_programmes as TP
from test_gpu_programmes import FS, limiter_set, mismatch, run_family, selection

pytestmark = pytest.mark.gpu

RATES = P.SWEEP_RATES                       # 5408 .. 384000
BOUNDARY_RATES = (5408, 22050, 96000, 192000)
BELOW_FWIN, BELOW_WWIN, AT_WWIN = 5407, 1587, 1588
SWITCHES = TP.SWITCHES + ("IAMF_HIP_FIR_FUSED", "IAMF_HIP_FIR_F16", "IAMF_HIP_FIR_F32", "IAMF_HIP_LP_EARLY", "IAMF_HIP_INTERLEAVED_UNFUSED")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def frames_of(rate):
    return max(P.frames(rate), 4)           # (four frames: the shortest the non-finite programme fits)


def calls_of(rate):
    return P.cut_calls(frames_of(rate))


def wide_calls(rate):
    """calls in frames of 256: 1, 2, 3, the rest in one or two long calls, 2"""
    rest = 4 * frames_of(rate) - 8
    return [1, 2, 3] + ([rest // 3, rest - rest // 3] if rest >= 10 else [rest]) + [2]


def full_set(m, rate, n=None, nonfinite=True):
    """every limiter programme, nonfinite and the eight sweep streams, at every rate (78 frames at 384 kHz: a case still
    takes well under a second on the MI355X)"""
    n = n or FS * frames_of(rate)
    return limiter_set(m, n, rate, nonfinite=nonfinite) + [("attack_across_chunks", P.attack_across_chunks(m, n, rate))]


def boundary(m, rate, packet_bits=0):
    return P.boundary_set(m, FS * frames_of(rate), rate, packet_bits=packet_bits)


def plateau(m, n, rate, db):
    return [("dc_at_threshold", P.dc_at_threshold(m, n, rate, db=db)), ("dc_one_ulp_above", P.dc_one_ulp_above(m, n, rate, db=db))]


PLATEAU = [(rate, db) for rate in (48000, 96000) for db in (0.0, -6.0)]


# ------------------------------------------------------------------------------------------
# the five copies on the full programme set
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oc,bd", [(2, 16), (1, 16), (2, -32)], ids=["stereo", "mono", "stereo_f32"])
@pytest.mark.parametrize("rate", RATES + (BELOW_FWIN,))
def test_fast(rate, oc, bd):
    """f32 output: every gain by its bits, where 16-bit PCM hides a difference of an ulp"""
    inst = ("FAST", 0, 2, oc, 0) if rate >= 5408 else R.gen(2)
    run_family(inst, 2, oc, full_set(2, rate), calls=calls_of(rate), rate=rate, bd=bd)


@pytest.mark.parametrize("rate", RATES + (BELOW_FWIN,))
def test_wide4(rate):
    """at 5407 Hz the call lands on the 256-sample kernel, whose window is 320"""
    inst = ("WIDE4", 0, 6, 6, 0) if rate >= 5408 else ("WIDE", 0, 6, 0, 0)
    run_family(inst, 6, 6, full_set(6, rate), calls=calls_of(rate), rate=rate)


@pytest.mark.parametrize("rate", RATES + (BELOW_FWIN, AT_WWIN, BELOW_WWIN))
def test_wide(rate):
    inst = ("WIDE", 0, 12, 0, 0) if rate >= AT_WWIN else R.gen(12)
    run_family(inst, 12, 11, full_set(12, rate), fs=256, calls=wide_calls(rate), rate=rate)


@pytest.mark.parametrize("rate", RATES + (BELOW_FWIN,))
def test_fanout(rate):
    """4 -> {2, 1}; at 5407 Hz no member's call is a call of the fast kernel, and each is rendered singly by the general one"""
    TP.run_fanout(4, [2, 1], full_set(4, rate), calls=calls_of(rate), rate=rate, fused=rate >= 5408)


@pytest.mark.parametrize("bd", [16, -32], ids=["s16", "f32"])
@pytest.mark.parametrize("rate", RATES + (BELOW_FWIN,))
def test_generic(rate, bd):
    """1000-sample frames: every call is ragged, and every other kernel refuses it"""
    frames = -(-FS * frames_of(rate) // 1000)
    calls = P.cut_calls(frames)
    for i in range(len(calls) - 1, 0, -1):      # eight frames of 1000 are a multiple of 64: such a call would not be ragged
        if calls[i] % 8 == 0:
            calls[i], calls[i - 1] = calls[i] - 1, calls[i - 1] + 1
    assert all(c % 8 for c in calls) and sum(calls) == frames, calls
    run_family(R.gen(2), 2, 2, full_set(2, rate, 1000 * frames), fs=1000, calls=calls, rate=rate, bd=bd)


def il_lengths(rate):
    """a ragged sequence (one sample either side of a chunk boundary), calls of the resampler's lengths, and the rest of the
    sweep's length in one odd call"""
    need = max(P.LAST_TRIGGER + P.limiter_steps(rate)[1] + 2 + 1024, 4096)
    out = [1023, 1025, 2049] + [1115, 1114, 1115] * 2
    if sum(out) < need:
        out.append((need - sum(out)) | 1)
    return out


@pytest.mark.parametrize("bd", [16, -32], ids=["s16", "f32"])
@pytest.mark.parametrize("rate", RATES + (BELOW_FWIN,))
def test_fast_interleaved(rate, bd):
    """the RAG form; a twin batch through iamf_hip_batch_render_range (the general kernel) must give the same bytes"""
    import interleaved_util as IU
    lengths = il_lengths(rate)
    progs = full_set(2, rate, sum(lengths))
    x = np.stack([p[1] for p in progs])
    IU.check(2, 2, x, lengths, mats=selection(2, 2), eg=[1.0], og=[1.0], fused=None if rate >= 5408 else [False] * len(lengths),
             what="%d Hz" % rate, export=False, sample_rate=rate, bd=bd)


def run_fir(rate, env, inst, progs=None, thr=-1.0, calls=None):
    """a two-channel element through an HRTF set that is the identity (one tap of 1.0 per ear).  The FFT stage is inexact by
    design, so, as tests/test_gpu_fir.py::test_fir_pipeline_with_limiter does, the oracle's limiter and pack run on the
    kernel's OWN f32 stage output, taken with a threshold of +60 dB (gain exactly 1.0); that output is the programme to
    within the stage's tolerance, so the programme still does what it is for."""
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    from test_gpu_fir import F32_TOL
    m, taps = 2, 32
    h = np.zeros((2, m, taps), dtype=np.float32)
    h[0, 0, 0] = h[1, 1, 0] = 1.0
    # (no value of 1000 or more: it would pass +60 dB; no NaN or inf: the transform spreads them over the hop)
    progs = progs or [p for p in full_set(m, rate, nonfinite=False) if p[0] != "loud"]
    calls = calls or calls_of(rate)
    x = np.stack([p[1] for p in progs])
    F = x.shape[2] // FS
    kw = dict(frame_size=FS, limiter=True, flush=True, frames_per_call=calls, fir_taps=taps, sample_rate=rate)
    expect = {inst: len(calls), R.gen(m): 1}
    if inst[0] == "FIR_SPLIT":
        expect[("FAST", 0, 2, 2, 0)] = len(calls)       # gains, limiter and pack behind the stage
    with R.environment(env):
        A.route_reset()
        got = G.hip_render(A.fir_matrix(h), 2, x, fmt=A.FMT_S16, threshold_db=thr, **kw)
        R.check_tally(A.route_tally(), expect)
        A.route_reset()
        stage = G.hip_render(A.fir_matrix(h), 2, x, fmt=A.FMT_F32, threshold_db=60.0, **kw)
        R.check_tally(A.route_tally(), expect)
    bad = []
    for s, (name, xs) in enumerate(progs):
        y = np.ascontiguousarray(stage[s].T)
        assert y.shape == xs.shape and np.abs(y - xs).max() <= F32_TOL * max(1.0, float(np.abs(xs).max())), name
        z, _ = O.limiter_run(y, [FS] * F, rate=rate, thr_db=thr)
        d = mismatch(got[s], O.pack(z, 16))
        if d:
            bad.append("%s: %s" % (name, d))
    assert not bad, "\n".join(["%s at %d Hz:" % (inst[0], rate)] + bad)


@pytest.mark.parametrize("rate", RATES)
def test_fir_fused(rate):
    """the !kTab form of render_fast.hpp: no staged window, every coefficient from global memory"""
    run_fir(rate, {"IAMF_HIP_FIR_FUSED": "1"}, ("FIR_FUSED", 3, 2, 0, 0))


@pytest.mark.parametrize("rate", RATES)
def test_fir_split(rate):
    """the back end of the split form: render_fast_kernel<2, 2> over the FFT kernel's output"""
    run_fir(rate, {}, ("FIR_SPLIT", 0, 2, 0, 0))


# ------------------------------------------------------------------------------------------
# thresholds: the plateau pair at 0 dB (the threshold is exactly 1.0f) and at -6 dB, 48 and 96 kHz
# ------------------------------------------------------------------------------------------

def test_fast_thresholds():
    for rate, db in PLATEAU:
        run_family(("FAST", 0, 2, 2, 0), 2, 2, plateau(2, TP.N, rate, db), thr=db, rate=rate)


def test_wide4_thresholds():
    for rate, db in PLATEAU:
        run_family(("WIDE4", 0, 6, 6, 0), 6, 6, plateau(6, TP.N, rate, db), thr=db, rate=rate)


def test_wide_thresholds():
    for rate, db in PLATEAU:
        run_family(("WIDE", 0, 12, 0, 0), 12, 11, plateau(12, TP.N, rate, db), fs=256, calls=TP.WIDE_CALLS, thr=db, rate=rate)


def test_fanout_thresholds():
    for rate, db in PLATEAU:
        TP.run_fanout(4, [2, 1], plateau(4, TP.N, rate, db), thr=db, rate=rate)


def test_generic_thresholds():
    for rate, db in PLATEAU:
        run_family(R.gen(2), 2, 2, plateau(2, 13000, rate, db), fs=1000, calls=[1, 3, 2, 5, 2], thr=db, rate=rate)


# ------------------------------------------------------------------------------------------
# every other family on the boundary programmes: the eight sweep streams, release_to_idle, onset_after_silence,
# loud_then_silence, silence
# ------------------------------------------------------------------------------------------

def second_pairs(m, rate):
    """the boundary programmes as a mix: streams take turns between (programme, silent second element) and (silent first
    element, the programme's first channel as the second element), so that each phase boundary is hit from either side"""
    n = FS * frames_of(rate)
    out = []
    for i, (name, x) in enumerate(boundary(m, rate)):
        if i % 2 == 0:
            out.append((name + " + silence", x, P.silence(1, n)))
        else:
            out.append(("silence + " + name, P.silence(m, n), np.ascontiguousarray(x[:1])))
    return out


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_fast_second_element(rate):
    TP.run_second(("FAST", 1, 2, 2, 0), 2, 2, second_pairs(2, rate), calls=calls_of(rate), rate=rate)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_wide4_second_element(rate):
    TP.run_second(("WIDE4_MIX", 0, 6, 6, 0), 6, 6, second_pairs(6, rate), calls=calls_of(rate), rate=rate)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_fast_down(rate):
    """(the down-mixer weighs and sums the channels, so where exactly a stream re-triggers is the oracle's to say)"""
    TP.run_down(("FAST_DOWN", 0, 6, 2, 0), 6, 2, boundary(6, rate), N=FS * frames_of(rate), calls=calls_of(rate), rate=rate)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_wide4_down(rate):
    TP.run_down(("WIDE4_DOWN", 0, 12, 10, 0), 12, 10, boundary(12, rate), N=FS * frames_of(rate), calls=calls_of(rate), rate=rate)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_wide4_lfe(rate):
    run_family(("WIDE4_LFE", 0, 4, 6, 0), 4, 6, boundary(4, rate), calls=calls_of(rate), rate=rate, lfe=True)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_wide4_demix(rate):
    """the boundary programmes as the decoded layers of stereo -> 5.1.2 -> 7.1.4 (programmes.demix_case's schedule, repeated):
    the demixer rebuilds channels from them, so where exactly a stream re-triggers is the oracle's to say"""
    import torch
    import demix_cases as D
    A, G, O = TP._mods()
    dc = P.demix_case(FS)
    F = frames_of(rate)
    dc["schedule"] = [dc["schedule"][f % len(dc["schedule"])] for f in range(F)]
    m = oc = len(dc["order"])
    progs = boundary(m, rate)
    S, calls = len(progs), calls_of(rate)
    mx, omx = selection(m, oc)
    x = np.stack([np.ascontiguousarray(xs.reshape(m, F, FS).transpose(1, 0, 2)) for _, xs in progs])      # [S][F][m][fs]
    rec = np.frombuffer(bytes(R.demix_frames(A, dc, S)), dtype=np.uint8).reshape(S, F, -1)

    def extra(a, f0, nf):
        d = torch.from_numpy(rec[:, f0:f0 + nf].copy()).cuda()
        a.d_demix_frames = d.data_ptr()
        return d

    A.route_reset()
    b = A.Batch(S, mx, oc, frame_size=FS, out_format=A.FMT_S16, limiter=True, projection=A.PROJ_EXACT, sample_rate=rate)
    b.set_demixer(dc["layout"], dc["order"], dc["gains"], dc["offset"])
    got = R._ex_loop(A, b, x, extra, list(calls), oc)
    b.close()
    R.check_tally(A.route_tally(), TP.expected_tally(("WIDE4_DEMIX", 0, m, oc, 0), m, len(calls)))
    bad = []
    with np.errstate(all="ignore"):
        for s, (name, _) in enumerate(progs):
            dem = D.drive_demixer(O.lib(), "orc_demixer_", dc, x[s])
            want = O.stream_run(omx, oc, np.ascontiguousarray(dem.transpose(1, 0, 2).reshape(m, F * FS)), FS, rate=rate)
            d = mismatch(got[s], want)
            if d:
                bad.append("%s: %s" % (name, d))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_fanout_members(rate, k):
    TP.run_fanout(4, [2, 1, 2, 1][:k], boundary(4, rate), calls=calls_of(rate), rate=rate)


MFMA_SET = ["silence", "release_to_idle", "square_full_scale"]


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_wide4_mfma(rate):
    run_family(("WIDE4", 1, 6, 6, 0), 6, 6, TP.some(6, MFMA_SET, FS * frames_of(rate), rate), calls=calls_of(rate), rate=rate, mfma=True)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_wide_mfma(rate):
    run_family(("WIDE", 1, 12, 0, 0), 12, 11, TP.some(12, MFMA_SET, FS * frames_of(rate), rate), fs=256, calls=wide_calls(rate), rate=rate,
               mfma=True)


# ---- the packet-fed families: the boundary programmes on the packet's integer grid (programmes.to_packet_grid: the
#      programme divided by 4 as packet samples, a selection matrix of weight 4.0) ----

def packet_frames(m, rate, bits):
    """-> (names, ints [S][F][m][fs] in decoded channel order)"""
    progs = boundary(m, rate)
    ints = np.stack([P.to_packet_grid(x, bits) for _, x in progs])
    S, _, n = ints.shape
    return [p[0] for p in progs], np.ascontiguousarray(ints.reshape(S, m, n // FS, FS).transpose(0, 2, 1, 3))


def packet_planar(ints, perm, bits):
    """the f32 the kernel converts the packets to, [S][m][n] in playback order (exact: an integer over a power of two)"""
    S, F, m, fs = ints.shape
    x = (ints[:, :, perm, :].astype(np.float64) / 2.0 ** (bits - 1)).astype(np.float32)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)


def packet_tallies(A, reset=False):
    """-> (base table, table 2: LPCM24, the coupled family, the extension table: FANOUT_LPCM)"""
    if reset:
        A.route_reset()
        A.route_tally_ext(reset=True)
        A.route_table_tally(2, reset=True)
        A.route_family_tally("LPCM_COUPLED", reset=True)
        return None
    return A.route_tally(), A.route_table_tally(2, reset=True), A.route_family_tally("LPCM_COUPLED", reset=True), A.route_tally_ext()


def run_packets(kind, m, oc, rate, early=1):
    import lpcm_util as LP
    import route_cases_lpcm_mix as RM
    A, G, O = TP._mods()
    bits = 24 if kind == "LPCM24" else 16
    names, ints = packet_frames(m, rate, bits)
    if kind == "LPCM_COUPLED":
        widths, perm = RM.elem0_substreams(m, None)
    else:
        widths, perm = [1] * m, list(range(m))[::-1]
    raw, L, row = LP.rows(ints, bits // 8, True, widths, perm, head=16, pad=0, frame_size=FS)
    mx, omx = selection(m, oc, weight=P.PACKET_WEIGHT)
    calls = calls_of(rate)
    with R.environment({} if early else {"IAMF_HIP_LP_LATE": "1"}):
        packet_tallies(A, reset=True)
        got = LP.render_lpcm(mx, oc, raw, L, row, FS, list(calls), sample_rate=rate)
        base, t2, coupled, ext = packet_tallies(A)
    own = {(kind, early, m, oc, 0): len(calls)}
    flush = {R.gen(m): 1}
    want = {"LPCM": ({**own, **flush}, {}, {}), "LPCM24": (flush, own, {}), "LPCM_COUPLED": (flush, {}, own)}[kind]
    assert (base, t2, coupled, ext) == want + ({},), (kind, base, t2, coupled, ext)
    x = packet_planar(ints, perm, bits)
    bad = []
    for s, name in enumerate(names):
        d = mismatch(got[s].view(np.int16).reshape(-1, oc), O.stream_run(omx, oc, x[s], FS, rate=rate))
        if d:
            bad.append("%s: %s" % (name, d))
    assert not bad, "\n".join(["%s at %d Hz:" % (kind, rate)] + bad)


@pytest.mark.parametrize("early", [1, 0], ids=["early", "late"])
@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_lpcm(rate, early):
    run_packets("LPCM", 4, 2, rate, early)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_lpcm24(rate):
    run_packets("LPCM24", 4, 2, rate)


@pytest.mark.parametrize("m", [2, 6], ids=["stereo", "5.1"])
@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_lpcm_coupled(rate, m):
    run_packets("LPCM_COUPLED", m, 2, rate)


@pytest.mark.parametrize("m,m2,form2", [(4, 1, "mono"), (6, 2, "pair")], ids=["mono_coded_bed", "coupled_bed"])
@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_lpcm_mix(rate, m, m2, form2):
    """both elements as packets; streams take turns between (programme, silent second element) and (silent bed, the programme
    as the second element).  route_cases_lpcm_mix.check: the family's tally, the oracle, and an unfused twin"""
    import route_cases_lpcm_mix as RM
    names, i0 = packet_frames(m, rate, 16)
    _, i1 = packet_frames(m2, rate, 16)
    for s in range(len(names)):
        (i1 if s % 2 == 0 else i0)[s] = 0
    mats = (selection(m, 2, weight=P.PACKET_WEIGHT), selection(m2, 2, weight=P.PACKET_WEIGHT))
    S = len(names)
    mix = RM.Mix(m, 2, m2, form2, S=S, calls=calls_of(rate), sample_rate=rate, ints=(i0, i1), mats=mats, eg=[1.0] * S, eg2=[1.0] * S,
                 og=[1.0] * S)
    RM.check(mix, fused=True, what="%d Hz" % rate)


@pytest.mark.parametrize("rate", BOUNDARY_RATES)
def test_fanout_lpcm(rate):
    """a first-order element as 16-bit packets into a stereo and a mono member in one launch (render_fanout_kernel<4, 2, LP>)"""
    import torch
    import lpcm_util as LP
    A, G, O = TP._mods()
    m, ocs = 4, [2, 1]
    names, ints = packet_frames(m, rate, 16)
    S, F = ints.shape[:2]
    perm = list(range(m))[::-1]
    raw, L, row = LP.rows(ints, 2, True, [1] * m, perm, head=16, pad=0, frame_size=FS)
    mxs = [selection(m, oc, weight=P.PACKET_WEIGHT) for oc in ocs]
    calls = calls_of(rate)
    d_raw = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    batches = [A.Batch(S, mxs[j][0], ocs[j], frame_size=FS, projection=A.PROJ_EXACT, sample_rate=rate) for j in range(2)]
    outs = [[[] for _ in range(S)] for _ in range(2)]

    def take(j, pcm, n):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[j][s].append(h[s][:n * ocs[j] * 2].view(np.int16).reshape(n, ocs[j]).copy())

    packet_tallies(A, reset=True)
    try:
        f0 = 0
        for nf in calls:
            caps = [(nf * FS * oc * 2 + 15) & ~15 for oc in ocs]
            pcms = [torch.zeros((S, cap), dtype=torch.uint8, device="cuda") for cap in caps]
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr() + f0 * row, F * row, row, L
            n_emitted, report = A.render_fanout_lpcm(batches, inp, nf, [p.data_ptr() for p in pcms], caps, st)
            assert report == (2, 1, 0), report
            for j in range(2):
                take(j, pcms[j], n_emitted[j])
            f0 += nf
        for j, b in enumerate(batches):
            cap = (240 * ocs[j] * 2 + 15) & ~15
            pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
            take(j, pcm, b.flush(pcm.data_ptr(), cap, st))
    finally:
        for b in batches:
            b.close()
    base, t2, coupled, ext = packet_tallies(A)
    assert ext == {("FANOUT_LPCM", 0, m, 0, 2): len(calls)} and base == {R.gen(m): 2} and t2 == {} and coupled == {}, (ext, base, t2, coupled)
    x = packet_planar(ints, perm, 16)
    bad = []
    for j in range(2):
        for s, name in enumerate(names):
            d = mismatch(np.concatenate(outs[j][s]), O.stream_run(mxs[j][1], ocs[j], x[s], FS, rate=rate))
            if d:
                bad.append("member %d, %s: %s" % (j, name, d))
    assert not bad, "\n".join(bad)
