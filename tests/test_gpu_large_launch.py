"""-m gpu: launches the host has to cut — the unfused packet path at more than 65 535 grid rows.

lpcm_unpack_range (iamf_render.hip) puts streams x frames into the third dimension of the unpacker's grid and cuts a call
into launches of fmax = 65535 / n_streams frames each; with more than 65 535 streams it answers UNIMPLEMENTED.  The
per-launch pointer arithmetic (+ f * raw_frame_stride, + f * ch * fs) is what these tests hold against the oracle.  The
same pass serves the members of iamf_hip_batch_render_fanout_lpcm that need f32.

The unfused path is forced with IAMF_HIP_LPCM_UNFUSED=1 (or taken by big-endian packets); the tallies of all three
tables show that no packet-fed instance ran.  Cases (streams x frames x frame size, every stream its own seed), each
followed by a second call of two frames on the same batch and by the flush:

  257 x 255 x 4     16-bit little-endian   streams x frames = 65 535: one launch
  257 x 256 x 4     16-bit little-endian   255 + 1 frames: a one-frame tail
  1024 x 65 x 64    16-bit little-endian   63 + 2 frames
  1024 x 65 x 64    24-bit big-endian      63 + 2 frames
  1024 x 130 x 4    16-bit little-endian   63 + 63 + 4 frames

into stereo s16, from a stereo element and from a mono one.  Streams 0, 1, the middle and the last one are compared with
the oracle (the cut is across frames, so every stream crosses it), the 16-bit cases in every stream with the same calls
on a twin batch without the switch, and the 0xA5 canaries behind every emitted run must survive (lpcm_util.render_lpcm
reads its PCM through gpu_util.rows_and_rest).  The packet-fed kernel has instances for 1, 4, 9 and 16 inputs and takes
whole multiples of 64 samples: the twin of the mono element runs it where the call has that shape — the tally says which
calls did — and every other twin call is unpacked like the call under test."""
import numpy as np
import pytest

import fanout_lpcm_util as U
import long_positions as LPOS
import lpcm_util as LP
import oracle_lib as O
import route_cases as R

pytestmark = pytest.mark.gpu

UNIMPLEMENTED = -6
FILL = 0xA5
SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION")
UNFUSED = {"IAMF_HIP_LPCM_UNFUSED": "1"}
LPCM_M = (1, 4, 9, 16)

# (streams, frames, frame size, bytes per sample, little-endian, the unpack launches of the first call)
CASES = [(257, 255, 4, 2, True, [255]), (257, 256, 4, 2, True, [255, 1]), (1024, 65, 64, 2, True, [63, 2]),
         (1024, 65, 64, 3, False, [63, 2]), (1024, 130, 4, 2, True, [63, 63, 4])]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _reset(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)


def _tallies(A):
    return A.route_tally(), A.route_tally_ext(), A.route_table_tally(2, reset=True)


def expected_base(m, fs, calls, packet_fed):
    """the rows of the base table: a call of whole 64s takes the fast kernel (packet_fed: its packet-fed form, the early
    variant up to 1024 streams), every other call and the flush the generic one"""
    exp, pos = {}, 0
    for nf in calls:
        total = nf * fs
        fast = total % 64 == 0 and (pos % 16 == 0 or pos >= 240)
        key = (("LPCM", 1, m, 2, 0) if packet_fed else ("FAST", 0, m, 2, 0)) if fast else R.gen(m)
        exp[key] = exp.get(key, 0) + 1
        pos += total
    exp[R.gen(m)] = exp.get(R.gen(m), 0) + 1
    return exp


@pytest.mark.parametrize("m", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("S,nf,fs,bps,le,launches", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_a_call_cut_into_several_unpack_launches(S, nf, fs, bps, le, launches, m):
    import iac_amd as A
    fmax = 65535 // S
    assert launches == [min(fmax, nf - f) for f in range(0, nf, fmax)] and sum(launches) == nf
    calls = [nf, 2]
    F = sum(calls)
    ints = U.ints16(S, F, m, fs, seed0=9000 + 7 * nf, bps=bps)
    perm = list(range(m))[::-1]
    raw, L, row = LP.rows(ints, bps, le, [1] * m, perm, head=16, pad=0, frame_size=fs)
    x = U.decoded(ints, perm, bps)                      # [S][m][F * fs]: what the decoder would hand the renderer
    mx, omx = LPOS.selection(m, 2)
    with R.environment(UNFUSED):
        _reset(A)
        got = LP.render_lpcm(mx, 2, raw, L, row, fs, calls)
        base, ext, t2 = _tallies(A)
    assert ext == {} and t2 == {}, (ext, t2)
    R.check_tally(base, expected_base(m, fs, calls, False))     # no packet-fed instance ran
    for s in sorted({0, 1, S // 2, S - 1}):
        want = O.stream_run(omx, 2, x[s], fs)
        assert float(np.abs(x[s]).max()) > 0.95 or s % 2 == 1, "the programme does not drive the limiter"
        R.compare(got[s].view(np.int16).reshape(-1, 2), want, 0, ("oracle", S, nf, fs, bps, s))
    if le and bps == 2:
        _reset(A)
        twin = LP.render_lpcm(mx, 2, raw, L, row, fs, calls)
        base, ext, t2 = _tallies(A)
        assert ext == {} and t2 == {}, (ext, t2)
        R.check_tally(base, expected_base(m, fs, calls, m in LPCM_M))
        for s in range(S):
            assert np.array_equal(got[s], twin[s]), "stream %d differs from the twin batch without the switch" % s


def test_fanout_whose_shared_unpack_pass_is_cut():
    """one iamf_hip_batch_render_fanout_lpcm call at 1024 x 65 x 64, a first-order element into {stereo s16, 5.1 s16}: the
    stereo member reads the packets itself, the 5.1 member needs f32, so the entry's unpack pass runs and is cut (63 + 2
    frames).  Each member equals its own single call bit for bit, and the oracle in streams 0, 1, 512 and 1023."""
    import iac_amd as A
    S, nf, fs, m = 1024, 65, 64, 4
    calls = [nf, 2]
    specs = [U.member("A"), U.member("B")]
    raw, L, row, x = U.reversed_rows(U.ints16(S, sum(calls), m, fs, seed0=9500), fs)
    mats = [(A.get_h2m_matrix(1, A.SS[sp["layout"]]), O.get_h2m(1, O.SS[sp["layout"]])) for sp in specs]
    got = U.Drive([mo[0] for mo in mats], specs, raw, L, row, None, fs)
    twin = U.Drive([mo[0] for mo in mats], specs, raw, L, row, None, fs)
    try:
        _reset(A)
        for n in calls:
            assert got.fan(n) == (0, 0, 1), got.reports      # nothing shared but the unpack pass
        got.flush()
        base, ext, t2 = _tallies(A)
        assert ext == {} and t2 == {}, (ext, t2)
        # (4160 and 128 samples: a last chunk of 64 is no call of render_wide4_kernel, so 5.1 takes the 256-sample kernel)
        R.check_tally(base, {("LPCM", 1, m, 2, 0): 2, ("WIDE", 0, m, 0, 0): 2, R.gen(m): 2})
        for n in calls:
            twin.single(n)
        twin.flush()
        single, ext, t2 = _tallies(A)
        assert single == base and ext == {} and t2 == {}, (single, base)
        U.assert_same(got, twin, "fan-out against the single calls")
        for j, sp in enumerate(specs):
            oc = got.batches[j].oc
            for s in (0, 1, S // 2, S - 1):
                want = O.stream_run(mats[j][1], oc, x[s], fs)
                R.compare(got.bytes_of(j, s).view(np.int16).reshape(-1, oc), want, 0, ("oracle", sp["layout"], s))
    finally:
        got.close()
        twin.close()


def test_more_streams_than_grid_rows_is_refused_before_anything_happens():
    """65 536 mono streams, 16 frames of 4 samples.  Unfused, the unpacker's grid has no room for one frame of them: the call
    answers UNIMPLEMENTED, allocates nothing, and leaves the positions and the PCM rows as they were.  The packet-fed
    kernel has the streams in the grid's first dimension and takes the call; with the flush behind it streams 0 and
    65 535 match the oracle.  (A call of a single 4-sample frame is no call of the packet-fed kernel — it takes whole
    multiples of 64 samples — and is refused either way.)"""
    import torch
    import gpu_util as G
    import iac_amd as A
    S, nf, fs, m = 65536, 16, 4, 1
    ints = LP.ints(np.random.default_rng(9700), S, nf, m, fs, 2)
    raw, L, row = LP.rows(ints, 2, True, [1], [0], head=16, pad=0, frame_size=fs)
    x = U.decoded(ints, [0])
    mx, omx = LPOS.selection(m, 2)
    st = torch.cuda.current_stream().cuda_stream
    d_raw = torch.from_numpy(raw).cuda()
    cap = 240 * 2 * 2
    b = A.Batch(S, mx, 2, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    nbytes = b.stream_state_bytes()
    blob = torch.zeros((2, nbytes), dtype=torch.uint8, device="cuda")

    def positions():
        return [b.export_range(s, 1, blob.data_ptr(), nbytes, st)[0].cursor[0] for s in (0, S - 1)]

    def call(n_frames):
        rows, d_pcm, stride = G.pcm_rows(S, cap, G.DENSE)
        inp = A.LpcmInput()
        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
        a = A.RenderArgs()
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n_frames, d_pcm, stride, st
        return rows, inp, a

    try:
        assert positions() == [0, 0]
        torch.cuda.synchronize()
        for env, n_frames in ((UNFUSED, nf), (UNFUSED, 1), ({}, 1)):
            rows, inp, a = call(n_frames)
            free_before = torch.cuda.mem_get_info()[0]
            with R.environment(env):
                _reset(A)
                with pytest.raises(A.IamfHipError) as e:
                    b.render_lpcm(inp, a)
                tallies = _tallies(A)
            free_after = torch.cuda.mem_get_info()[0]
            assert e.value.code == UNIMPLEMENTED, (env, n_frames, e.value.code)
            assert tallies == ({}, {}, {}), tallies
            # the f32 rows of the call would be S * n_frames * fs floats
            assert free_before - free_after < S * n_frames * fs * 4, "the refused call allocated its f32 buffer"
            torch.cuda.synchronize()
            G.rows_and_rest(rows, G.DENSE, 0)
            assert positions() == [0, 0]
        out = []
        _reset(A)
        rows, inp, a = call(nf)
        n = b.render_lpcm(inp, a)
        torch.cuda.synchronize()
        out.append(G.rows_and_rest(rows, G.DENSE, n * 4))
        assert positions() == [nf * fs, nf * fs]
        rows, d_pcm, stride = G.pcm_rows(S, cap, G.DENSE)
        n = b.flush(d_pcm, stride, st)
        torch.cuda.synchronize()
        out.append(G.rows_and_rest(rows, G.DENSE, n * 4))
        base, ext, t2 = _tallies(A)
        assert ext == {} and t2 == {}
        R.check_tally(base, {("LPCM", 0, m, 2, 0): 1, R.gen(m): 1})     # more than 1024 workgroups: the late variant
        for s in (0, S - 1):
            got = np.concatenate([o[s] for o in out]).view(np.int16).reshape(-1, 2)
            R.compare(got, O.stream_run(omx, 2, x[s], fs), 0, ("oracle", s))
    finally:
        rows = d_raw = None
        b.close()
