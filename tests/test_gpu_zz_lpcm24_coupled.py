"""-m gpu: the coupled 24-bit form of the packet-fed headline kernel (render_fast_kernel<.., LP, EARLY, 3, LPC>,
iac_amd/csrc/iamf_render_lpcm24_coupled.hip) behind iamf_hip_batch_render_packets: 24-bit packets of a channel-based element
whose L/R, Ls/Rs .. pairs are coupled sub-streams, C and LFE mono ones.

Every fused case asserts: the listing by family (iamf_hip_route_family_tally) names the instance of LPCM24_COUPLED, once per
call; no other packet-fed family and no table shows a packet row (the base tally holds the flush's GENERIC row and nothing
else); every stream is bit for bit the oracle's (oracle_lib.stream_run on ints / 2^23 — the reference's LPCM decode,
pcm/IAMF_pcm_decoder.c:71-76, is exact in f32), with PCM and n_emitted equal to a twin batch run under IAMF_HIP_LPCM_UNFUSED=1
(unpack, then the f32 kernel: the path every such call took before), and both batches export the same stream state in front
of the flush.  Tolerance 0 everywhere.  Both prefetch variants are forced by their switches, so no case depends on where the
host cuts between them.  Shapes: 3-6 streams, chunks of 1024 samples, at most a few thousand samples per stream.

The calls that must stay on the old path assert the family's tally empty and tallies, PCM, n_emitted and state equal to the
twin's; the totality cases assert that iamf_hip_batch_render_packets and iamf_hip_batch_render_lpcm leave the same tallies
and bytes for every form the older entry fuses, and that the older entry keeps S24C packets unfused.

(The file's name sorts it behind the other GPU test files: the tests that were there run first, in the order and under the
numbers they had in a run's report.)"""
import functools
import gc

import numpy as np
import pytest

import lpcm_util as LP
import route_cases as R

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_NO_WIDE4", "IAMF_HIP_RAGGED_UNFUSED", "IAMF_HIP_INTERLEAVED_UNFUSED")
FAM = "LPCM24_COUPLED"
COUPLED_M = [2, 6, 8, 10, 12]
OTHER_FAMILIES = ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED")
PACKET_FED = ("LPCM", "LPCM24", "FANOUT_LPCM", "LPCM_COUPLED", "LPCM_MIX", FAM)
UNFUSED = {"IAMF_HIP_LPCM_UNFUSED": "1"}
FULL = 1 << 23


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _mods():
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    return A, G, O


def _variant(early):
    return {} if early is None else ({"IAMF_HIP_LP_EARLY": "1"} if early else {"IAMF_HIP_LP_LATE": "1"})


def _reset(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    for f in (FAM,) + OTHER_FAMILIES:
        A.route_family_tally(f, reset=True)


def _tallies(A):
    """-> (the family's tally, table 0, everything else that lists a kernel: table 1, table 2 and the other families listed
    by family only, as one dict), all reset"""
    fam, base = A.route_family_tally(FAM, reset=True), A.route_tally()
    rest = dict(A.route_tally_ext())
    rest.update(A.route_table_tally(2, reset=True))
    for f in OTHER_FAMILIES:
        rest.update(A.route_family_tally(f, reset=True))
    A.route_reset()
    A.route_tally_ext(reset=True)
    return fam, base, rest


def _no_packet_rows(*tables):
    return not [k for t in tables for k in t if k[0] in PACKET_FED]


def coupled(m):
    """-> (widths, perm) of lpcm_util.rows for a loudspeaker layout of m channels: sub-streams in audio-layer order (the
    coupled pairs, then C and LFE), perm[p] = the decoded channel playback channel p takes (L R C LFE, then the pairs)"""
    if m <= 2:
        return [m], list(range(m))
    return [2] * ((m - 2) // 2) + [1, 1], [0, 1, m - 2, m - 1] + list(range(2, m - 2))


def planar(ints, perm, bits=24):
    S, F, m, fs = ints.shape
    x = (ints[:, :, perm, :].astype(np.float64) / 2.0 ** (bits - 1)).astype(np.float32)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)


def drive_limiter(O, omx, oc, ints, perm):
    """the packets' samples scaled, stream by stream, so that the rendered peak is about 1.3 (threshold: -1 dB = 0.89) where
    it is lower: the scale comes from the oracle's rendering, never from the code under test (samples that leave the 24-bit
    range are clipped; the callers assert the peak they got)"""
    ints = ints.copy()
    for s in range(ints.shape[0]):
        for _ in range(4):          # (clipping takes some of the peak back: scaled again where it took too much)
            peak = float(np.abs(O.render(omx, planar(ints[s:s + 1], perm)[0], oc)).max())
            assert peak > 0.0
            if peak >= 1.1:
                break
            ints[s] = np.clip(np.rint(ints[s] * (1.3 / peak)), -FULL, FULL - 1).astype(np.int64)
    return ints


def fill_gaps(raw, L):
    """every byte of the rows that belongs to no run: 0x7F / 0x80 alternating (a load that strays reads a large sample)"""
    A, G, O = _mods()
    used = G.packet_run_mask(L, raw.shape[-1])
    fill = np.where(np.arange(raw.shape[-1]) % 2 == 0, 0x7F, 0x80).astype(np.uint8)
    return np.where(used[None, None, :], raw, fill[None, None, :])


def _export(b, S, st):
    import torch
    sb = b.stream_state_bytes()
    d_state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
    b.export_range(0, S, d_state.data_ptr(), sb, st)
    torch.cuda.synchronize()
    return d_state.cpu().numpy()


def _render(mx, oc, raw, L, row, fs, calls, first=0, n_samples=0, args_hook=None, batch_hook=None, fmt=None, entry="packets",
            packets=None, rate=48000, limiter=True, batch_kw=None, trims=None, states=None, before_call=None):
    """calls of `entry` ("packets": iamf_hip_batch_render_packets, "lpcm": iamf_hip_batch_render_lpcm) and the flush on one
    batch -> (the streams as gpu_util._view gives them, what every call and the flush emitted, the exported state of every
    stream in front of the flush).  packets: a packet layout of gpu_util (place_packets); None: the rows as they are.
    trims: {call number: (first_sample, n_samples)}; states: a list that receives the exported state behind every call;
    before_call: called in front of every call of the entry"""
    import torch
    A, G, O = _mods()
    S, F, _ = raw.shape
    fmt = A.FMT_S16 if fmt is None else fmt
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=fmt, limiter=limiter, sample_rate=rate, **(batch_kw or {}))
    sc = (batch_kw or {}).get("pcm_stride_channels", 0) or oc
    keep = d_raw = pk_keep = None
    try:
        keep = batch_hook(b) if batch_hook else None
        if packets is None:
            d_raw = torch.from_numpy(raw).cuda()
        st = torch.cuda.current_stream().cuda_stream
        outs, ns, f0 = [[] for _ in range(S)], [], 0
        for k, nf in enumerate(calls):
            cap = max(nf * fs, 240) * sc * bps
            pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
            inp = A.LpcmInput()
            if packets is None:
                inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = d_raw.data_ptr() + f0 * row, F * row, row
            else:
                pl = G.place_packets(raw, L, packets, f0, nf, keep=pk_keep)
                inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, pk_keep = pl.d_raw, pl.stream_stride, pl.frame_stride, pl.keep
            tr = (trims or {}).get(k, (first, n_samples))
            inp.first_sample, inp.layout = tr[0], L
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, tr[1], pcm.data_ptr(), cap, st
            held = args_hook(a, nf) if args_hook else None
            if before_call:
                before_call()
            n = b.render_packets(inp, a) if entry == "packets" else b.render_lpcm(inp, a)
            torch.cuda.synchronize()
            del held
            h = pcm.cpu().numpy()
            for s in range(S):
                outs[s].append(h[s, :n * sc * bps].copy())
            ns.append(n)
            f0 += nf
            if states is not None:
                states.append(_export(b, S, st))
        state = _export(b, S, st)
        pcm = torch.zeros((S, 240 * sc * bps), dtype=torch.uint8, device="cuda")
        n = b.flush(pcm.data_ptr(), 240 * sc * bps, st)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(h[s, :n * sc * bps].copy())
        ns.append(n)
    finally:
        b.close()
        del keep, d_raw, pk_keep
    return [G._view(np.concatenate(o), sum(ns), sc, fmt) for o in outs], ns, state


def check_fused(mx, omx, oc, ints, fs, calls, early, head=16, pad=0, first=0, n_samples=0, fill=False, what="", bd=16, check=None,
                fused=True, hot=False, rate=48000, twin_rows=None):
    """early None: no switch, the variant is whichever the host's rule picks; fused False: the library unpacks this call itself
    (same PCM, the f32 kernel's row: the twin's tally, twin_rows where it is another); hot: the precondition that the programme drives the limiter is asserted"""
    import test_gpu_programmes as TP
    A, G, O = _mods()
    fmt = {16: A.FMT_S16, 24: A.FMT_S24, 32: A.FMT_S32, -32: A.FMT_F32}[bd]
    S, F, m, _ = ints.shape
    widths, perm = coupled(m)
    if hot:
        ints = drive_limiter(O, omx, oc, ints, perm)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=head, pad=pad, frame_size=fs)
    if fill:
        raw = fill_gaps(raw, L)
    with R.environment(_variant(early)):
        _reset(A)
        got, ns, state = _render(mx, oc, raw, L, row, fs, calls, first, n_samples, fmt=fmt, rate=rate)
        fam, base, rest = _tallies(A)
    with R.environment(UNFUSED):
        twin, ns_twin, state_twin = _render(mx, oc, raw, L, row, fs, calls, first, n_samples, fmt=fmt, rate=rate)
        fam_twin, base_twin, rest_twin = _tallies(A)
    if early is None:      # whichever variant the host's rule picks for this size (lpcm24_coupled_early, render_route.hpp)
        assert len(fam) == 1 and next(iter(fam))[1] in (0, 1), (what, fam)
    variant = next(iter(fam))[1] if early is None and fam else early
    f32 = twin_rows or {("FAST", 0, m, oc, 0): len(calls), R.gen(m): 1}
    if fused:
        assert fam == {(FAM, variant, m, oc, 0): len(calls)}, (what, fam, base, rest)
        assert base == {R.gen(m): 1} and rest == {}, (what, base, rest)
    else:
        assert fam == {} and base == f32 and rest == {}, (what, fam, base, rest)
    assert fam_twin == {} and base_twin == f32 and rest_twin == {}, (what, fam_twin, base_twin, rest_twin)
    assert ns == ns_twin, (what, ns, ns_twin)
    assert np.array_equal(state, state_twin), (what, "the exported stream state against the unfused twin's")
    x = planar(ints, perm)
    if n_samples:
        x, ofs = np.ascontiguousarray(x[:, :, first:first + n_samples]), n_samples
    else:
        ofs = fs
    for s in (range(S) if check is None else check):
        if hot:
            assert float(np.abs(O.render(omx, x[s], oc)).max()) > 0.95, (what, "stream %d does not drive the limiter" % s)
        want = TP.oracle_stream(O, omx, oc, x[s], ofs, bd) if rate == 48000 else O.stream_run(omx, oc, x[s], ofs, rate=rate)
        assert TP.mismatch(got[s], want) is None, (what, "stream %d against the oracle" % s, TP.mismatch(got[s], want))
        assert TP.mismatch(got[s], twin[s]) is None, (what, "stream %d against the unfused twin" % s, TP.mismatch(got[s], twin[s]))


# ------------------------------------------------------------------------------------------
# every instance, the cut, geometry
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", [False, True], ids=["dense", "table"])
@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("oc", [1, 2])
@pytest.mark.parametrize("m", COUPLED_M)
def test_every_instance(m, oc, early, table):
    """dense: a seeded matrix with a different weight for every (channel, slot) — a symmetric down-mix into mono would not
    notice L and R swapped; table: the reference's layout -> layout matrix"""
    mx, omx = R.matrices(m, oc, table=table)
    ints = LP.ints(np.random.default_rng(3200 + 10 * m + oc), 3, 3, m, 1024, 3)
    check_fused(mx, omx, oc, ints, 1024, [2, 1], early, hot=True, what="table" if table else "dense")


def test_the_dense_matrix_tells_left_from_right():
    for m in COUPLED_M:
        for oc in (1, 2):
            mx, _ = R.matrices(m, oc, table=False)
            w = np.ctypeslib.as_array(mx.mat, shape=(m * oc,))
            assert len(set(np.abs(w).tolist())) == m * oc, (m, oc)


def _selection(m, oc, gains):
    """[(channel, slot, weight)] -> a matrix with those weights and zeros elsewhere"""
    A, G, O = _mods()
    w = np.zeros((m, oc), dtype=np.float32)
    for c, o, g in gains:
        w[c, o] = g
    return R._custom(A, O, A.KIND_M2M, m, oc, w, oc)


@pytest.mark.parametrize("early", [1, 0])
def test_the_cut_at_the_extremes_and_with_left_and_right_different_in_every_byte(early):
    """One stream each of constant -2^23, 2^23 - 1, +-1 alternating and 0x7FFF80 / -0x7FFF80 alternating, and one whose L and R
    (and every other pair's halves, and C and LFE) differ in every byte of every sample: 0x123456-like bytes on L and their
    complements on R, walking, so that a byte taken from the neighbouring sample or from the partner changes the PCM.  Each
    channel is one step behind its neighbour, so every value sits in every sample of a lane's 24 bytes.  A selection matrix
    with weights 2^-2, 2^-11 and 2^-20 keeps the limiter idle and every bit of every product in the PCM's reach for the first
    pair; the gaps of the rows are 0x7F / 0x80, head 4 and pad 4."""
    m, oc, fs, F, S = 6, 2, 1024, 3, 5
    i = np.arange(F * fs)
    ints = np.zeros((S, F, m, fs), dtype=np.int64)
    for c in range(m):
        alt = np.where((i + c) % 2 == 0, 1, -1)
        ints[0, :, c, :] = np.full(F * fs, -FULL).reshape(F, fs)
        ints[1, :, c, :] = np.full(F * fs, FULL - 1).reshape(F, fs)
        ints[2, :, c, :] = alt.reshape(F, fs)
        ints[3, :, c, :] = (alt * 0x7FFF80).reshape(F, fs)
        # three different bytes per sample, all three walking with the sample index; R (odd c) the bitwise complement of L
        b0, b1, b2 = (0x11 + 7 * i + 3 * c) & 0xFF, (0x5A + 13 * i + 5 * c) & 0xFF, (0x23 + 29 * i + 11 * c) & 0xFF
        u = b0 | (b1 << 8) | (b2 << 16)
        if c & 1:
            u = (~(((0x11 + 7 * i + 3 * (c - 1)) & 0xFF) | (((0x5A + 13 * i + 5 * (c - 1)) & 0xFF) << 8) |
                   (((0x23 + 29 * i + 11 * (c - 1)) & 0xFF) << 16))) & 0xFFFFFF
        ints[4, :, c, :] = ((u ^ FULL) - FULL).reshape(F, fs)
    assert np.all(((ints[4, :, 0] ^ ints[4, :, 1]) & 0xFFFFFF) == 0xFFFFFF)       # L and R differ in every bit, so in every byte
    mx, omx = _selection(m, oc, [(0, 0, 0.25), (1, 1, 0.25), (4, 0, 2.0 ** -11), (5, 1, 2.0 ** -11), (2, 0, 2.0 ** -20), (3, 1, 2.0 ** -20)])
    check_fused(mx, omx, oc, ints, fs, [1, 2], early, head=4, pad=4, fill=True)
    # the same packets into f32 PCM through weights 1, 2^-1, 2^-2 .. per channel into one slot each way round: every bit of
    # every converted sample is a bit of the PCM (|sum| < 0.89: the limiter idle for the streams looked at)
    mx, omx = _selection(m, oc, [(0, 0, 0.5), (1, 1, 0.5)])
    check_fused(mx, omx, oc, ints, fs, [1, 2], early, head=4, pad=4, fill=True, bd=-32, check=[2, 3, 4], what="f32")


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("m", [2, 6, 12])
def test_1025_samples_and_runs_that_are_only_dword_aligned(m, early):
    """frames of 2048 (a call of 1025 samples is no whole number of blocks and is unpacked), two calls of one frame = two chunks
    each, with the first, the 1024th, the 1025th and the last sample of every run at the extremes — the 1024th and the 1025th
    land in different chunks, the last lane of one and the first of the next — head 4 and pad 4 (runs at 4, 8, 12 mod 16), gaps
    filled"""
    mx, omx = R.matrices(m, 2, table=False)
    ints = LP.ints(np.random.default_rng(3266 + m), 3, 2, m, 2048, 3, level=0.2)
    for k, v in ((0, FULL - 1), (1023, -FULL), (1024, FULL - 1), (2047, -FULL)):
        ints[:, :, 0::2, k], ints[:, :, 1::2, k] = v, -v - 1
    widths, perm = coupled(m)
    _, L, _ = LP.rows(ints, 3, True, widths, perm, head=4, pad=4, frame_size=2048)
    offs = [L.src_offset[c] for c in range(m)]
    assert all(o % 4 == 0 or (c % 2 == 1 and L.src_step[c] == 6) for c, o in enumerate(offs)) and any(o % 8 == 4 for o in offs)
    check_fused(mx, omx, 2, ints, 2048, [1, 1], early, head=4, pad=4, fill=True)


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("m", [6, 12])
def test_chunks_straddle_frames_and_the_last_chunk_is_short(m, early):
    # 192-sample frames, 11 of them: calls of 1152 and 960 samples, chunks of 1024 + 128 and of 960, a lane's frame by division
    mx, omx = R.matrices(m, 2, table=False)
    ints = LP.ints(np.random.default_rng(3264 + m), 3, 11, m, 192, 3)
    check_fused(mx, omx, 2, ints, 192, [6, 5], early, hot=True)


@pytest.mark.parametrize("early", [1, 0])
def test_frames_of_128(early):
    mx, omx = R.matrices(8, 2, table=False)
    ints = LP.ints(np.random.default_rng(3270), 3, 20, 8, 128, 3)
    check_fused(mx, omx, 2, ints, 128, [9, 8, 3], early, hot=True)


@pytest.mark.parametrize("m,oc,early", [(12, 2, 1), (12, 2, 0), (6, 1, 1)])
@pytest.mark.parametrize("bd", [24, 32, -32])
def test_into_s24_s32_and_f32_pcm(m, oc, early, bd):
    mx, omx = R.matrices(m, oc, table=False)
    ints = LP.ints(np.random.default_rng(3300 + 10 * m + oc), 3, 3, m, 1024, 3)
    check_fused(mx, omx, oc, ints, 1024, [2, 1], early, bd=bd, what="bd %d" % bd)


@pytest.mark.parametrize("early", [0, 1, None], ids=["late", "early", "the_hosts_rule"])
def test_1025_streams(early):
    """more workgroups than four a CU: the late variant, the early one and whichever the host's rule picks with no switch set
    (lpcm24_coupled_early, render_route.hpp); the first, the 1024th and the 1025th stream"""
    mx, omx = R.matrices(2, 2, table=False)
    ints = LP.ints(np.random.default_rng(3320), 1025, 1, 2, 1024, 3)
    check_fused(mx, omx, 2, ints, 1024, [1], early, check=[0, 1023, 1024])


# ------------------------------------------------------------------------------------------
# per-call decisions through the new entry
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("m,first,fused", [(2, 2, True), (2, 6, True), (2, 1, False), (2, 3, False), (6, 4, True), (6, 8, True), (6, 2, False),
                                           (6, 1, False)])
def test_a_trimmed_frame(m, first, fused, early):
    """a pair's run is on the dword grid from every even first sample; C and LFE from every fourth.  Off it the library
    unpacks the call itself: the same PCM."""
    mx, omx = R.matrices(m, 2, table=False)
    ints = LP.ints(np.random.default_rng(3265 + m), 4, 1, m, 1024, 3)
    check_fused(mx, omx, 2, ints, 1024, [1], early, first=first, n_samples=512, fused=fused)


@pytest.mark.parametrize("early", [1, 0])
def test_a_call_that_is_no_whole_number_of_blocks_is_unfused(early):
    mx, omx = R.matrices(6, 2, table=False)
    ints = LP.ints(np.random.default_rng(3330), 3, 1, 6, 1024, 3)
    check_fused(mx, omx, 2, ints, 1024, [1], early, first=0, n_samples=1000, fused=False, twin_rows={R.gen(6): 2})


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("first,n_samples", [(24, 1000), (0, 237), (0, 3)])
def test_positions_off_the_16_sample_grid(first, n_samples, early):
    """A first one-frame call trimmed to [first, first + n_samples), two calls of a whole frame, the flush.  The tally follows
    fast_shape_ok (render_route.hpp): the trimmed call is no call of the vector kernels (its sample count is no multiple of
    64), a whole frame from a position of at least 240 is fused whatever its residue mod 16, one from an off-grid position
    below 240 is not."""
    A, G, O = _mods()
    m, oc, fs, S, F = 6, 2, 1024, 3, 3
    assert n_samples % 64 and first + n_samples <= fs
    mx, omx = R.matrices(m, oc, table=False)
    ints = LP.ints(np.random.default_rng(3340 + n_samples), S, F, m, fs, 3)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=16, pad=0, frame_size=fs)
    raw = fill_gaps(raw, L)
    calls, trims = [1, 1, 1], {0: (first, n_samples)}

    def run(env):
        with R.environment(env):
            _reset(A)
            got, ns, state = _render(mx, oc, raw, L, row, fs, calls, trims=trims)
            return (got, ns, state) + _tallies(A)

    got, ns, state, fam, base, rest = run(_variant(early))
    twin, ns_twin, state_twin, fam_twin, base_twin, rest_twin = run(UNFUSED)
    fused = [pos >= 240 or pos % 16 == 0 for pos in (n_samples, n_samples + fs)]     # where the whole-frame calls start
    general = 1 + fused.count(False) + 1                                               # the trimmed call, ..., the flush
    assert fam == ({(FAM, early, m, oc, 0): fused.count(True)} if any(fused) else {}), fam
    assert base == {R.gen(m): general} and rest == {}, (base, rest)
    want_twin = {R.gen(m): general}
    if any(fused):
        want_twin[("FAST", 0, m, oc, 0)] = fused.count(True)
    assert fam_twin == rest_twin == {} and base_twin == want_twin, (fam_twin, base_twin)
    assert ns == ns_twin and np.array_equal(state, state_twin), (ns, ns_twin)
    x = planar(ints, perm)
    kept = np.ascontiguousarray(np.concatenate([x[:, :, first:first + n_samples], x[:, :, fs:]], axis=2))
    for s in range(S):
        want = O.stream_run(omx, oc, kept[s], fs)
        assert got[s].shape == want.shape and np.array_equal(got[s], want), "stream %d against the oracle" % s
        assert np.array_equal(got[s], twin[s]), "stream %d against the unfused twin" % s


def check_unfused(mx, oc, ints, widths, perm, fs, calls, omx=None, args_hook=None, batch_hook=None, kernel=("FAST", 0), what="", limiter=True,
                  batch_kw=None, bps=3, le=True, own=None):
    """through iamf_hip_batch_render_packets: the new family's tally empty, tallies, PCM, n_emitted and state the twin's (and
    the oracle's where one is given).  own: the tally the call is to show instead of the f32 kernel's (a form the older entry
    fuses) — then the twin is the SAME call through iamf_hip_batch_render_lpcm, not the unfused pair"""
    A, G, O = _mods()
    S, F, m, _ = ints.shape
    raw, L, row = LP.rows(ints, bps, le, widths, perm, head=16, pad=0, frame_size=fs)
    kw = dict(args_hook=args_hook, batch_hook=batch_hook, limiter=limiter, batch_kw=batch_kw)
    _reset(A)
    got, ns, state = _render(mx, oc, raw, L, row, fs, calls, **kw)
    fam, base, rest = _tallies(A)
    with R.environment({} if own is not None else UNFUSED):
        twin, ns_twin, state_twin = _render(mx, oc, raw, L, row, fs, calls, entry="lpcm", **kw)
        fam_twin, base_twin, rest_twin = _tallies(A)
    assert fam == fam_twin == {}, (what, fam)
    assert base == base_twin and rest == rest_twin, (what, base, base_twin, rest, rest_twin)
    if own is not None:
        merged = dict(base)
        merged.update(rest)
        assert merged == own, (what, base, rest)
    else:
        assert _no_packet_rows(base) and rest == {}, (what, base, rest)
        if kernel:
            assert base == {kernel + (m, oc, 0): len(calls), R.gen(m): 1}, (what, base)
    assert ns == ns_twin and np.array_equal(state, state_twin), what
    for s in range(S):
        assert np.array_equal(got[s], twin[s]), (what, "stream %d against the twin" % s)
        if omx is not None:
            want = O.stream_run(omx, oc, planar(ints, perm, 8 * bps)[s], fs)
            assert np.array_equal(got[s], want), (what, "stream %d against the oracle" % s)


def test_limiter_off_stays_unfused():
    mx, omx = R.matrices(6, 2, table=False)
    widths, perm = coupled(6)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(3350), 3, 3, 6, 1024, 3, level=0.1), widths, perm, 1024, [2, 1], limiter=False, kernel=None)


def test_more_than_two_output_channels_stays_unfused():
    # 7.1.4 into Sound System B: a wide kernel behind the unpacker
    A, G, O = _mods()
    mx, omx = A.get_m2m_matrix(A.SS["L714"], A.SS["B"]), O.get_m2m(O.SS["L714"], O.SS["B"])
    widths, perm = coupled(12)
    check_unfused(mx, 6, LP.ints(np.random.default_rng(3351), 3, 3, 12, 1024, 3), widths, perm, 1024, [2, 1], omx=omx, kernel=None)


def test_a_fixed_pcm_channel_stride_stays_unfused():
    mx, omx = R.matrices(6, 2, table=False)
    widths, perm = coupled(6)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(3352), 3, 3, 6, 1024, 3), widths, perm, 1024, [2, 1], kernel=("FAST", 0),
                  batch_kw={"pcm_stride_channels": 4})


def test_a_batch_with_a_second_element_is_refused_as_the_older_entry_refuses_it():
    """iamf_hip_packet_call has no second element (d_in2 must be NULL), and iamf_hip_batch_render_lpcm_range refuses a batch with
    a second element that is given none: the new entry answers with that entry's code, and with d_in2 set with its own
    IAMF_HIP_ERR_BAD_ARG; neither changes the batch or the PCM"""
    import ctypes as C
    import torch
    A, G, O = _mods()
    m, oc, fs, S = 6, 2, 1024, 3
    mx, _ = R.matrices(m, oc, table=False)
    mx2, _ = R.matrices(2, 2)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(LP.ints(np.random.default_rng(3353), S, 1, m, fs, 3), 3, True, widths, perm, head=16, pad=0, frame_size=fs)
    d_raw = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    try:
        b.set_second_element(mx2)
        pcm = torch.full((S, fs * oc * 2), 0xA5, dtype=torch.uint8, device="cuda")
        x2 = torch.zeros((S, 2, fs), dtype=torch.float32, device="cuda")
        call = A.PacketCall()
        call.in_.d_raw, call.in_.raw_stream_stride, call.in_.raw_frame_stride, call.in_.layout = d_raw.data_ptr(), row, row, L
        call.args.n_frames, call.args.d_pcm, call.args.pcm_stream_stride_bytes, call.args.stream = 1, pcm.data_ptr(), fs * oc * 2, st
        before = _export(b, S, st)
        _reset(A)
        want = A.lib().iamf_hip_batch_render_lpcm_range(b.h, C.byref(call.in_), C.byref(call.args), 0, S)
        assert want == -1 and A.lib().iamf_hip_batch_render_packets(b.h, C.byref(call), 0, S) == want
        call.args.d_in2, call.args.in2_stream_stride, call.args.in2_frame_stride = x2.data_ptr(), 2 * fs, 2 * fs
        assert A.lib().iamf_hip_batch_render_packets(b.h, C.byref(call), 0, S) == -1
        torch.cuda.synchronize()
        fam, base, rest = _tallies(A)
        assert fam == base == rest == {} and np.array_equal(_export(b, S, st), before) and bool((pcm == 0xA5).all())
    finally:
        b.close()


def test_a_weight_of_2_to_the_minus_110_stays_unfused():
    A, G, O = _mods()
    m, oc = 6, 2
    w = np.random.default_rng(3354).uniform(0.1, 0.5, (m, oc)).astype(np.float32)
    w[4, 0] = np.float32(2.0 ** -110)
    mx, omx = R._custom(A, O, A.KIND_M2M, m, oc, w, oc)
    widths, perm = coupled(m)
    check_unfused(mx, oc, LP.ints(np.random.default_rng(3355), 3, 3, m, 1024, 3), widths, perm, 1024, [2, 1], omx=omx)


def test_other_24_bit_pairings_stay_unfused():
    mx, omx = R.matrices(6, 2, table=False)
    ints = LP.ints(np.random.default_rng(3356), 3, 3, 6, 1024, 3)
    check_unfused(mx, 2, ints, [1] * 6, list(range(6)), 1024, [2, 1], omx=omx, what="six mono runs")
    # the element's own pairing, handed over in audio-layer order (L R Ls Rs C LFE): pairs on (0,1) and (2,3), C and LFE last
    check_unfused(mx, 2, ints, [2, 2, 1, 1], list(range(6)), 1024, [2, 1], omx=omx, what="pairs on (0,1), (2,3)")
    mx2, omx2 = R.matrices(2, 2, table=False)
    check_unfused(mx2, 2, LP.ints(np.random.default_rng(3357), 3, 3, 2, 1024, 3), [1, 1], [0, 1], 1024, [2, 1], omx=omx2, what="stereo as two mono runs")


# ------------------------------------------------------------------------------------------
# totality: the forms of the older entry through the new one, and S24C through the older one
# ------------------------------------------------------------------------------------------

def test_16_bit_coupled_packets_take_the_16_bit_coupled_form():
    m, oc = 6, 2
    mx, omx = R.matrices(m, oc, table=False)
    widths, perm = coupled(m)
    check_unfused(mx, oc, LP.ints(np.random.default_rng(3360), 3, 3, m, 1024, 2), widths, perm, 1024, [2, 1], omx=omx, bps=2,
                  own={("LPCM_COUPLED", 1, m, oc, 0): 2, R.gen(m): 1})


@pytest.mark.parametrize("bps", [2, 3])
def test_mono_coded_packets_take_their_forms(bps):
    m, oc = 4, 2
    mx, omx = R.matrices(m, oc, table=False)
    own = {("LPCM" if bps == 2 else "LPCM24", 1, m, oc, 0): 2, R.gen(m): 1}
    check_unfused(mx, oc, LP.ints(np.random.default_rng(3361 + bps), 3, 3, m, 1024, bps), [1] * m, list(range(m)), 1024, [2, 1], omx=omx, bps=bps,
                  own=own)


def test_big_endian_coupled_packets_are_unpacked():
    m, oc = 6, 2
    mx, omx = R.matrices(m, oc, table=False)
    widths, perm = coupled(m)
    check_unfused(mx, oc, LP.ints(np.random.default_rng(3364), 3, 3, m, 1024, 3), widths, perm, 1024, [2, 1], omx=omx, le=False)


def test_the_older_entry_keeps_coupled_24_bit_packets_unfused():
    """iamf_hip_batch_render_lpcm on S24C packets: the unpacker and the f32 kernel, the new family's tally empty"""
    A, G, O = _mods()
    m, oc, fs = 6, 2, 1024
    mx, omx = R.matrices(m, oc, table=False)
    ints = LP.ints(np.random.default_rng(3365), 3, 3, m, fs, 3)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=16, pad=0, frame_size=fs)
    _reset(A)
    got, ns, state = _render(mx, oc, raw, L, row, fs, [2, 1], entry="lpcm")
    fam, base, rest = _tallies(A)
    assert fam == {} and rest == {} and base == {("FAST", 0, m, oc, 0): 2, R.gen(m): 1}, (fam, base, rest)
    new, ns_new, state_new = _render(mx, oc, raw, L, row, fs, [2, 1])
    fam, base, rest = _tallies(A)
    assert fam == {(FAM, 1, m, oc, 0): 2} or fam == {(FAM, 0, m, oc, 0): 2}, fam
    assert ns == ns_new and np.array_equal(state, state_new)
    for s in range(3):
        assert np.array_equal(got[s], new[s]) and np.array_equal(got[s], O.stream_run(omx, oc, planar(ints, perm)[s], fs)), s


# ------------------------------------------------------------------------------------------
# ranges and state
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("early", [1, 0])
def test_stream_ranges_advance_on_their_own(early):
    """iamf_hip_batch_render_packets over [0, 2) and [2, 5) of a 5-stream batch: the ranges take different frame counts per
    round and in one round only the first advances; per stream against the oracle, and the PCM rows outside a call's range
    keep their fill"""
    import torch
    A, G, O = _mods()
    m, oc, fs, S, F = 8, 2, 1024, 5, 4
    mx, omx = R.matrices(m, oc, table=False)
    ints = LP.ints(np.random.default_rng(3370), S, F, m, fs, 3)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=16, pad=0, frame_size=fs)
    d_raw = torch.from_numpy(fill_gaps(raw, L)).cuda()
    ranges = [(0, 2), (2, 3)]
    rounds = [(1, 2), (2, 0), (1, 2)]          # frames per range and round: 1 + 2 + 1 and 2 + 0 + 2
    st = torch.cuda.current_stream().cuda_stream
    outs = [[] for _ in range(S)]
    at = [0, 0]
    with R.environment(_variant(early)):
        _reset(A)
        b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
        try:
            def take(rows, n, s0, cnt):
                torch.cuda.synchronize()
                h = G.rows_and_rest(rows, G.DENSE, n * oc * 2, only=(s0, cnt))
                for s in range(s0, s0 + cnt):
                    outs[s].append(h[s])

            for frames in rounds:
                for r, (s0, cnt) in enumerate(ranges):
                    nf = frames[r]
                    if not nf:
                        continue
                    rows, d_pcm, stride = G.pcm_rows(S, nf * fs * oc * 2, G.DENSE, 2)
                    inp = A.LpcmInput()
                    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr() + at[r] * row, F * row, row, L
                    a = A.RenderArgs()
                    a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, d_pcm, stride, st
                    take(rows, b.render_packets(inp, a, s0, cnt), s0, cnt)
                    at[r] += nf
            for s0, cnt in ranges:
                rows, d_pcm, stride = G.pcm_rows(S, 240 * oc * 2, G.DENSE, 2)
                take(rows, b.flush_range(d_pcm, stride, st, s0, cnt), s0, cnt)
        finally:
            b.close()
        fam, base, rest = _tallies(A)
    assert at == [F, F]
    assert fam == {(FAM, early, m, oc, 0): 5} and base == {R.gen(m): 2} and rest == {}, (fam, base, rest)
    x = planar(ints, perm)
    for s in range(S):
        want = O.stream_run(omx, oc, x[s], fs)
        got = np.concatenate(outs[s]).view(np.int16).reshape(-1, oc)
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d" % s


def test_fused_unfused_f32_restart_and_import_follow_one_another_on_one_batch():
    """steps on ONE batch of 3 streams: fused, f32 (render_ex), unfused (IAMF_HIP_LPCM_UNFUSED), a refused call (reserved set;
    a NULL d_raw; d_in set) that changes nothing, fused, export -> a second batch imports -> both render the same fused call and
    flush to the same bytes; then restart of the first batch and one more fused call equal to a fresh stream's.  The whole
    equals the oracle's run over the concatenation."""
    import ctypes as C
    import synth
    import torch
    A, G, O = _mods()
    m, oc, fs, S = 6, 2, 1024, 3
    mx, omx = R.matrices(m, oc, table=False)
    rng = np.random.default_rng(3380)
    st = torch.cuda.current_stream().cuda_stream
    widths, perm = coupled(m)
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    b2 = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    outs, xs = [[] for _ in range(S)], []

    def take(pcm, n, into):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            into[s].append(h[s, :n * oc * 2].copy())

    def packet_call(bb, ints, nf, into, keep_x=True):
        raw, L, row = LP.rows(ints, 3, True, widths, perm, head=16, pad=0, frame_size=fs)
        d_raw = torch.from_numpy(raw).cuda()
        pcm = torch.zeros((S, nf * fs * oc * 2), dtype=torch.uint8, device="cuda")
        inp = A.LpcmInput()
        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
        a = A.RenderArgs()
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), nf * fs * oc * 2, st
        take(pcm, bb.render_packets(inp, a), into)
        if keep_x:
            xs.append(planar(ints, perm))
        return inp, a, pcm

    try:
        _reset(A)
        packet_call(b, LP.ints(rng, S, 2, m, fs, 3), 2, outs)
        xf = np.stack([synth.hot(3381 + s, m, fs, sigma=0.22, burst_phase=300, burst_period=900) for s in range(S)])
        d_in = torch.from_numpy(G.to_frames(xf, fs)).cuda()
        pcm = torch.zeros((S, fs * oc * 2), dtype=torch.uint8, device="cuda")
        a = A.RenderArgs()
        a.d_in, a.in_stream_stride, a.in_frame_stride = d_in.data_ptr(), m * fs, m * fs
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 1, pcm.data_ptr(), fs * oc * 2, st
        take(pcm, b.render_ex(a), outs)
        xs.append(xf.astype(np.float32))
        with R.environment(UNFUSED):
            inp, a, pcm = packet_call(b, LP.ints(rng, S, 1, m, fs, 3), 1, outs)
        # refusals: nothing is queued, allocated or changed — the state exported before and after is the same, the PCM keeps its fill
        before = _export(b, S, st)
        pcm.fill_(0xA5)
        call = A.PacketCall()
        call.in_, call.args = inp, a
        for what, edit in (("reserved", lambda c: c.reserved.__setitem__(2, 1)), ("d_in", lambda c: setattr(c.args, "d_in", d_in.data_ptr())),
                           ("d_in2", lambda c: setattr(c.args, "d_in2", d_in.data_ptr())), ("d_raw", lambda c: setattr(c.in_, "d_raw", None)),
                           ("channels", lambda c: setattr(c.in_.layout, "channels", 5))):
            bad = A.PacketCall()
            C.memmove(C.byref(bad), C.byref(call), C.sizeof(call))
            edit(bad)
            assert A.lib().iamf_hip_batch_render_packets(b.h, C.byref(bad), 0, S) == -1, what
        assert A.lib().iamf_hip_batch_render_packets(b.h, C.byref(call), 1, S) == -1      # a range past the batch's end
        torch.cuda.synchronize()
        assert np.array_equal(_export(b, S, st), before) and bool((pcm == 0xA5).all())
        packet_call(b, LP.ints(rng, S, 1, m, fs, 3), 1, outs)
        # export -> import into a second batch: both render the same call and flush to the same bytes
        sb = b.stream_state_bytes()
        d_state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
        tickets = b.export_range(0, S, d_state.data_ptr(), sb, st)
        b2.import_range(0, S, d_state.data_ptr(), sb, tickets, st)
        last = LP.ints(rng, S, 2, m, fs, 3)
        outs2 = [[] for _ in range(S)]
        packet_call(b2, last, 2, outs2, keep_x=False)
        packet_call(b, last, 2, outs)
        for bb, into in ((b, outs), (b2, outs2)):
            pcm = torch.zeros((S, 240 * oc * 2), dtype=torch.uint8, device="cuda")
            take(pcm, bb.flush(pcm.data_ptr(), 240 * oc * 2, st), into)
        fam, base, rest = _tallies(A)
        assert fam == {(FAM, 1, m, oc, 0): 4} and base == {("FAST", 0, m, oc, 0): 2, R.gen(m): 2} and rest == {}, (fam, base, rest)
        x = np.concatenate(xs, axis=2)
        for s in range(S):
            got = np.concatenate(outs[s]).view(np.int16).reshape(-1, oc)
            want = O.stream_run(omx, oc, np.ascontiguousarray(x[s]), fs)
            assert got.shape == want.shape and np.array_equal(got, want), "stream %d" % s
            tail = np.concatenate(outs2[s]).view(np.int16).reshape(-1, oc)
            assert np.array_equal(tail, want[-tail.shape[0]:]), "stream %d of the importing batch" % s
        # restart: a fresh stream
        b.restart_range(0, S, stream=st)
        fresh = LP.ints(rng, S, 1, m, fs, 3)
        outs3 = [[] for _ in range(S)]
        xs.clear()
        packet_call(b, fresh, 1, outs3)
        pcm = torch.zeros((S, 240 * oc * 2), dtype=torch.uint8, device="cuda")
        take(pcm, b.flush(pcm.data_ptr(), 240 * oc * 2, st), outs3)
        fam, base, rest = _tallies(A)
        assert fam == {(FAM, 1, m, oc, 0): 1} and base == {R.gen(m): 1} and rest == {}, (fam, base, rest)
        for s in range(S):
            got = np.concatenate(outs3[s]).view(np.int16).reshape(-1, oc)
            assert np.array_equal(got, O.stream_run(omx, oc, xs[0][s], fs)), "stream %d after the restart" % s
    finally:
        b.close()
        b2.close()


# ------------------------------------------------------------------------------------------
# where a caller may put the packets (the PK_ layouts of tests/gpu_util.py), and a caller-owned stream
# ------------------------------------------------------------------------------------------

PK_S, PK_FS, PK_F, PK_CALLS = 3, 1024, 4, [1, 3]
# which of PK_CALLS the kernel takes under each layout: the mono-coded 24-bit form's answers (tests/test_gpu_packet_layouts.py) —
# the same 4-byte grid (gpu_util.pk_grid), the same 16-byte rule for d_raw, the same 32-bit bound.  PK_GRID (strides on the
# 4-byte grid only): the call that starts at frame 0 is fused, the one that starts at frame 1 has d_raw at 16 + row + 4, off the
# 16-byte rule; PK_OFF_BASE (d_raw + 8) and PK_OFF_STRIDE (strides 2 mod 4) in none; PK_BEYOND (one step beyond B(3)) in the
# call of one frame only
PK_FUSED = {"PK_DENSE": (1, 1), "PK_PAD16": (1, 1), "PK_GRID": (1, 0), "PK_OFF_BASE": (0, 0), "PK_OFF_STRIDE": (0, 0),
            "PK_FAR_STREAMS": (1, 1), "PK_BOUND": (1, 1), "PK_BEYOND": (1, 0)}


@functools.lru_cache(maxsize=None)
def _pk_programme(m):
    ints = LP.ints(np.random.default_rng(3400 + m), PK_S, PK_F, m, PK_FS, 3)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=4, pad=4, frame_size=PK_FS)
    return raw, L, row, planar(ints, perm)


@functools.lru_cache(maxsize=None)
def _pk_reference(m, oc):
    """-> (the oracle's PCM per stream, the unfused twin's PCM per stream, what the twin's calls emitted): once per case"""
    A, G, O = _mods()
    raw, L, row, x = _pk_programme(m)
    mx, omx = R.matrices(m, oc, table=False)
    want = [O.stream_run(omx, oc, x[s], PK_FS) for s in range(PK_S)]
    with R.environment(UNFUSED):
        _reset(A)
        twin, ns, _ = _render(mx, oc, raw, L, row, PK_FS, PK_CALLS, packets=G.PK_DENSE)
        fam, base, rest = _tallies(A)
    assert fam == rest == {} and base == {("FAST", 0, m, oc, 0): len(PK_CALLS), R.gen(m): 1}, (fam, base)
    for a in want + twin:
        a.setflags(write=False)
    return want, twin, tuple(ns)


def run_placed(m, oc, early, pk):
    A, G, O = _mods()
    raw, L, row, x = _pk_programme(m)
    mx, omx = R.matrices(m, oc, table=False)
    want, twin, twin_emitted = _pk_reference(m, oc)
    fused = PK_FUSED[pk.name]
    with R.environment(_variant(early)):
        _reset(A)
        got, ns, _ = _render(mx, oc, raw, L, row, PK_FS, PK_CALLS, packets=pk)
        fam, base, rest = _tallies(A)
    base_want = {R.gen(m): 1}
    if len(fused) - sum(fused):
        base_want[("FAST", 0, m, oc, 0)] = len(fused) - sum(fused)
    assert fam == ({(FAM, early, m, oc, 0): sum(fused)} if sum(fused) else {}), (pk.name, fam)
    assert base == base_want and rest == {}, (pk.name, base, rest)
    assert tuple(ns) == twin_emitted, (ns, twin_emitted)
    for s in range(PK_S):
        assert got[s].shape == want[s].shape and np.array_equal(got[s], want[s]), "%s: stream %d against the oracle" % (pk.name, s)
        assert np.array_equal(got[s], twin[s]), "%s: stream %d against the unfused twin" % (pk.name, s)


def _pk_small():
    import gpu_util as G
    return G.PK_SMALL


def _pk_far():
    import gpu_util as G
    return G.PK_FAR


@pytest.mark.parametrize("pk", _pk_small(), ids=lambda l: l.name)
@pytest.mark.parametrize("m,oc,early", [(12, 2, 1), (6, 1, 0), (2, 2, 0)])
def test_under_every_small_packet_layout(m, oc, early, pk):
    run_placed(m, oc, early, pk)


@pytest.mark.parametrize("pk", _pk_far(), ids=lambda l: l.name)
def test_under_the_far_packet_layouts(pk):
    import torch
    try:
        run_placed(12, 2, 1, pk)
    finally:
        gc.collect()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", ["null", "same"])
def test_on_a_caller_owned_non_blocking_stream(where):
    """three calls and the flush on a side stream, a stall in front of every library call (tests/stream_util.py) on the null
    stream or on the call's own: one launch per call, all of them on the call's stream.  (stream_util.stalled stalls the
    entries its table names — the export and the flush here; the new entry's calls get the same stall by hand.)"""
    import stream_util as SU
    import torch
    A, G, O = _mods()
    where = {"null": SU.NULL, "same": SU.SAME}[where]
    m, oc, fs, calls = 6, 2, 1024, [1, 3, 2]
    ints = LP.ints(np.random.default_rng(3410), R.S, sum(calls), m, fs, 3)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=16, pad=0, frame_size=fs)
    x = planar(ints, perm)
    mx, omx = R.matrices(m, oc, table=False)
    SU.calibrate()
    _reset(A)
    stalls = []

    def stall_in_front():
        s = torch.cuda.current_stream()
        SU.assert_non_blocking(s.cuda_stream)
        ev = SU.stall(SU.torch_stream(0) if where == SU.NULL else s)
        assert not ev.query(), "the stall in front of the call had finished before the call was made"
        stalls.append(ev)

    with SU.side_stream(), SU.stalled(where) as log:
        got, ns, _ = _render(mx, oc, raw, L, row, fs, calls, before_call=stall_in_front)
    fam, base, rest = _tallies(A)
    assert len(stalls) == len(calls) and len(log) >= 2, [r.entry for r in log]
    assert fam == {(FAM, 1, m, oc, 0): len(calls)} and base == {R.gen(m): 1} and rest == {}, (fam, base, rest)
    for s in range(R.S):
        assert float(np.abs(O.render(omx, x[s], oc)).max()) > 0.95, "the programme does not drive the limiter"
        R.compare(got[s], O.stream_run(omx, oc, x[s], fs), 0, ("side stream", s))


# ------------------------------------------------------------------------------------------
# hand-over: the new family against the f32 kernel and the general kernel, every ordered pair
# ------------------------------------------------------------------------------------------

HO_S, HO_N2 = 6, 1024
HO_KERNELS = ("early", "late", "f32", "generic")
HO_ENV = {"early": {"IAMF_HIP_LP_EARLY": "1"}, "late": {"IAMF_HIP_LP_LATE": "1"}, "f32": UNFUSED, "generic": {"IAMF_HIP_FORCE_GENERIC": "1"}}


def _ho_programme(b):
    """5.1 on the 24-bit grid, six streams, one limiter phase each at the boundary b (handover_util.peaks: idle, look-ahead,
    mid-attack, release, re-trigger, edge): noise of +-500 * 256 with, per peak, one sample on L and R that takes output 0
    of the selection matrix (weight 1 on L -> 0, R -> 1) to the target level"""
    import handover_util as H
    rng = np.random.default_rng(9300 + b)
    total = b + HO_N2
    ints = (rng.integers(-500, 501, size=(HO_S, 6, total)) * 256).astype(np.int64)
    for s in range(HO_S):
        for p, level in H.peaks(H.PHASES[s], b):
            ints[s, :2, p] = int(np.ceil(level * FULL)) if level < 1.0 else FULL - 1
    return ints


def _ho_want(omx, oc, ints, b):
    A, G, O = _mods()
    x = (ints.astype(np.float64) / FULL).astype(np.float32)
    out = []
    for s in range(HO_S):
        z = O.render(omx, np.ascontiguousarray(x[s]), oc)
        y, _ = O.limiter_run(np.ascontiguousarray(z), [b, HO_N2])
        out.append(O.pack(y, 16))
    return out


def _ho_run(mx, oc, ints, b, kernels):
    """call 1 of b samples under kernels[0], call 2 of HO_N2 under kernels[1], the flush -> (PCM per stream, the exported
    state behind call 1 and behind call 2, the tallies of the two calls)"""
    import torch
    A, G, O = _mods()
    fs = 1024 if b % 1024 == 0 or b < 1024 else b        # 1088: one frame of 1088; 1000: one trimmed frame of 1024
    st = torch.cuda.current_stream().cuda_stream
    bb = A.Batch(HO_S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    outs, states, tallies = [[] for _ in range(HO_S)], [], []
    try:
        pos = 0
        for kname, n in zip(kernels, (b, HO_N2)):
            nf, ns = (1, n) if n < fs else (n // fs, 0)
            assert n <= fs or n % fs == 0
            fr = np.zeros((HO_S, nf, 6, fs), dtype=np.int64)
            seg = ints[:, :, pos:pos + n]
            if n < fs:
                fr[:, 0, :, :n] = seg
            else:
                fr[:] = seg.reshape(HO_S, 6, nf, fs).transpose(0, 2, 1, 3)
            widths, perm = coupled(6)
            inv = np.argsort(perm)                       # ints are in playback order: decoded channel d = playback inv[d]
            raw, L, row = LP.rows(np.ascontiguousarray(fr[:, :, inv, :]), 3, True, widths, perm, head=16, pad=0, frame_size=fs)
            d_raw = torch.from_numpy(raw).cuda()
            pcm = torch.zeros((HO_S, max(n, 240) * oc * 2), dtype=torch.uint8, device="cuda")
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, ns, pcm.data_ptr(), max(n, 240) * oc * 2, st
            with R.environment(HO_ENV[kname]):
                _reset(A)
                k = bb.render_packets(inp, a)
                torch.cuda.synchronize()
                tallies.append(_tallies(A))
            h = pcm.cpu().numpy()
            for s in range(HO_S):
                outs[s].append(h[s, :k * oc * 2].copy())
            states.append(_export(bb, HO_S, st))
            pos += n
        pcm = torch.zeros((HO_S, 240 * oc * 2), dtype=torch.uint8, device="cuda")
        k = bb.flush(pcm.data_ptr(), 240 * oc * 2, st)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(HO_S):
            outs[s].append(h[s, :k * oc * 2].copy())
    finally:
        bb.close()
    return [np.concatenate(o).view(np.int16).reshape(-1, oc) for o in outs], states, tallies


@pytest.mark.parametrize("b", [1024, 1088, 1000])
def test_handover_between_the_new_family_the_f32_kernel_and_the_general_kernel(b):
    """every ordered pair (A, B) of {new early, new late, unfused f32 kernel, general kernel}: A renders call 1 of b samples, B
    call 2 of 1024, the flush ends the stream.  b = 1000 is no whole number of blocks: call 1 falls to the general kernel
    whatever A says.  After each call the exported state equals a control batch's that ran both calls on the general kernel;
    the PCM equals the oracle's; a failed pair is kept and the next one runs."""
    A, G, O = _mods()
    oc = 2
    mx, omx = _selection(6, oc, [(0, 0, 1.0), (1, 1, 1.0), (2, 0, 2.0 ** -3), (3, 1, 2.0 ** -3), (4, 0, 2.0 ** -2), (5, 1, 2.0 ** -2)])
    ints = _ho_programme(b)
    want = _ho_want(omx, oc, ints, b)
    control, control_states, _ = _ho_run(mx, oc, ints, b, ("generic", "generic"))
    failed = []
    row_of = {"early": (FAM, 1, 6, oc, 0), "late": (FAM, 0, 6, oc, 0), "f32": ("FAST", 0, 6, oc, 0), "generic": R.gen(6)}
    for ka in HO_KERNELS:
        for kb in HO_KERNELS:
            try:
                got, states, tallies = _ho_run(mx, oc, ints, b, (ka, kb))
                for k, (kname, n) in enumerate(zip((ka, kb), (b, HO_N2))):
                    fam, base, rest = tallies[k]
                    rw = row_of[kname] if n % 64 == 0 else R.gen(6)
                    merged = dict(fam)
                    merged.update(base)
                    assert merged == {rw: 1} and rest == {}, ("call %d" % (k + 1), fam, base, rest)
                    assert np.array_equal(states[k], control_states[k]), "the state behind call %d against the control's" % (k + 1)
                for s in range(HO_S):
                    assert got[s].shape == want[s].shape and np.array_equal(got[s], want[s]), "stream %d against the oracle" % s
                    assert np.array_equal(got[s], control[s]), "stream %d against the control" % s
            except AssertionError as e:
                failed.append("b = %d, A = %s, B = %s: %s" % (b, ka, kb, e))
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------
# structured programmes on the 24-bit grid
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("early", [1, 0], ids=["early", "late"])
@pytest.mark.parametrize("m", [2, 6], ids=["stereo", "5.1"])
@pytest.mark.parametrize("rate", [48000, 22050, 192000])
def test_the_boundary_programmes(rate, m, early):
    """programmes.boundary_set (the eight re-trigger sweep streams, release to idle, onset after silence, loud then silence,
    silence) and attack_across_chunks on the 24-bit packet grid through a selection matrix of weight programmes.PACKET_WEIGHT,
    as the other packet-fed families run them (tests/test_gpu_rates.py)"""
    import programmes as P
    import test_gpu_programmes as TP
    import test_gpu_rates as TR
    A, G, O = _mods()
    FS, oc = TP.FS, 2
    n = FS * TR.frames_of(rate)
    progs = P.boundary_set(m, n, rate, packet_bits=24) + [("attack_across_chunks", P.on_packet_grid(P.attack_across_chunks(m, n, rate), 24))]
    ints = np.stack([P.to_packet_grid(x, 24) for _, x in progs])
    S = ints.shape[0]
    ints = np.ascontiguousarray(ints.reshape(S, m, n // FS, FS).transpose(0, 2, 1, 3))
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=16, pad=0, frame_size=FS)
    mx, omx = TP.selection(m, oc, weight=P.PACKET_WEIGHT)
    calls = list(TR.calls_of(rate))
    with R.environment(_variant(early)):
        _reset(A)
        got, ns, _ = _render(mx, oc, raw, L, row, FS, calls, rate=rate)
        fam, base, rest = _tallies(A)
    assert fam == {(FAM, early, m, oc, 0): len(calls)} and base == {R.gen(m): 1} and rest == {}, (fam, base, rest)
    x = planar(ints, perm)
    bad = []
    for s, (name, _) in enumerate(progs):
        d = TP.mismatch(got[s], O.stream_run(omx, oc, x[s], FS, rate=rate))
        if d:
            bad.append("%s: %s" % (name, d))
    assert not bad, "\n".join(["%s at %d Hz:" % (FAM, rate)] + bad)


@pytest.mark.parametrize("early", [1, 0], ids=["early", "late"])
@pytest.mark.parametrize("above", [0, 1], ids=["at_the_threshold", "one_ulp_above"])
@pytest.mark.parametrize("rate", [48000, 22050, 192000])
def test_a_plateau_at_and_one_ulp_above_the_threshold(rate, above, early):
    """DC exactly at the threshold (never a trigger) and one ulp above it (a trigger on every step): the packets hold 2^22 =
    0.5 on L and R, the matrix twice the level — a power of two times the weight, so the product is the level exactly"""
    import programmes as P
    A, G, O = _mods()
    m, oc, fs, F, S = 2, 2, 1024, 4, 3
    level = np.float32(P.THR) if not above else np.nextafter(np.float32(P.THR), np.float32(2))
    mx, omx = _selection(m, oc, [(0, 0, np.float32(2) * level), (1, 1, np.float32(2) * level)])
    ints = np.full((S, F, m, fs), 1 << 22, dtype=np.int64)
    ints[1, :, 1] = -(1 << 22)
    ints[2, :, :, :300] = 0
    x = planar(ints, [0, 1])
    assert float(np.abs(O.render(omx, x[0], oc)).max()) == float(level)
    check_fused(mx, omx, oc, ints, fs, [1, 2, 1], early, what="plateau at %d Hz" % rate, rate=rate)
