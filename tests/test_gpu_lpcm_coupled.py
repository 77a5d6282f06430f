"""-m gpu: the coupled form of the packet-fed headline kernel (render_fast_kernel<.., LP, EARLY, 2, LPC>,
iac_amd/csrc/iamf_render_lpcm_coupled.hip) behind iamf_hip_batch_render_lpcm: 16-bit packets of a channel-based element
whose L/R, Ls/Rs .. pairs are coupled sub-streams, C and LFE mono ones.

Every fused case asserts: the listing by family (iamf_hip_route_family_tally) names the instance, once per call; tables
0 .. 2 show no packet-fed row (the base tally holds the flush's GENERIC row and nothing else); every stream is bit for bit
the oracle's (oracle_lib.stream_run on ints / 2^15 — the reference's LPCM decode, pcm/IAMF_pcm_decoder.c:64-83, is exact in
f32), with PCM and n_emitted equal to a twin batch run under IAMF_HIP_LPCM_UNFUSED=1 (unpack, then the f32 kernel: the path
every such call took before), and both batches export the same stream state in front of the flush.  Tolerance 0
everywhere.  Both prefetch variants are forced by their switches, so no case depends on where the host cuts between them.
Shapes: 3-5 streams, chunks of 1024 samples, at most a few thousand samples per stream.

The forms that must stay on the old path assert the family's tally empty and PCM equal to the twin."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import lpcm_util as LP
import route_cases as R

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_FACADE_UNPACK", "IAMF_HIP_GROUP_UNPACK", "IAMF_HIP_NO_WIDE4")
FAM = "LPCM_COUPLED"
COUPLED_M = [2, 6, 8, 10, 12]
PACKET_FED = ("LPCM", "LPCM24", "FANOUT_LPCM", FAM)


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
    A.route_family_tally(FAM, reset=True)


def _tallies(A):
    """-> (the coupled family's tally, table 0, table 1, table 2), all reset"""
    return A.route_family_tally(FAM, reset=True), A.route_tally(), A.route_tally_ext(), A.route_table_tally(2, reset=True)


def _no_packet_rows(*tables):
    return not [k for t in tables for k in t if k[0] in PACKET_FED]


def coupled(m):
    """-> (widths, perm) of lpcm_util.rows for a loudspeaker layout of m channels: sub-streams in audio-layer order (the
    coupled pairs, then C and LFE), perm[p] = the decoded channel playback channel p takes (L R C LFE, then the pairs); a mono
    element is its one mono sub-stream"""
    if m <= 2:
        return [m], list(range(m))
    return [2] * ((m - 2) // 2) + [1, 1], [0, 1, m - 2, m - 1] + list(range(2, m - 2))


def planar(ints, perm):
    S, F, m, fs = ints.shape
    x = (ints[:, :, perm, :].astype(np.float64) / 32768.0).astype(np.float32)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)


def drive_limiter(O, omx, oc, ints, perm):
    """the packets' samples scaled, stream by stream, so that the rendered peak is about 1.3 (threshold: -1 dB = 0.89) where
    it is lower, as route_cases.drive_limiter does for f32 programmes: the scale comes from the oracle's rendering, never
    from the code under test (samples that leave the 16-bit range are clipped; the callers assert the peak they got)"""
    ints = ints.copy()
    for s in range(ints.shape[0]):
        for _ in range(4):          # (clipping takes some of the peak back: scaled again where it took too much)
            peak = float(np.abs(O.render(omx, planar(ints[s:s + 1], perm)[0], oc)).max())
            assert peak > 0.0
            if peak >= 1.1:
                break
            ints[s] = np.clip(np.rint(ints[s] * (1.3 / peak)), -32768, 32767).astype(np.int64)
    return ints


def fill_gaps(raw, L):
    """every byte of the rows that belongs to no run: 0x7F / 0x80 alternating (a load that strays reads a large sample)"""
    A, G, O = _mods()
    used = G.packet_run_mask(L, raw.shape[-1])
    fill = np.where(np.arange(raw.shape[-1]) % 2 == 0, 0x7F, 0x80).astype(np.uint8)
    return np.where(used[None, None, :], raw, fill[None, None, :])


def _render(mx, oc, raw, L, row, fs, calls, first=0, n_samples=0, args_hook=None, batch_hook=None, fmt=None):
    """-> (the streams as gpu_util._view gives them, what every call and the flush emitted, the exported state of every
    stream in front of the flush)"""
    import torch
    A, G, O = _mods()
    S, F, _ = raw.shape
    d_raw = torch.from_numpy(raw).cuda()
    fmt = A.FMT_S16 if fmt is None else fmt
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=fmt, limiter=True)
    keep = batch_hook(b) if batch_hook else None
    st = torch.cuda.current_stream().cuda_stream
    outs, ns, f0 = [[] for _ in range(S)], [], 0
    for nf in calls:
        cap = max(nf * fs, 240) * oc * bps
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        inp = A.LpcmInput()
        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = d_raw.data_ptr() + f0 * row, F * row, row
        inp.first_sample, inp.layout = first, L
        a = A.RenderArgs()
        a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n_samples, pcm.data_ptr(), cap, st
        held = args_hook(a, nf) if args_hook else None
        n = b.render_lpcm(inp, a)
        torch.cuda.synchronize()
        del held
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(h[s, :n * oc * bps].copy())
        ns.append(n)
        f0 += nf
    sb = b.stream_state_bytes()
    d_state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
    b.export_range(0, S, d_state.data_ptr(), sb, st)
    torch.cuda.synchronize()
    state = d_state.cpu().numpy()
    pcm = torch.zeros((S, 240 * oc * bps), dtype=torch.uint8, device="cuda")
    n = b.flush(pcm.data_ptr(), 240 * oc * bps, st)
    torch.cuda.synchronize()
    h = pcm.cpu().numpy()
    for s in range(S):
        outs[s].append(h[s, :n * oc * bps].copy())
    ns.append(n)
    b.close()
    del keep
    return [G._view(np.concatenate(o), sum(ns), oc, fmt) for o in outs], ns, state


def check_fused(mx, omx, oc, ints, fs, calls, early, head=16, pad=0, first=0, n_samples=0, fill=False, what="", bd=16, check=None,
                fused=True, hot=False):
    """early None: no switch, the variant is whichever the host's rule picks; fused False: the library unpacks this call itself
    (same PCM, the f32 kernel's row); hot: the precondition that the programme drives the limiter is asserted"""
    import test_gpu_programmes as TP
    A, G, O = _mods()
    fmt = {16: A.FMT_S16, 24: A.FMT_S24, 32: A.FMT_S32, -32: A.FMT_F32}[bd]
    S, F, m, _ = ints.shape
    widths, perm = coupled(m)
    if hot:
        ints = drive_limiter(O, omx, oc, ints, perm)
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=head, pad=pad, frame_size=fs)
    if fill:
        raw = fill_gaps(raw, L)
    with R.environment(_variant(early)):
        _reset(A)
        got, ns, state = _render(mx, oc, raw, L, row, fs, calls, first, n_samples, fmt=fmt)
        fam, base, ext, t2 = _tallies(A)
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        twin, ns_twin, state_twin = _render(mx, oc, raw, L, row, fs, calls, first, n_samples, fmt=fmt)
        fam_twin, base_twin, ext_twin, t2_twin = _tallies(A)
    if early is None:      # whichever variant the host's rule picks for this size (lpcm_coupled_early, render_route.hpp)
        assert len(fam) == 1 and next(iter(fam))[1] in (0, 1), (what, fam)
    variant = next(iter(fam))[1] if early is None and fam else early
    f32 = {("FAST", 0, m, oc, 0): len(calls), R.gen(m): 1}
    if fused:
        assert fam == {(FAM, variant, m, oc, 0): len(calls)}, (what, fam)
        assert base == {R.gen(m): 1} and ext == {} and t2 == {}, (what, base, ext, t2)
    else:
        assert fam == {} and base == f32 and ext == {} and t2 == {}, (what, fam, base, ext, t2)
    assert fam_twin == {} and base_twin == f32 and ext_twin == {} and t2_twin == {}, (what, fam_twin, base_twin)
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
        want = TP.oracle_stream(O, omx, oc, x[s], ofs, bd)
        assert TP.mismatch(got[s], want) is None, (what, "stream %d against the oracle" % s, TP.mismatch(got[s], want))
        assert TP.mismatch(got[s], twin[s]) is None, (what, "stream %d against the unfused twin" % s, TP.mismatch(got[s], twin[s]))


@pytest.mark.parametrize("table", [False, True], ids=["dense", "table"])
@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("oc", [1, 2])
@pytest.mark.parametrize("m", COUPLED_M)
def test_every_instance(m, oc, early, table):
    """dense: a seeded matrix with a different weight for every (channel, slot) — a symmetric down-mix into mono would not
    notice L and R swapped; table: the reference's layout -> layout matrix"""
    mx, omx = R.matrices(m, oc, table=table)
    ints = LP.ints(np.random.default_rng(2600 + 10 * m + oc), 3, 3, m, 1024, 2)
    check_fused(mx, omx, oc, ints, 1024, [2, 1], early, hot=True, what="table" if table else "dense")


def test_the_dense_matrix_tells_left_from_right():
    for m in COUPLED_M:
        for oc in (1, 2):
            mx, _ = R.matrices(m, oc, table=False)
            w = np.ctypeslib.as_array(mx.mat, shape=(m * oc,))
            assert len(set(np.abs(w).tolist())) == m * oc, (m, oc)


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("m", [6, 12])
def test_chunks_straddle_frames_and_the_last_chunk_is_short(m, early):
    # 192-sample frames, 11 of them: calls of 1152 and 960 samples, chunks of 1024 + 128 and of 960, a lane's frame by division
    mx, omx = R.matrices(m, 2, table=False)
    ints = LP.ints(np.random.default_rng(2664 + m), 3, 11, m, 192, 2)
    check_fused(mx, omx, 2, ints, 192, [6, 5], early, hot=True)


@pytest.mark.parametrize("early", [1, 0])
def test_sign_and_carry_patterns_in_every_position_of_the_quad_and_both_halves(early):
    """-2^15, 2^15 - 1, -1, 0, 1, 0x7F00 and 0x00FF with period 7 against the quad's 4, each channel one step behind its
    neighbour: every value sits in every sample-frame of a lane's 16 bytes, in the low half (L) and in the high half (R), next
    to every other — +32767 beside -32768, -1 beside 0 among them.  A selection matrix at gain 1/4 keeps the limiter idle, so
    a wrong bit of the conversion — a borrow from the neighbouring half — is a wrong bit of the PCM."""
    A, G, O = _mods()
    vals = np.array([-32768, 32767, -1, 0, 1, 0x7F00, 0x00FF], dtype=np.int64)
    m, oc, fs, F, S = 6, 2, 1024, 3, 3
    i = np.arange(F * fs)
    ints = np.zeros((S, F, m, fs), dtype=np.int64)
    for s in range(S):
        for c in range(m):
            ints[s, :, c, :] = vals[(i + c + 2 * s) % 7].reshape(F, fs)
    w = np.zeros((m, oc), dtype=np.float32)
    w[0, 0] = w[1, 1] = 0.25                  # L, R
    w[4, 0] = w[5, 1] = 2.0 ** -9             # Ls, Rs: a second product per slot below the first, every bit of both counts
    w[2, 0] = w[3, 1] = 2.0 ** -18            # C, LFE
    mx, omx = R._custom(A, O, A.KIND_M2M, m, oc, w, oc)
    check_fused(mx, omx, oc, ints, fs, [1, 2], early, head=8, pad=8, fill=True)


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("m,first,fused", [(2, 2, True), (2, 6, True), (2, 1, False), (6, 4, True), (6, 2, False)])
def test_a_trimmed_frame(m, first, fused, early):
    """a pair's run is on the 8-byte grid from every even first sample; C and LFE from every fourth.  Off it the library
    unpacks the call itself: the same PCM."""
    mx, omx = R.matrices(m, 2, table=False)
    ints = LP.ints(np.random.default_rng(2665 + m), 4, 1, m, 1024, 2)
    check_fused(mx, omx, 2, ints, 1024, [1], early, first=first, n_samples=512, fused=fused)


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("m", [2, 12])
def test_pair_runs_that_are_only_8_byte_aligned(m, early):
    """head 8, pad 8: the runs start at 8, 16 mod 16 in turn; the bytes between them are 0x7F / 0x80 and every run's first
    and last sample-frame is at the extremes: a load that starts or ends off its run shows"""
    mx, omx = R.matrices(m, 2, table=False)
    ints = LP.ints(np.random.default_rng(2666 + m), 3, 3, m, 1024, 2, level=0.2)
    ints[:, :, 0::2, 0], ints[:, :, 1::2, 0] = 32767, -32768
    ints[:, :, 0::2, -1], ints[:, :, 1::2, -1] = -32768, 32767
    widths, perm = coupled(m)
    _, L, _ = LP.rows(ints, 2, True, widths, perm, head=8, pad=8, frame_size=1024)
    offs = [L.src_offset[c] for c in range(m) if L.src_step[c] == 4 and c % 2 == 0]
    assert all(o % 8 == 0 for o in offs) and any(o % 16 == 8 for o in offs)
    check_fused(mx, omx, 2, ints, 1024, [2, 1], early, head=8, pad=8, fill=True)


@pytest.mark.parametrize("m,oc,early", [(12, 2, 1), (12, 2, 0), (6, 1, 1)])
@pytest.mark.parametrize("bd", [24, 32, -32])
def test_into_s24_s32_and_f32_pcm(m, oc, early, bd):
    mx, omx = R.matrices(m, oc, table=False)
    ints = LP.ints(np.random.default_rng(2700 + 10 * m + oc), 3, 3, m, 1024, 2)
    check_fused(mx, omx, oc, ints, 1024, [2, 1], early, bd=bd, what="bd %d" % bd)


@pytest.mark.parametrize("early", [0, 1, None], ids=["late", "early", "the_hosts_rule"])
def test_1025_streams(early):
    """more workgroups than four a CU, where the mono-coded form switches to its late variant: the late variant, the early
    one and whichever the host's rule picks with no switch set (lpcm_coupled_early, render_route.hpp); the first, the 1024th
    and the 1025th stream"""
    mx, omx = R.matrices(2, 2, table=False)
    ints = LP.ints(np.random.default_rng(2720), 1025, 1, 2, 1024, 2)
    check_fused(mx, omx, 2, ints, 1024, [1], early, check=[0, 1023, 1024])


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
    ints = LP.ints(np.random.default_rng(2730 + n_samples), S, F, m, fs, 2)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=16, pad=0, frame_size=fs)
    raw = fill_gaps(raw, L)
    calls, trims = [1, 1, 1], {0: (first, n_samples)}

    def run(env):
        emitted = []
        with R.environment(env):
            _reset(A)
            got = LP.render_lpcm(mx, oc, raw, L, row, fs, calls, trims=trims, emitted=emitted)
            return (got, emitted) + _tallies(A)

    got, ns, fam, base, ext, t2 = run(_variant(early))
    twin, ns_twin, fam_twin, base_twin, ext_twin, t2_twin = run({"IAMF_HIP_LPCM_UNFUSED": "1"})
    fused = [pos >= 240 or pos % 16 == 0 for pos in (n_samples, n_samples + fs)]     # where the whole-frame calls start
    general = 1 + fused.count(False) + 1                                               # the trimmed call, ..., the flush
    assert fam == ({(FAM, early, m, oc, 0): fused.count(True)} if any(fused) else {}), fam
    assert base == {R.gen(m): general} and ext == t2 == {}, (base, ext, t2)
    want_twin = {R.gen(m): general}
    if any(fused):
        want_twin[("FAST", 0, m, oc, 0)] = fused.count(True)
    assert fam_twin == ext_twin == t2_twin == {} and base_twin == want_twin, (fam_twin, base_twin)
    assert ns == ns_twin, (ns, ns_twin)
    x = planar(ints, perm)
    kept = np.ascontiguousarray(np.concatenate([x[:, :, first:first + n_samples], x[:, :, fs:]], axis=2))
    for s in range(S):
        want = O.stream_run(omx, oc, kept[s], fs)
        g = got[s].view(np.int16).reshape(-1, oc)
        assert g.shape == want.shape and np.array_equal(g, want), "stream %d against the oracle" % s
        assert np.array_equal(got[s], twin[s]), "stream %d against the unfused twin" % s


@pytest.mark.parametrize("early", [1, 0])
def test_stream_ranges_advance_on_their_own(early):
    """iamf_hip_batch_render_lpcm_range over [0, 2) and [2, 5) of a 5-stream batch: the ranges take different frame counts
    per round and in one round only the first advances; per stream against the oracle, and the PCM rows outside a call's
    range keep their fill"""
    import torch
    A, G, O = _mods()
    m, oc, fs, S, F = 8, 2, 1024, 5, 4
    mx, omx = R.matrices(m, oc, table=False)
    ints = LP.ints(np.random.default_rng(2740), S, F, m, fs, 2)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=16, pad=0, frame_size=fs)
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
                    take(rows, b.render_lpcm_range(inp, a, s0, cnt), s0, cnt)
                    at[r] += nf
            for s0, cnt in ranges:
                rows, d_pcm, stride = G.pcm_rows(S, 240 * oc * 2, G.DENSE, 2)
                take(rows, b.flush_range(d_pcm, stride, st, s0, cnt), s0, cnt)
        finally:
            b.close()
        fam, base, ext, t2 = _tallies(A)
    assert at == [F, F]
    assert fam == {(FAM, early, m, oc, 0): 5} and base == {R.gen(m): 2} and ext == t2 == {}, (fam, base, ext, t2)
    x = planar(ints, perm)
    for s in range(S):
        want = O.stream_run(omx, oc, x[s], fs)
        got = np.concatenate(outs[s]).view(np.int16).reshape(-1, oc)
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d" % s


def _one_batch_sequence(m, oc, steps, fam_want, base_want):
    """steps: [(kind, frames)] on ONE batch, kind in "coupled" (the element's canonical packets), "mono" (the same element
    as mono sub-streams), "unfused" (canonical packets under IAMF_HIP_LPCM_UNFUSED=1), "f32" (render_ex); then the flush.  The
    whole equals the oracle's run over the concatenation: the persisted state is the same whichever kernel left it."""
    import synth
    import torch
    A, G, O = _mods()
    fs, S = 1024, 3
    mx, omx = R.matrices(m, oc, table=False)
    rng = np.random.default_rng(2770 + m)
    st = torch.cuda.current_stream().cuda_stream
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    outs, xs = [[] for _ in range(S)], []

    def take(pcm, n):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(h[s, :n * oc * 2].copy())

    def lpcm_call(ints, widths, perm, nf):
        raw, L, row = LP.rows(ints, 2, True, widths, perm, head=16, pad=0, frame_size=fs)
        d_raw = torch.from_numpy(raw).cuda()
        pcm = torch.zeros((S, nf * fs * oc * 2), dtype=torch.uint8, device="cuda")
        inp = A.LpcmInput()
        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
        a = A.RenderArgs()
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), nf * fs * oc * 2, st
        take(pcm, b.render_lpcm(inp, a))
        xs.append(planar(ints, perm))

    _reset(A)
    for k, (kind, nf) in enumerate(steps):
        if kind == "f32":
            xf = np.stack([synth.hot(2771 + 10 * k + s, m, nf * fs, sigma=0.22, burst_phase=300, burst_period=900) for s in range(S)])
            d_in = torch.from_numpy(G.to_frames(xf, fs)).cuda()
            pcm = torch.zeros((S, nf * fs * oc * 2), dtype=torch.uint8, device="cuda")
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = d_in.data_ptr(), nf * m * fs, m * fs
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), nf * fs * oc * 2, st
            take(pcm, b.render_ex(a))
            xs.append(xf.astype(np.float32))
            continue
        ints = LP.ints(rng, S, nf, m, fs, 2)
        widths, perm = ([1] * m, list(range(m))) if kind == "mono" else coupled(m)
        with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"} if kind == "unfused" else {}):
            lpcm_call(ints, widths, perm, nf)
    pcm = torch.zeros((S, 240 * oc * 2), dtype=torch.uint8, device="cuda")
    take(pcm, b.flush(pcm.data_ptr(), 240 * oc * 2, st))
    b.close()
    fam, base, ext, t2 = _tallies(A)
    assert fam == fam_want and base == base_want and ext == t2 == {}, (fam, base, ext, t2)
    x = np.concatenate(xs, axis=2)
    for s in range(S):
        got = np.concatenate(outs[s]).view(np.int16).reshape(-1, oc)
        want = O.stream_run(omx, oc, np.ascontiguousarray(x[s]), fs)
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d" % s


def test_fused_f32_unfused_mono_coded_and_coupled_calls_follow_one_another_on_one_batch():
    m, oc = 6, 2
    _one_batch_sequence(m, oc, [("coupled", 2), ("f32", 2), ("unfused", 1), ("mono", 1), ("coupled", 2)],
                        {(FAM, 1, m, oc, 0): 2}, {("FAST", 0, m, oc, 0): 3, R.gen(m): 1})


def test_a_mono_element_keeps_the_mono_coded_form():
    """M = 1 (a mono channel-based element: one mono sub-stream) is the 16-bit family's, as before: fused, f32, unfused, fused"""
    m, oc = 1, 2
    _one_batch_sequence(m, oc, [("mono", 2), ("f32", 1), ("unfused", 1), ("mono", 1)],
                        {}, {("LPCM", 1, m, oc, 0): 2, ("FAST", 0, m, oc, 0): 2, R.gen(m): 1})


# ------------------------------------------------------------------------------------------
# forms that stay on the old path
# ------------------------------------------------------------------------------------------

def check_unfused(mx, oc, ints, widths, perm, fs, calls, omx=None, args_hook=None, batch_hook=None, kernel=("FAST", 0), what=""):
    """no packet-fed row anywhere, the f32 path's kernel runs, the PCM is the twin's (and the oracle's where one is given)"""
    A, G, O = _mods()
    S, F, m, _ = ints.shape
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=16, pad=0, frame_size=fs)
    _reset(A)
    got, ns, state = _render(mx, oc, raw, L, row, fs, calls, args_hook=args_hook, batch_hook=batch_hook)
    fam, base, ext, t2 = _tallies(A)
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        twin, ns_twin, state_twin = _render(mx, oc, raw, L, row, fs, calls, args_hook=args_hook, batch_hook=batch_hook)
        fam_twin, base_twin, _, _ = _tallies(A)
    assert fam == fam_twin == {} and ext == t2 == {}, (what, fam, ext, t2)
    assert _no_packet_rows(base) and base == base_twin, (what, base, base_twin)
    if kernel:
        assert base == {kernel + (m, oc, 0): len(calls), R.gen(m): 1}, (what, base)
    assert ns == ns_twin and np.array_equal(state, state_twin)
    for s in range(S):
        assert np.array_equal(got[s], twin[s]), (what, "stream %d against the twin" % s)
        if omx is not None:
            want = O.stream_run(omx, oc, planar(ints, perm)[s], fs)
            assert np.array_equal(got[s], want), (what, "stream %d against the oracle" % s)


def test_a_5_1_of_six_mono_substreams_stays_unfused():
    mx, omx = R.matrices(6, 2, table=False)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2780), 3, 3, 6, 1024, 2), [1] * 6, list(range(6)), 1024, [2, 1], omx=omx)


def test_a_stereo_of_two_mono_substreams_stays_unfused():
    mx, omx = R.matrices(2, 2, table=False)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2781), 3, 3, 2, 1024, 2), [1, 1], [0, 1], 1024, [2, 1], omx=omx)


def test_a_5_1_whose_pairs_sit_on_other_channels_stays_unfused():
    # the element's own pairing, handed over in audio-layer order (L R Ls Rs C LFE): pairs on (0,1) and (2,3), C and LFE last
    mx, omx = R.matrices(6, 2, table=False)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2782), 3, 3, 6, 1024, 2), [2, 2, 1, 1], list(range(6)), 1024, [2, 1], omx=omx)


def test_a_coupled_element_into_5_1_stays_unfused():
    # 7.1.4 into Sound System B, as tests/test_gpu_lpcm.py renders it into J: a wide kernel behind the unpacker
    A, G, O = _mods()
    mx, omx = A.get_m2m_matrix(A.SS["L714"], A.SS["B"]), O.get_m2m(O.SS["L714"], O.SS["B"])
    widths, perm = coupled(12)
    check_unfused(mx, 6, LP.ints(np.random.default_rng(2783), 3, 3, 12, 1024, 2), widths, perm, 1024, [2, 1], omx=omx, kernel=None)


def test_a_weight_of_2_to_the_minus_110_stays_unfused():
    A, G, O = _mods()
    m, oc = 6, 2
    w = np.random.default_rng(2784).uniform(0.1, 0.5, (m, oc)).astype(np.float32)
    w[4, 0] = np.float32(2.0 ** -110)
    mx, omx = R._custom(A, O, A.KIND_M2M, m, oc, w, oc)
    widths, perm = coupled(m)
    check_unfused(mx, oc, LP.ints(np.random.default_rng(2785), 3, 3, m, 1024, 2), widths, perm, 1024, [2, 1], omx=omx)


def test_a_call_with_an_output_ramp_stays_unfused():
    import torch
    mx, omx = R.matrices(6, 2, table=False)
    S, fs = 3, 1024

    def ramp(a, nf):
        r = torch.from_numpy(np.linspace(1.0, 0.5, S * nf * fs, dtype=np.float32).reshape(S, nf * fs)).cuda()
        a.d_output_ramp, a.ramp_stream_stride = r.data_ptr(), nf * fs
        return r

    widths, perm = coupled(6)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2786), S, 3, 6, fs, 2), widths, perm, fs, [2, 1], args_hook=ramp, kernel=("FAST", 1))


def test_a_batch_with_a_second_element_stays_unfused():
    import torch
    mx, omx = R.matrices(6, 2, table=False)
    mx2, _ = R.matrices(2, 2)
    S, fs = 3, 1024

    def second(b):
        b.set_second_element(mx2)
        return mx2

    def in2(a, nf):
        x2 = torch.from_numpy(np.random.default_rng(2790 + nf).uniform(-0.2, 0.2, (S, nf, 2, fs)).astype(np.float32)).cuda()
        a.d_in2, a.in2_stream_stride, a.in2_frame_stride = x2.data_ptr(), nf * 2 * fs, 2 * fs
        return x2

    widths, perm = coupled(6)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2787), S, 3, 6, fs, 2), widths, perm, fs, [2, 1], args_hook=in2, batch_hook=second,
                  kernel=("FAST", 1))


def test_the_fanout_entry_keeps_coupled_packets_on_one_unpack_and_the_f32_fanout():
    """a coupled 5.1 into {A, mono}: (2, 0, 1) as before, and every member equals its single call — which is now a call of
    the coupled kernel"""
    import torch
    A, G, O = _mods()
    m, fs, S, K, nf = 6, 1024, 3, 2, 2
    ocs = [2, 1]
    mxs = [R.matrices(m, oc) for oc in ocs]
    ints = LP.ints(np.random.default_rng(2788), S, nf, m, fs, 2)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=8, pad=8, frame_size=fs)
    d_raw = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    batches = [A.Batch(S, mxs[j][0], ocs[j], frame_size=fs, out_format=A.FMT_S16, limiter=True) for j in range(K)]
    pcms = [torch.zeros((S, nf * fs * ocs[j] * 2), dtype=torch.uint8, device="cuda") for j in range(K)]
    inp = A.LpcmInput()
    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
    _reset(A)
    emitted, report = A.render_fanout_lpcm(batches, inp, nf, [p.data_ptr() for p in pcms], [nf * fs * oc * 2 for oc in ocs], stream=st)
    torch.cuda.synchronize()
    assert report == (K, 0, 1), report
    fam, base, ext, t2 = _tallies(A)
    assert fam == ext == t2 == {} and base == {("FANOUT", 0, m, 0, K): 1}, (fam, base, ext, t2)
    x = planar(ints, perm)
    for j in range(K):
        h = pcms[j].cpu().numpy()
        batches[j].close()
        single, ns, _ = _render(mxs[j][0], ocs[j], raw, L, row, fs, [nf])
        fam, base, _, _ = _tallies(A)
        assert fam == {(FAM, 1, m, ocs[j], 0): 1} and base == {R.gen(m): 1}, (j, fam, base)
        assert ns[0] == emitted[j]
        for s in range(S):
            got = h[s, :emitted[j] * ocs[j] * 2].view(np.int16).reshape(-1, ocs[j])
            want = O.stream_run(mxs[j][1], ocs[j], x[s], fs, flush=False)
            assert np.array_equal(got, want), (j, s, "against the oracle")
            assert np.array_equal(got, single[s][:emitted[j]]), (j, s, "against the single call")


# ------------------------------------------------------------------------------------------
# where a caller may put the packets (the PK_ layouts of tests/gpu_util.py), and a caller-owned stream
# ------------------------------------------------------------------------------------------

PK_S, PK_FS, PK_F, PK_CALLS = 3, 1024, 4, [1, 3]
# which of PK_CALLS the coupled kernel takes under each layout: the 16-bit form's answers (tests/test_gpu_packet_layouts.py) —
# the same 8-byte grid, the same 16-byte rule for d_raw, the same 32-bit bound
PK_FUSED = {"PK_DENSE": (1, 1), "PK_PAD16": (1, 1), "PK_GRID": (1, 0), "PK_OFF_BASE": (0, 0), "PK_OFF_STRIDE": (0, 0),
            "PK_FAR_STREAMS": (1, 1), "PK_BOUND": (1, 1), "PK_BEYOND": (1, 0)}


@functools.lru_cache(maxsize=None)
def _pk_programme(m):
    ints = LP.ints(np.random.default_rng(2800 + m), PK_S, PK_F, m, PK_FS, 2)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=8, pad=8, frame_size=PK_FS)
    return raw, L, row, planar(ints, perm)


@functools.lru_cache(maxsize=None)
def _pk_reference(m, oc):
    """-> (the oracle's PCM per stream, the unfused twin's bytes per stream, what the twin's calls emitted): once per case"""
    A, G, O = _mods()
    raw, L, row, x = _pk_programme(m)
    mx, omx = R.matrices(m, oc, table=False)
    want = [O.stream_run(omx, oc, x[s], PK_FS) for s in range(PK_S)]
    emitted = []
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        _reset(A)
        twin = LP.render_lpcm(mx, oc, raw, L, row, PK_FS, PK_CALLS, packets=G.PK_DENSE, emitted=emitted)
        fam, base, ext, t2 = _tallies(A)
    assert fam == ext == t2 == {} and base == {("FAST", 0, m, oc, 0): len(PK_CALLS), R.gen(m): 1}, (fam, base)
    for a in want + twin:
        a.setflags(write=False)
    return want, twin, tuple(emitted)


def run_placed(m, oc, early, pk):
    A, G, O = _mods()
    raw, L, row, x = _pk_programme(m)
    mx, omx = R.matrices(m, oc, table=False)
    want, twin, twin_emitted = _pk_reference(m, oc)
    fused = PK_FUSED[pk.name]
    emitted = []
    with R.environment(_variant(early)):
        _reset(A)
        got = LP.render_lpcm(mx, oc, raw, L, row, PK_FS, PK_CALLS, packets=pk, emitted=emitted)
        fam, base, ext, t2 = _tallies(A)
    base_want = {R.gen(m): 1}
    if len(fused) - sum(fused):
        base_want[("FAST", 0, m, oc, 0)] = len(fused) - sum(fused)
    assert fam == ({(FAM, early, m, oc, 0): sum(fused)} if sum(fused) else {}), (pk.name, fam)
    assert base == base_want and ext == t2 == {}, (pk.name, base, ext, t2)
    assert tuple(emitted) == twin_emitted, (emitted, twin_emitted)
    for s in range(PK_S):
        g = got[s].view(np.int16).reshape(-1, oc)
        assert g.shape == want[s].shape and np.array_equal(g, want[s]), "%s: stream %d against the oracle" % (pk.name, s)
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
    stream or on the call's own: one launch per call, all of them on the call's stream"""
    import stream_util as SU
    A, G, O = _mods()
    where = {"null": SU.NULL, "same": SU.SAME}[where]
    m, oc, fs, calls = 6, 2, 1024, [1, 3, 2]
    ints = LP.ints(np.random.default_rng(2810), R.S, sum(calls), m, fs, 2)
    widths, perm = coupled(m)
    raw, L, row = LP.rows(ints, 2, True, widths, perm, head=16, pad=0, frame_size=fs)
    x = planar(ints, perm)
    mx, omx = R.matrices(m, oc, table=False)
    SU.calibrate()
    _reset(A)
    with SU.side_stream(), SU.stalled(where) as log:
        got = LP.render_lpcm(mx, oc, raw, L, row, fs, calls)
    fam, base, ext, t2 = _tallies(A)
    assert len(log) >= len(calls) + 1, [r.entry for r in log]
    assert fam == {(FAM, 1, m, oc, 0): len(calls)} and base == {R.gen(m): 1} and ext == t2 == {}, (fam, base, ext, t2)
    for s in range(R.S):
        assert float(np.abs(O.render(omx, x[s], oc)).max()) > 0.95, "the programme does not drive the limiter"
        R.compare(got[s].view(np.int16).reshape(-1, oc), O.stream_run(omx, oc, x[s], fs), 0, ("side stream", s))


# ------------------------------------------------------------------------------------------
# callers of the reference API: the stored reference-decoded goldens
# ------------------------------------------------------------------------------------------

def _decoder_lib():
    import iac_amd
    lib = C.CDLL(iac_amd.lib_path())   # the prototypes group_decode_all and open_handle rely on (test_gpu_group's fixture)
    lib.IAMF_decoder_open.restype = C.c_void_p
    lib.IAMF_decoder_close.argtypes = [C.c_void_p]
    lib.IAMF_decoder_configure.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.IAMF_decoder_decode.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_uint32), C.c_void_p]
    lib.IAMF_decoder_output_layout_set_sound_system.argtypes = [C.c_void_p, C.c_int]
    lib.IAMF_decoder_output_layout_set_binaural.argtypes = [C.c_void_p]
    lib.IAMF_decoder_set_normalization_loudness.argtypes = [C.c_void_p, C.c_float]
    lib.IAMF_decoder_set_bit_depth.argtypes = [C.c_void_p, C.c_uint32]
    lib.IAMF_decoder_peak_limiter_enable.argtypes = [C.c_void_p, C.c_uint32]
    lib.IAMF_decoder_peak_limiter_set_threshold.argtypes = [C.c_void_p, C.c_float]
    lib.IAMF_decoder_set_sampling_rate.argtypes = [C.c_void_p, C.c_uint32]
    lib.IAMF_decoder_set_pts.argtypes = [C.c_void_p, C.c_int64, C.c_uint32]
    lib.IAMF_layout_sound_system_channels_count.argtypes = [C.c_int]
    lib.iamf_hip_decoder_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.iamf_hip_decoder_group_decode.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    lib.iamf_hip_decoder_group_destroy.argtypes = [C.c_void_p]
    lib.iamf_hip_decoder_group_destroy.restype = None
    return lib


def _packet_tallies(A):
    """-> {family: launches} of the packet-fed families, reset"""
    out = {}
    for f in PACKET_FED:
        out[f] = sum(A.route_family_tally(f, reset=True).values())
    return out


def _decode(golden, name):
    import e2e_cases as E
    import iac_amd
    from decoder_driver import decode_stream
    A, G, O = _mods()
    case = E.CASES[name]
    stream, _ = E.build(name)
    lib = C.CDLL(iac_amd.lib_path())
    _reset(A)
    A.route_family_tally("LPCM", reset=True)
    pcm, rets = decode_stream(lib, stream, case["layout"], bit_depth=case.get("bit_depth", 16), out_rate=case.get("out_rate", 0),
                              loudness=case.get("loudness", 0.0), limiter=case.get("limiter", True), threshold=case.get("threshold", -1.0))
    tallies = _packet_tallies(A)
    want = golden.npz("e2e")[name]
    assert list(rets) == list(golden.npz("e2e")[name + "_rets"]), name
    assert pcm.shape == want.shape and np.array_equal(pcm, want), name
    return tallies


FACADE = [("stereo_A_s16", FAM), ("stereo_fs128", FAM), ("l51_A_s16", FAM), ("l714_A_s16", FAM), ("l714_mono_s16", FAM),
          ("mono_A_s16", "LPCM"), ("stereo_trim", FAM)]


@pytest.mark.parametrize("name,family", FACADE, ids=[n for n, _ in FACADE])
def test_a_single_handle_on_a_channel_based_stream_runs_the_fused_kernel(golden, name, family):
    t = _decode(golden, name)
    assert t[family] > 0 and not [f for f in t if f != family and t[f]], (name, t)


@pytest.mark.parametrize("name", [n for n, _ in FACADE])
def test_a_single_handle_that_unpacks_first_gives_the_same_bytes(golden, name, monkeypatch):
    monkeypatch.setenv("IAMF_HIP_FACADE_UNPACK", "1")
    t = _decode(golden, name)
    assert not any(t.values()), (name, t)


def test_a_24_bit_coupled_stream_still_decodes_unfused(golden):
    t = _decode(golden, "stereo_in24le")
    assert not any(t.values()), t


@pytest.mark.parametrize("unpack_first", [False, True])
def test_a_group_of_four_handles_on_a_5_1_stream(golden, unpack_first, monkeypatch):
    import e2e_cases as E
    import test_gpu_group as TG
    A, G, O = _mods()
    if unpack_first:
        monkeypatch.setenv("IAMF_HIP_GROUP_UNPACK", "1")
    name = "l51_A_s16"
    case = E.CASES[name]
    stream, _ = E.build(name)
    want, want_rets = golden.npz("e2e")[name], list(golden.npz("e2e")[name + "_rets"])
    lib = _decoder_lib()
    _reset(A)
    A.route_family_tally("LPCM", reset=True)
    rc, outs = TG.group_decode_all(lib, case, stream, 4, 2, starve=lambda r, i: False)
    assert rc == 0, rc
    t = _packet_tallies(A)
    if unpack_first:
        assert not any(t.values()), t
    else:
        assert t[FAM] > 0 and not [f for f in t if f != FAM and t[f]], t
    for i, (pcm, rets) in enumerate(outs):
        assert rets == want_rets and np.array_equal(pcm, want), i
