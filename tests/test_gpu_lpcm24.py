"""-m gpu: the 24-bit form of the packet-fed headline kernel (render_fast_kernel<.., LP, EARLY, LPB = 3>,
iac_amd/csrc/iamf_render_lpcm24.hip) behind iamf_hip_batch_render_lpcm.

Every fused case asserts three things: table 2 of the indexed route listing (iamf_hip_route_table_tally) names the
instance, once per call; the base tally holds the flush's GENERIC row and nothing else; every stream is bit for bit the
oracle's (oracle_lib.stream_run on ints / 2^23 — the reference's LPCM decode, pcm/IAMF_pcm_decoder.c:71-76, 144-148, is
exact in f32), with PCM and n_emitted equal to a twin batch run under IAMF_HIP_LPCM_UNFUSED=1 (unpack, then the f32 kernel:
the path every such call took before).  Both prefetch variants are forced by their switches, so no case depends on where
the host cuts between them.  Shapes: 2-4 streams, chunks of 1024 samples, at most a few thousand samples per stream.

The forms that must stay on the old path assert table 2 empty and PCM equal to the twin."""
import ctypes as C

import numpy as np
import pytest

import lpcm_util as LP
import route_cases as R

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_FACADE_UNPACK", "IAMF_HIP_GROUP_UNPACK")
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
    return {"IAMF_HIP_LP_EARLY": "1"} if early else {"IAMF_HIP_LP_LATE": "1"}


def _reset(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)


def _render(mx, oc, raw, L, row, fs, calls, first=0, n_samples=0, args_hook=None, batch_hook=None, fmt=None):
    """lpcm_util.render_lpcm that also returns what every call (and the flush) said it emitted; fmt: the PCM format
    (None: s16), the streams come back as gpu_util._view gives them"""
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
    pcm = torch.zeros((S, 240 * oc * bps), dtype=torch.uint8, device="cuda")
    n = b.flush(pcm.data_ptr(), 240 * oc * bps, st)
    torch.cuda.synchronize()
    h = pcm.cpu().numpy()
    for s in range(S):
        outs[s].append(h[s, :n * oc * bps].copy())
    ns.append(n)
    b.close()
    del keep
    return [G._view(np.concatenate(o), sum(ns), oc, fmt) for o in outs], ns


def _fill_gaps(raw, L, fs, bps, m):
    """every byte of the rows that belongs to no run: 0x7F / 0x80 alternating (a load that strays reads a large sample)"""
    used = np.zeros(raw.shape[-1], dtype=bool)
    for c in range(m):
        used[L.src_offset[c]:L.src_offset[c] + fs * bps] = True
    fill = np.where(np.arange(raw.shape[-1]) % 2 == 0, 0x7F, 0x80).astype(np.uint8)
    return np.where(used[None, None, :], raw, fill[None, None, :])


def _planar(ints, perm, bps=3):
    S, F, m, fs = ints.shape
    x = (ints[:, :, perm, :].astype(np.float64) / float(1 << (8 * bps - 1))).astype(np.float32)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)


def check_fused(mx, omx, oc, ints, fs, calls, early, head=16, pad=0, perm=None, first=0, n_samples=0, fill=False, what="", bd=16,
                check=None):
    """bd: the PCM format as tests/test_gpu_programmes.py names it (16 / 24 / 32, -32 = f32); check: the streams held against
    the oracle and the twin (None: all); early None: no switch, the variant the host's rule picks (the early one)"""
    import test_gpu_programmes as TP
    A, G, O = _mods()
    fmt = {16: A.FMT_S16, 24: A.FMT_S24, 32: A.FMT_S32, -32: A.FMT_F32}[bd]
    S, F, m, _ = ints.shape
    perm = list(range(m)) if perm is None else perm
    raw, L, row = LP.rows(ints, 3, True, [1] * m, perm, head=head, pad=pad, frame_size=fs)
    if fill:
        raw = _fill_gaps(raw, L, fs, 3, m)
    with R.environment({} if early is None else _variant(early)):
        _reset(A)
        got, ns = _render(mx, oc, raw, L, row, fs, calls, first, n_samples, fmt=fmt)
        t2, base, ext = A.route_table_tally(2, reset=True), A.route_tally(), A.route_tally_ext()
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        twin, ns_twin = _render(mx, oc, raw, L, row, fs, calls, first, n_samples, fmt=fmt)
        t2_twin, base_twin = A.route_table_tally(2, reset=True), A.route_tally()
    early = 1 if early is None else early
    assert t2 == {("LPCM24", early, m, oc, 0): len(calls)}, (what, t2)
    assert base == {R.gen(m): 1} and ext == {}, (what, base, ext)
    assert t2_twin == {} and base_twin == {("FAST", 0, m, oc, 0): len(calls), R.gen(m): 1}, (what, t2_twin, base_twin)
    assert ns == ns_twin, (what, ns, ns_twin)
    x = _planar(ints, perm)
    if n_samples:
        x, ofs = np.ascontiguousarray(x[:, :, first:first + n_samples]), n_samples
    else:
        ofs = fs
    for s in (range(S) if check is None else check):
        want = TP.oracle_stream(O, omx, oc, x[s], ofs, bd)
        assert TP.mismatch(got[s], want) is None, (what, "stream %d against the oracle" % s, TP.mismatch(got[s], want))
        assert TP.mismatch(got[s], twin[s]) is None, (what, "stream %d against the unfused twin" % s, TP.mismatch(got[s], twin[s]))


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("oc", [1, 2])
@pytest.mark.parametrize("m", R.LPCM_M)
def test_every_instance(m, oc, early):
    mx, omx = R.matrices(m, oc)
    ints = LP.ints(np.random.default_rng(2400 + 10 * m + oc), 3, 3, m, 1024, 3)
    perm = list(np.random.default_rng(m).permutation(m))
    check_fused(mx, omx, oc, ints, 1024, [2, 1], early, perm=perm)


@pytest.mark.parametrize("early", [1, 0])
def test_chunks_straddle_frames_and_the_last_chunk_is_short(early):
    # 640-sample frames, calls of 1920 and 1280 samples: chunks of 1024 + 896 and 1024 + 256, a lane's frame by division
    mx, omx = R.matrices(16, 2)
    ints = LP.ints(np.random.default_rng(2464), 3, 5, 16, 640, 3)
    check_fused(mx, omx, 2, ints, 640, [3, 2], early)


@pytest.mark.parametrize("early", [1, 0])
def test_a_trimmed_frame(early):
    mx, omx = R.matrices(9, 2)
    ints = LP.ints(np.random.default_rng(2465), 4, 1, 9, 1024, 3)
    check_fused(mx, omx, 2, ints, 1024, [1], early, first=64, n_samples=512)


@pytest.mark.parametrize("early", [1, 0])
def test_runs_that_are_only_dword_aligned(early):
    """head 4, pad 4: run c starts at 4 + 3076 c — 4 mod 8 and 4 mod 16 among them — the bytes between the runs are 0x7F / 0x80
    and every run's first and last sample is at an extreme: a load that starts or ends one byte off shows"""
    mx, omx = R.matrices(16, 2)
    ints = LP.ints(np.random.default_rng(2466), 3, 3, 16, 1024, 3, level=0.2)
    ints[:, :, 0::2, 0], ints[:, :, 1::2, 0] = FULL - 1, -FULL
    ints[:, :, 0::2, -1], ints[:, :, 1::2, -1] = -FULL, FULL - 1
    raw, L, row = LP.rows(ints, 3, True, [1] * 16, list(range(16)), head=4, pad=4, frame_size=1024)
    offs = [L.src_offset[c] for c in range(16)]
    assert all(o % 4 == 0 for o in offs) and any(o % 8 == 4 for o in offs) and any(o % 16 == 4 for o in offs)
    check_fused(mx, omx, 2, ints, 1024, [2, 1], early, head=4, pad=4, fill=True)


@pytest.mark.parametrize("early", [1, 0])
def test_sign_and_carry_patterns_in_every_position_of_the_quad(early):
    """-2^23, 2^23 - 1, -1, 0, 1, 0x7FFF00 and 0x0000FF rotated through the four samples of a lane's 12 bytes: every value
    sits in each of a[23:0], {b[15:0], a[31:24]}, {c[7:0], b[31:16]} and c[31:8], next to every other.  A selection matrix
    at gain 1/4 keeps the limiter idle, so a wrong bit of the conversion is a wrong bit of the PCM."""
    A, G, O = _mods()
    vals = np.array([-FULL, FULL - 1, -1, 0, 1, 0x7FFF00, 0x0000FF], dtype=np.int64)
    m, oc, fs, F, S = 4, 2, 1024, 3, 3
    i = np.arange(F * fs)
    ints = np.zeros((S, F, m, fs), dtype=np.int64)
    for s in range(S):
        for c in range(m):
            # period 7 against the quad's 4: all 28 (value, position) pairs, shifted per channel and stream
            ints[s, :, c, :] = vals[(i + c + 2 * s) % 7].reshape(F, fs)
    w = np.zeros((m, oc), dtype=np.float32)
    w[0, 0] = w[1, 1] = 0.25
    w[2, 0] = w[3, 1] = 2.0 ** -24      # a second product per slot, far below the first: every bit of both counts
    mx, omx = R._custom(A, O, A.KIND_M2M, m, oc, w, oc)
    check_fused(mx, omx, oc, ints, fs, [1, 2], early, head=4, pad=4, fill=True)


@pytest.mark.parametrize("early", [1, 0])
def test_programmes(early):
    """all-zero packets; alternating +-full scale; a full-scale burst, then zeros (as test_gpu_programmes.test_lpcm_packets)"""
    import test_gpu_programmes as TP
    m, oc, fs, F = 4, 2, 1024, 4
    ints = np.zeros((3, F, m, fs), dtype=np.int64)
    ints[1] = np.where(np.arange(fs) % 2 == 0, FULL - 1, -FULL)[None, None, :]
    ints[2, 0, :, 100:340] = np.where(np.arange(240) % 2 == 0, FULL - 1, -FULL)[None, :]
    mx, omx = TP.selection(m, oc)
    check_fused(mx, omx, oc, ints, fs, [1, 2, 1], early, perm=[2, 0, 3, 1])


@pytest.mark.parametrize("m,oc,early", [(16, 2, 1), (16, 2, 0), (9, 1, 1)])
@pytest.mark.parametrize("bd", [24, 32, -32])
def test_into_s24_s32_and_f32_pcm(m, oc, early, bd):
    """the kernel's other pack stages behind the 24-bit loads: against the unfused twin and, in the formats
    tests/test_gpu_programmes.py compares, the oracle"""
    mx, omx = R.matrices(m, oc)
    ints = LP.ints(np.random.default_rng(2500 + 10 * m + oc), 3, 3, m, 1024, 3)
    perm = list(np.random.default_rng(50 + m).permutation(m))
    check_fused(mx, omx, oc, ints, 1024, [2, 1], early, perm=perm, bd=bd, what="bd %d" % bd)


def test_1025_streams():
    """more workgroups than the 16-bit form's early variant takes (tests/route_cases.py, lpcm_m1_oc2_1025_streams): the first,
    the 1024th and the 1025th stream, under the variant the host's rule picks"""
    mx, omx = R.matrices(1, 2)
    ints = LP.ints(np.random.default_rng(2520), 1025, 1, 1, 1024, 3)
    check_fused(mx, omx, 2, ints, 1024, [1], None, check=[0, 1023, 1024])


def check_off_grid(sb, first, n_samples, early):
    """A first one-frame call trimmed to [first, first + n_samples), two calls of a whole frame, the flush.  The tally follows
    fast_shape_ok (render_route.hpp): the trimmed call is no call of the vector kernels (its sample count is no multiple of
    64), a whole frame from a position of at least 240 is fused whatever its residue mod 16, one from an off-grid position
    below 240 is not.  PCM against the oracle over the kept samples and against the unfused twin.  (Shared with
    tests/test_gpu_lpcm.py for the 16-bit form.)"""
    A, G, O = _mods()
    m, oc, fs, S, F = 16, 2, 1024, 3, 3
    fam = "LPCM24" if sb == 3 else "LPCM"
    assert n_samples % 64 and first + n_samples <= fs
    mx, omx = R.matrices(m, oc)
    ints = LP.ints(np.random.default_rng(2530 + 7 * sb + n_samples), S, F, m, fs, sb)
    perm = list(np.random.default_rng(n_samples).permutation(m))
    raw, L, row = LP.rows(ints, sb, True, [1] * m, perm, head=16, pad=0, frame_size=fs)
    raw = _fill_gaps(raw, L, fs, sb, m)
    calls, trims = [1, 1, 1], {0: (first, n_samples)}

    def run(env):
        emitted = []
        with R.environment(env):
            _reset(A)
            got = LP.render_lpcm(mx, oc, raw, L, row, fs, calls, trims=trims, emitted=emitted)
            return got, emitted, A.route_tally(), A.route_tally_ext(), A.route_table_tally(2, reset=True)

    got, ns, base, ext, t2 = run(_variant(early))
    twin, ns_twin, base_twin, ext_twin, t2_twin = run({"IAMF_HIP_LPCM_UNFUSED": "1"})
    fused = [pos >= 240 or pos % 16 == 0 for pos in (n_samples, n_samples + fs)]     # where the whole-frame calls start
    general = 1 + fused.count(False) + 1                                               # the trimmed call, ..., the flush
    inst = {(fam, early, m, oc, 0): fused.count(True)}
    if sb == 3:
        assert t2 == inst and base == {R.gen(m): general}, (t2, base)
    else:
        assert t2 == {} and base == {**inst, R.gen(m): general}, (t2, base)
    assert ext == ext_twin == t2_twin == {}
    assert base_twin == {("FAST", 0, m, oc, 0): fused.count(True), R.gen(m): general}, base_twin
    assert ns == ns_twin, (ns, ns_twin)
    x = _planar(ints, perm, sb)
    kept = np.ascontiguousarray(np.concatenate([x[:, :, first:first + n_samples], x[:, :, fs:]], axis=2))
    for s in range(S):
        want = O.stream_run(omx, oc, kept[s], fs)
        g = got[s].view(np.int16).reshape(-1, oc)
        assert g.shape == want.shape and np.array_equal(g, want), "stream %d against the oracle" % s
        assert np.array_equal(got[s], twin[s]), "stream %d against the unfused twin" % s


@pytest.mark.parametrize("early", [1, 0])
@pytest.mark.parametrize("first,n_samples", [(24, 1000), (0, 237), (0, 3)])
def test_positions_off_the_16_sample_grid(first, n_samples, early):
    check_off_grid(3, first, n_samples, early)


@pytest.mark.parametrize("early", [1, 0])
def test_stream_ranges_advance_on_their_own(early):
    """iamf_hip_batch_render_lpcm_range over [0, 2) and [2, 5) of a 5-stream batch: the ranges take different frame counts
    per round and in one round only the first advances; per stream against the oracle, and the PCM rows outside a call's
    range keep their fill"""
    import torch
    A, G, O = _mods()
    m, oc, fs, S, F = 16, 2, 1024, 5, 4
    mx, omx = R.matrices(m, oc)
    ints = LP.ints(np.random.default_rng(2540), S, F, m, fs, 3)
    perm = list(np.random.default_rng(2541).permutation(m))
    raw, L, row = LP.rows(ints, 3, True, [1] * m, perm, head=16, pad=0, frame_size=fs)
    d_raw = torch.from_numpy(_fill_gaps(raw, L, fs, 3, m)).cuda()
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
        t2, base, ext = A.route_table_tally(2, reset=True), A.route_tally(), A.route_tally_ext()
    assert at == [F, F]
    assert t2 == {("LPCM24", early, m, oc, 0): 5} and base == {R.gen(m): 2} and ext == {}, (t2, base, ext)
    x = _planar(ints, perm)
    for s in range(S):
        want = O.stream_run(omx, oc, x[s], fs)
        got = np.concatenate(outs[s]).view(np.int16).reshape(-1, oc)
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d" % s


def test_fused_f32_unfused_and_16_bit_calls_follow_one_another_on_one_batch():
    """fused 24-bit call -> render_ex on f32 -> unfused 24-bit call -> fused 16-bit call -> flush: the whole equals the
    oracle's run over the concatenation (the persisted state is the same whichever kernel left it)"""
    import torch
    A, G, O = _mods()
    m, oc, fs, S = 16, 2, 1024, 3
    mx, omx = R.matrices(m, oc)
    rng = np.random.default_rng(2470)
    i24a, i24b = LP.ints(rng, S, 2, m, fs, 3), LP.ints(rng, S, 1, m, fs, 3)
    i16 = LP.ints(rng, S, 2, m, fs, 2)
    import synth
    xf = np.stack([synth.hot(2471 + s, m, 2 * fs, sigma=0.22, burst_phase=300, burst_period=900) for s in range(S)])
    perm = list(range(m))
    st = torch.cuda.current_stream().cuda_stream
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    outs = [[] for _ in range(S)]

    def take(pcm, n):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(h[s, :n * oc * 2].copy())

    def lpcm_call(ints, bps, nf):
        raw, L, row = LP.rows(ints, bps, True, [1] * m, perm, head=16, pad=0, frame_size=fs)
        d_raw = torch.from_numpy(raw).cuda()
        pcm = torch.zeros((S, nf * fs * oc * 2), dtype=torch.uint8, device="cuda")
        inp = A.LpcmInput()
        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
        a = A.RenderArgs()
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), nf * fs * oc * 2, st
        take(pcm, b.render_lpcm(inp, a))

    _reset(A)
    lpcm_call(i24a, 3, 2)
    assert A.route_table_tally(2) == {("LPCM24", 1, m, oc, 0): 1} and A.route_tally(reset=False) == {}
    d_in = torch.from_numpy(G.to_frames(xf, fs)).cuda()
    pcm = torch.zeros((S, 2 * fs * oc * 2), dtype=torch.uint8, device="cuda")
    a = A.RenderArgs()
    a.d_in, a.in_stream_stride, a.in_frame_stride = d_in.data_ptr(), 2 * m * fs, m * fs
    a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 2, pcm.data_ptr(), 2 * fs * oc * 2, st
    take(pcm, b.render_ex(a))
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        lpcm_call(i24b, 3, 1)
    lpcm_call(i16, 2, 2)
    pcm = torch.zeros((S, 240 * oc * 2), dtype=torch.uint8, device="cuda")
    take(pcm, b.flush(pcm.data_ptr(), 240 * oc * 2, st))
    b.close()
    assert A.route_table_tally(2, reset=True) == {("LPCM24", 1, m, oc, 0): 1}
    assert A.route_tally() == {("FAST", 0, m, oc, 0): 2, ("LPCM", 1, m, oc, 0): 1, R.gen(m): 1}
    x = np.concatenate([_planar(i24a, perm), xf.astype(np.float32), _planar(i24b, perm), _planar(i16, perm, 2)], axis=2)
    for s in range(S):
        got = np.concatenate(outs[s]).view(np.int16).reshape(-1, oc)
        want = O.stream_run(omx, oc, np.ascontiguousarray(x[s]), fs)
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d" % s


# ------------------------------------------------------------------------------------------
# forms that stay on the old path
# ------------------------------------------------------------------------------------------

def check_unfused(mx, oc, ints, bps, le, fs, calls, head=16, omx=None, args_hook=None, batch_hook=None, fast_variant=0, what=""):
    """table 2 stays empty, the f32 kernel runs, the PCM is the twin's (and the oracle's where one is given)"""
    A, G, O = _mods()
    S, F, m, _ = ints.shape
    raw, L, row = LP.rows(ints, bps, le, [1] * m, list(range(m)), head=head, pad=0, frame_size=fs)
    _reset(A)
    got, ns = _render(mx, oc, raw, L, row, fs, calls, args_hook=args_hook, batch_hook=batch_hook)
    t2, base = A.route_table_tally(2, reset=True), A.route_tally()
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        twin, ns_twin = _render(mx, oc, raw, L, row, fs, calls, args_hook=args_hook, batch_hook=batch_hook)
        base_twin = A.route_tally()
    assert t2 == {}, (what, t2)
    assert base == base_twin == {("FAST", fast_variant, m, oc, 0): len(calls), R.gen(m): 1}, (what, base, base_twin)
    assert ns == ns_twin
    for s in range(S):
        assert np.array_equal(got[s], twin[s]), (what, "stream %d against the twin" % s)
        if omx is not None:   # (little-endian 24 bit only: ints / 2^23)
            want = O.stream_run(omx, oc, _planar(ints, list(range(m)), bps)[s], fs)
            assert np.array_equal(got[s], want), (what, "stream %d against the oracle" % s)


def test_big_endian_24_bit_stays_unfused():
    mx, omx = R.matrices(16, 2)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2480), 3, 3, 16, 1024, 3), 3, False, 1024, [2, 1])


def test_32_bit_stays_unfused():
    mx, omx = R.matrices(16, 2)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2481), 3, 3, 16, 1024, 4), 4, True, 1024, [2, 1])


def test_runs_at_offset_2_mod_4_stay_unfused():
    mx, omx = R.matrices(16, 2)
    check_unfused(mx, 2, LP.ints(np.random.default_rng(2482), 3, 3, 16, 1024, 3), 3, True, 1024, [2, 1], head=2, omx=omx)


def test_a_weight_of_2_to_the_minus_110_stays_unfused():
    A, G, O = _mods()
    m, oc = 4, 2
    w = np.zeros((m, oc), dtype=np.float32)
    w[0, 0] = w[1, 1] = 0.9
    w[2, 0], w[3, 1] = np.float32(2.0 ** -110), 0.4
    mx, omx = R._custom(A, O, A.KIND_M2M, m, oc, w, oc)
    check_unfused(mx, oc, LP.ints(np.random.default_rng(2483), 3, 3, m, 1024, 3), 3, True, 1024, [2, 1], omx=omx)


def test_a_call_with_an_output_ramp_stays_unfused():
    import torch
    mx, omx = R.matrices(16, 2)
    S, fs = 3, 1024

    def ramp(a, nf):
        r = torch.from_numpy(np.linspace(1.0, 0.5, S * nf * fs, dtype=np.float32).reshape(S, nf * fs)).cuda()
        a.d_output_ramp, a.ramp_stream_stride = r.data_ptr(), nf * fs
        return r

    check_unfused(mx, 2, LP.ints(np.random.default_rng(2484), S, 3, 16, fs, 3), 3, True, fs, [2, 1], args_hook=ramp, fast_variant=1)


def test_a_batch_with_a_second_element_stays_unfused():
    import torch
    A, G, O = _mods()
    mx, omx = R.matrices(16, 2)
    mx2, _ = R.matrices(2, 2)
    S, fs = 3, 1024

    def second(b):
        b.set_second_element(mx2)
        return mx2

    def in2(a, nf):
        x2 = torch.from_numpy(np.random.default_rng(2490 + nf).uniform(-0.2, 0.2, (S, nf, 2, fs)).astype(np.float32)).cuda()
        a.d_in2, a.in2_stream_stride, a.in2_frame_stride = x2.data_ptr(), nf * 2 * fs, 2 * fs
        return x2

    check_unfused(mx, 2, LP.ints(np.random.default_rng(2485), S, 3, 16, fs, 3), 3, True, fs, [2, 1], args_hook=in2, batch_hook=second,
                  fast_variant=1)


def test_the_fanout_entry_keeps_24_bit_packets_on_one_unpack_and_the_f32_fanout():
    import torch
    A, G, O = _mods()
    m, fs, S, K, nf = 16, 1024, 3, 2, 2
    ocs = [2, 1]
    mxs = [R.matrices(m, oc) for oc in ocs]
    ints = LP.ints(np.random.default_rng(2486), S, nf, m, fs, 3)
    raw, L, row = LP.rows(ints, 3, True, [1] * m, list(range(m)), head=16, pad=0, frame_size=fs)
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
    assert A.route_table_tally(2, reset=True) == {} and A.route_tally_ext() == {}
    assert A.route_tally() == {("FANOUT", 0, m, 0, K): 1}
    x = _planar(ints, list(range(m)))
    for j in range(K):
        h = pcms[j].cpu().numpy()
        for s in range(S):
            got = h[s, :emitted[j] * ocs[j] * 2].view(np.int16).reshape(-1, ocs[j])
            want = O.stream_run(mxs[j][1], ocs[j], x[s], fs, flush=False)
            assert np.array_equal(got, want), (j, s)
        batches[j].close()


# ------------------------------------------------------------------------------------------
# callers of the reference API
# ------------------------------------------------------------------------------------------

def _toa24_stream(seed, frames, fs=1024):
    """one mono-coded 3rd-order element in 24-bit little-endian LPCM -> (bytes, the f32 samples the decoder reconstructs)"""
    import e2e_cases as E
    import iamf_writer as W
    import synth
    x = np.clip(synth.hot(seed, 16, frames * fs, sigma=0.2, burst_amp=0.7, burst_phase=900, burst_period=5000),
                -1, 1 - 2 ** -15).astype(np.float32)
    xq = W.quantize(x, 24)
    stream = W.sequence_header(1) + W.codec_config_lpcm(0, fs, 24, 48000, True)
    stream += W.audio_element_ambisonics_mono(1, 0, 16, list(range(16)))
    stream += W.mix_presentation(1, [dict(eid=1, pdef=E._pdef_static(100), default_q78=0)],
                                 dict(pdef=E._pdef_static(101), default_q78=0), [E._ss_layout("A")])
    for f in range(frames):
        stream += W.temporal_delimiter()
        stream += W.audio_frames([(i, W.lpcm_bytes(x[i:i + 1, f * fs:(f + 1) * fs], 24, True)) for i in range(16)])
    return stream, xq


def test_a_single_handle_on_a_24_bit_stream_runs_the_fused_kernel():
    import e2e_cases as E
    import iac_amd
    from decoder_driver import decode_stream
    A, G, O = _mods()
    stream, xq = _toa24_stream(2490, 4)
    lib = C.CDLL(iac_amd.lib_path())
    _reset(A)
    pcm, rets = decode_stream(lib, stream, E._ss_layout("A"), bit_depth=16)
    t2 = A.route_table_tally(2, reset=True)
    assert t2 and all(k[0] == "LPCM24" and k[2:] == (16, 2, 0) for k in t2) and sum(t2.values()) > 0, t2
    want = O.stream_run(O.get_h2m(3, O.SS["A"]), 2, xq, 1024)
    assert pcm.shape == want.shape and np.array_equal(pcm, want)


def test_a_group_of_four_handles_on_24_bit_streams_runs_the_fused_kernel():
    import e2e_cases as E
    import iac_amd
    import test_gpu_group as TG
    A, G, O = _mods()
    lib = C.CDLL(iac_amd.lib_path())   # the prototypes group_decode_all and open_handle rely on (test_gpu_group's fixture)
    lib.IAMF_decoder_open.restype = C.c_void_p
    lib.IAMF_decoder_close.argtypes = [C.c_void_p]
    lib.IAMF_decoder_configure.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.IAMF_decoder_output_layout_set_sound_system.argtypes = [C.c_void_p, C.c_int]
    lib.IAMF_decoder_set_normalization_loudness.argtypes = [C.c_void_p, C.c_float]
    lib.IAMF_decoder_set_bit_depth.argtypes = [C.c_void_p, C.c_uint32]
    lib.IAMF_decoder_peak_limiter_set_threshold.argtypes = [C.c_void_p, C.c_float]
    lib.IAMF_decoder_set_pts.argtypes = [C.c_void_p, C.c_int64, C.c_uint32]
    lib.IAMF_layout_sound_system_channels_count.argtypes = [C.c_int]
    lib.iamf_hip_decoder_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.iamf_hip_decoder_group_decode.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    lib.iamf_hip_decoder_group_destroy.argtypes = [C.c_void_p]
    lib.iamf_hip_decoder_group_destroy.restype = None
    built = [_toa24_stream(2491 + i, 3) for i in range(4)]
    case = dict(layout=E._ss_layout("A"), bit_depth=16)
    _reset(A)
    rc, outs = TG.group_decode_all(lib, case, [b[0] for b in built], 4, 2, starve=lambda r, i: False)
    assert rc == 0, rc
    t2 = A.route_table_tally(2, reset=True)
    assert t2 and all(k[0] == "LPCM24" and k[2:] == (16, 2, 0) for k in t2) and sum(t2.values()) > 0, t2
    for i, (pcm, rets) in enumerate(outs):
        want = O.stream_run(O.get_h2m(3, O.SS["A"]), 2, built[i][1], 1024)
        assert pcm.shape == want.shape and np.array_equal(pcm, want), i
