"""-m gpu: ordinary interleaved f32 of any call length through iamf_hip_batch_render_interleaved (render_fast_kernel<.., IL,
RAG>, iac_amd/csrc/iamf_render_interleaved.hip).

Every case is checked three ways (interleaved_util.check): (a) against the oracle, bit for bit; (b) against a twin batch
driven through iamf_hip_batch_render_range, after every call — PCM bytes, the value returned and the state
iamf_hip_batch_export_range hands out; (c) by the family's tally — exactly one launch of the expected row per fused call,
GENERIC where the route falls back — with every byte outside the emitted runs still 0xA5.  Tolerance 0 everywhere.
3 streams unless a test says otherwise; the programmes burst every 700 samples, so every call of the length sequences has
trigger runs and the limiter is in attack or release across every call boundary."""
import numpy as np
import pytest

import interleaved_util as IU

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_INTERLEAVED_UNFUSED", "IAMF_HIP_PROJECTION", "IAMF_HIP_DENSE")
BAD_ARG = -1
RESAMPLER = [1115, 1114, 1115]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


# ---- every instance ----

@pytest.mark.parametrize("m,oc", IU.INSTANCES)
def test_every_instance(m, oc):
    """a dense matrix whose weights all differ (a transpose that swapped left and right shows), calls as the resampler
    hands them out"""
    x = IU.hot(m, sum(RESAMPLER))
    IU.check(m, oc, x, RESAMPLER, what="dense %d -> %d" % (m, oc))


@pytest.mark.parametrize("ch", [1, 2])
def test_the_identity(ch):
    """the stage behind the resampler: the output layout's channels straight through"""
    x = IU.hot(ch, sum(RESAMPLER))
    IU.check(ch, ch, x, RESAMPLER, mats=IU.identity_matrices(ch), what="identity %d" % ch)


def test_the_dense_matrix_tells_left_from_right():
    amx, _ = IU.dense_matrices(2, 2)
    w = np.ctypeslib.as_array(amx.mat, shape=(4,))
    assert len(set(np.abs(w).tolist())) == 4


# ---- ragged ends, in every PCM format ----

RAGGED = [[1024, 1, 3, 63, 64, 65], [1023, 1025, 2049], [256, 4097]]


@pytest.mark.parametrize("bd", [16, 24, 32, -32], ids=["s16", "s24", "s32", "f32"])
@pytest.mark.parametrize("lengths", RAGGED, ids=["short", "chunk_edges", "long"])
def test_ragged_ends(lengths, bd):
    """a call shorter than a block, shorter than a quad, one sample either side of a chunk boundary; stereo and mono
    outputs take turns over the formats (the partial last quad is stored piece by piece in each)"""
    m, oc = (2, 2) if bd in (16, 32) else (2, 1)
    x = IU.hot(m, sum(lengths))
    IU.check(m, oc, x, lengths, bd=bd, what="%s bd %d" % (lengths, bd))
    if bd == 16:
        IU.check(1, 1, x[:, :1], lengths, bd=bd, what="mono %s" % (lengths,))


# ---- the limiter at the seam (the placement is proven from the oracle's trace in tests/test_interleaved_cpu.py) ----

def test_a_plateau_one_ulp_above_the_threshold_at_the_seam():
    x, lengths, _ = IU.seam_plateau()
    IU.check(2, 2, x, lengths, mats=IU.identity_matrices(2), eg=[1.0], og=[1.0], what="plateau")


def test_a_retrigger_with_the_release_across_three_calls():
    x, lengths, _ = IU.seam_retrigger()
    IU.check(2, 2, x, lengths, mats=IU.identity_matrices(2), eg=[1.0], og=[1.0], what="retrigger")


@pytest.mark.parametrize("bd", [16, -32], ids=["s16", "f32"])
def test_silence_and_off_scale_input(bd):
    import programmes as P
    n = sum(RESAMPLER)
    x = np.stack([P.silence(2, n), P.loud(2, n), P.dc_1e30(2, n)])
    IU.check(2, 2, x, RESAMPLER, bd=bd, mats=IU.identity_matrices(2), eg=[1.0], og=[1.0], what="off scale")


# ---- start-up ----

@pytest.mark.parametrize("first", [240, 256])
def test_a_first_call_that_holds_the_look_ahead(first):
    lengths = [first, 1115, 3, 1114]
    IU.check(2, 2, IU.hot(2, sum(lengths)), lengths, fused=[True] * 4, what="first %d" % first)


def test_a_first_call_of_239_sends_the_second_to_the_general_kernel():
    """position 239 is neither a multiple of 16 nor 240 on: the second call falls back, the third (position 239 + 1115) is
    fused again"""
    lengths = [239, 1115, 1114]
    IU.check(2, 2, IU.hot(2, sum(lengths)), lengths, fused=[True, False, True], what="first 239")


# ---- one batch, both entries ----

def test_both_entries_a_flush_and_a_reset_on_one_batch():
    import test_gpu_programmes as TP
    m = oc = 2
    amx, omx = IU.dense_matrices(m, oc)
    steps = [("il", 1115), ("range", 1114), ("il", 1115), ("flush",), ("reset",), ("il", 1115)]
    x = IU.hot(m, 3 * 1115 - 1)
    # (the driver's position restarts with the reset: the last call renders the programme's first 1115 again)
    got = IU.drive(amx, m, oc, x, steps)
    ref = IU.drive(amx, m, oc, x, IU.twin(steps))
    IU.assert_tallies(got, m, oc, [True, False, True, False, None, True], "both entries")
    IU.assert_same(got, ref, "both entries")
    for s in range(IU.S):
        w, _ = IU.want(omx, oc, x[s], [1115, 1114, 1115], 16, IU.EG[s], IU.OG[s])
        g = IU.stream_pcm(got[:4], s, oc, 16)
        assert TP.mismatch(g, w) is None, ("stream %d against the oracle" % s, TP.mismatch(g, w))
        w, _ = IU.want(omx, oc, x[s][:, :1115], [1115], 16, IU.EG[s], IU.OG[s], flush=False)
        g = IU.stream_pcm(got[5:], s, oc, 16)
        assert TP.mismatch(g, w) is None, ("stream %d behind the reset" % s, TP.mismatch(g, w))


# ---- ranges and lifecycle ----

def test_a_range_of_streams_leaves_the_others_untouched():
    x = IU.hot(2, sum(RESAMPLER), streams=4)
    got, ref = IU.check(2, 2, x, RESAMPLER, rng=(1, 2), what="range")
    for r in got:
        for s in (0, 3):
            assert r["pcm"][s].size == 0
        # the neighbours' exported state: what the twin's (never rendered) neighbours hold, and unchanged from call to call
        assert np.array_equal(r["state"][0][[0, 3]], got[0]["state"][0][[0, 3]])
        assert not np.array_equal(r["state"][0][1], r["state"][0][0])


def test_export_after_a_ragged_call_import_into_another_slot_and_continue():
    """stream 0 is exported behind a ragged call and imported into slot 2 of the same batch, whose own stream stands at the same
    position: slot 2 then renders stream 0's programme and must emit what stream 0 emits"""
    import torch
    import iac_amd as A
    import gpu_util as G
    m = oc = 2
    amx, omx = IU.identity_matrices(2)
    lengths = [1115, 1114]
    x = IU.hot(m, sum(lengths))
    st = torch.cuda.current_stream().cuda_stream
    b = A.Batch(3, amx, oc, frame_size=1, projection=A.PROJ_EXACT)
    try:
        def call(xi, n):
            ss = (n * m + 3) & ~3       # (the stream stride on the 16-byte grid)
            h = np.zeros((3, ss), dtype=np.float32)
            h[:, :n * m] = np.ascontiguousarray(xi.transpose(0, 2, 1)).reshape(3, n * m)
            d_x = torch.from_numpy(h).cuda()
            rows, d_pcm, stride = G.pcm_rows(3, n * oc * 2, G.PAD16, 2)
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = d_x.data_ptr(), ss, m
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n, d_pcm, stride, st
            r = b.render_interleaved(a)
            torch.cuda.synchronize()
            return G.rows_and_rest(rows, G.PAD16, r * oc * 2)
        call(x[:, :, :1115], 1115)
        sb = b.stream_state_bytes()
        blob = torch.zeros((1, sb), dtype=torch.uint8, device="cuda")
        tickets = b.export_range(0, 1, blob.data_ptr(), sb, st)
        b.import_range(2, 1, blob.data_ptr(), sb, tickets, st)
        A.route_family_tally(IU.FAM, reset=True)
        x2 = x[:, :, 1115:].copy()
        x2[2] = x2[0]
        pcm = call(x2, 1114)
        assert A.route_family_tally(IU.FAM, reset=True) == {IU.inst(m, oc): 1}
        assert np.array_equal(pcm[2], pcm[0])
        w, _ = IU.want(omx, oc, x[0], lengths, 16, flush=False)
        assert np.array_equal(pcm[0].view(np.int16).reshape(-1, oc), w[1115 - 240:])
    finally:
        b.close()


def test_1025_streams():
    """more workgroups than one wave of the launch fills; streams 0, 512 and 1024 against the oracle, all against the twin"""
    import test_gpu_programmes as TP
    m = oc = 2
    amx, omx = IU.dense_matrices(m, oc)
    base = IU.hot(m, 1115 + 63, streams=5)
    x = np.stack([base[s % 5] for s in range(1025)])
    steps = [("il", 1115), ("il", 63)]
    got = IU.drive(amx, m, oc, x, steps, export=False)
    ref = IU.drive(amx, m, oc, x, IU.twin(steps), export=False)
    IU.assert_tallies(got, m, oc, [True, True])
    IU.assert_same(got, ref, "1025 streams")
    for s in (0, 512, 1024):
        w, _ = IU.want(omx, oc, x[s], [1115, 63], 16, IU.EG[s % 3], IU.OG[s % 3], flush=False)
        g = IU.stream_pcm(got, s, oc, 16)
        assert TP.mismatch(g, w) is None, (s, TP.mismatch(g, w))


# ---- fall-backs: the same bytes, GENERIC in the tally ----

@pytest.mark.parametrize("what,kw", [("strided", dict(pad=1)), ("misaligned", dict(off_floats=1))])
def test_layouts_the_kernel_does_not_take(what, kw):
    x = IU.hot(2, sum(RESAMPLER))
    IU.check(2, 2, x, RESAMPLER, fused=[False] * 3, what=what, **kw)


def test_the_switch_sends_every_call_to_the_general_kernel(monkeypatch):
    monkeypatch.setenv("IAMF_HIP_INTERLEAVED_UNFUSED", "1")
    x = IU.hot(2, sum(RESAMPLER))
    IU.check(2, 2, x, RESAMPLER, fused=[False] * 3, what="switch")


@pytest.mark.parametrize("what", ["second_element", "output_ramp"])
def test_stages_the_kernel_does_not_take(what):
    """a batch with a second element, a call with an output ramp: against the twin and the tally (the oracle of these
    stages is tests/test_gpu_mixing.py's business)"""
    m = oc = 2
    amx, _ = IU.dense_matrices(m, oc)
    x = IU.hot(m, sum(RESAMPLER))
    kw = dict(second=(IU.identity_matrices(2)[0], IU.hot(2, sum(RESAMPLER), seed=77))) if what == "second_element" else dict(out_ramp=True)
    steps = [("il", n) for n in RESAMPLER] + [("flush",)]
    got = IU.drive(amx, m, oc, x, steps, **kw)
    ref = IU.drive(amx, m, oc, x, IU.twin(steps), **kw)
    IU.assert_tallies(got, m, oc, [False] * 4, what)
    IU.assert_same(got, ref, what)
    assert any(r["pcm"][0].any() for r in got)


# ---- refusals ----

def test_refusals_leave_the_batch_and_the_pcm_untouched():
    import torch
    import iac_amd as A
    amx, _ = IU.identity_matrices(2)
    n = 1115
    d_x = torch.zeros((3, n * 2), dtype=torch.float32, device="cuda")
    pcm = torch.full((3, 1024 * 2 * 2 * 2), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def args(**kw):
        a = A.RenderArgs()
        a.d_in, a.in_stream_stride, a.in_frame_stride = d_x.data_ptr(), n * 2, 2
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n, pcm.data_ptr(), pcm.shape[1], st
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(b, a, s0=None, cnt=None, code=BAD_ARG, reserved=None):
        call = A.InterleavedCall()
        call.args = a
        if reserved is not None:
            call.reserved[reserved] = 1
        r = A.lib().iamf_hip_batch_render_interleaved(b.h, call, 0 if s0 is None else s0, 3 if cnt is None else cnt)
        assert r == code, r
        torch.cuda.synchronize()
        assert bool((pcm == 0xA5).all())

    framed = A.Batch(3, amx, 2, frame_size=1024)
    try:
        refused(framed, args(n_frames=1, in_frame_stride=2048, in_stream_stride=2048))     # frame_size != 1
        assert A.route_family_tally(IU.FAM, reset=True) == {} and A.route_tally() == {}
    finally:
        framed.close()
    b = A.Batch(3, amx, 2, frame_size=1)
    try:
        for i in range(4):
            refused(b, args(), reserved=i)
        refused(b, args(d_in=None))
        refused(b, args(d_pcm=None))
        refused(b, args(n_frames=-1))
        refused(b, args(), 0, 4)
        refused(b, args(), -1, 2)
        refused(b, args(), 2, 0)
        refused(b, args(pcm_stream_stride_bytes=64), code=-2)      # IAMF_HIP_ERR_BUFFER_TOO_SMALL
        assert A.lib().iamf_hip_batch_render_interleaved(b.h, None, 0, 3) == BAD_ARG
        assert A.route_family_tally(IU.FAM, reset=True) == {} and A.route_tally() == {}
        assert b.render_interleaved(args()) == n - 240     # the batch stands where it stood: a first call
    finally:
        b.close()


# ---- behind the real resampler ----

def test_behind_the_resampler_44100_to_48000():
    """stereo, three calls of 1024 and the flush: iamf_hip_resampler_process runs into the new entry, a twin into
    iamf_hip_batch_render_range; both against the oracle's resampler + limiter, and against each other"""
    import torch
    import iac_amd as A
    import gpu_util as G
    import oracle_lib as O
    import test_gpu_programmes as TP
    ch, S = 2, IU.S
    amx, omx = IU.identity_matrices(ch)
    x = IU.hot(ch, 3 * 1024)
    st = torch.cuda.current_stream().cuda_stream
    outs = {}
    for entry in ("il", "range"):
        rs = A.Resampler(S, ch, 44100, 48000)
        b = A.Batch(S, amx, ch, frame_size=1, projection=A.PROJ_EXACT)
        pcm, counts, fam = [[] for _ in range(S)], [], {}
        try:
            cap = max(rs.out_capacity(1024), rs.flush_capacity())
            ss = (cap * ch + 3) & ~3
            d_y = torch.zeros((S, ss), dtype=torch.float32, device="cuda")
            A.route_family_tally(IU.FAM, reset=True)
            for k in range(4):
                if k < 3:
                    d_x = torch.from_numpy(np.ascontiguousarray(x[:, :, 1024 * k:1024 * (k + 1)].transpose(0, 2, 1))).cuda()
                    n = rs.process(d_x.data_ptr(), 1024 * ch, 1024, d_y.data_ptr(), ss, st)
                else:
                    n = rs.flush(d_y.data_ptr(), ss, st)
                counts.append(n)
                rows, d_pcm, stride = G.pcm_rows(S, max(n, 240) * ch * 2, G.PAD16, 2)
                a = A.RenderArgs()
                a.d_in, a.in_stream_stride, a.in_frame_stride = d_y.data_ptr(), ss, ch
                a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n, d_pcm, stride, st
                r = b.render_interleaved(a) if entry == "il" else b.render_range(a, 0, S)
                torch.cuda.synchronize()
                for s, h in enumerate(G.rows_and_rest(rows, G.PAD16, r * ch * 2)):
                    pcm[s].append(h)
            rows, d_pcm, stride = G.pcm_rows(S, 240 * ch * 2, G.PAD16, 2)
            r = b.flush(d_pcm, stride, st)
            torch.cuda.synchronize()
            for s, h in enumerate(G.rows_and_rest(rows, G.PAD16, r * ch * 2)):
                pcm[s].append(h)
            fam = A.route_family_tally(IU.FAM, reset=True)
        finally:
            b.close()
            rs.close()
        outs[entry] = ([np.concatenate(p) for p in pcm], counts, fam)
    # (the first call is short of the filter's latency, which the flush hands out: 1080, 1115, 1114, 35)
    assert outs["il"][1] == outs["range"][1] and 1114 in outs["il"][1] and 1115 in outs["il"][1], outs["il"][1]
    assert all(n > 0 for n in outs["il"][1])
    assert outs["il"][2] == {IU.inst(ch, ch): 4} and outs["range"][2] == {}, (outs["il"][2], outs["range"][2])
    for s in range(S):
        y, counts = O.resample_run(x[s], 44100, 48000, [1024] * 3)
        assert list(counts) == outs["il"][1], (counts, outs["il"][1])
        z, _ = O.limiter_run(np.ascontiguousarray(np.zeros_like(y) + y), list(counts))
        w = O.pack(z, 16)
        g = outs["il"][0][s].view(np.int16).reshape(-1, ch)
        assert np.array_equal(outs["il"][0][s], outs["range"][0][s]), "stream %d against the twin" % s
        assert TP.mismatch(g, w) is None, ("stream %d against the oracle" % s, TP.mismatch(g, w))


# ---- a caller-owned stream ----

@pytest.mark.parametrize("where", ["NULL", "SAME"])
def test_on_a_stalled_non_blocking_stream(where):
    """the entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call: on the legacy null
    stream (the call must neither wait for it nor leave work there that its own stream needs) and on the call's own stream"""
    import stream_util as SU
    m = oc = 2
    amx, omx = IU.dense_matrices(m, oc)
    x = IU.hot(m, sum(RESAMPLER))
    steps = [("il", n) for n in RESAMPLER]
    with SU.side_stream() as side:
        h = side.cuda_stream

        def before_call(k, st):
            assert st == h
            SU.assert_non_blocking(st)
            ev = SU.stall(SU.torch_stream(0 if where == "NULL" else st))
            assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
            return lambda: not ev.query()

        IU.drive(amx, m, oc, x, steps, out_stream=h, export=False)      # (the kernels are loaded: the steady state is observed)
        got = IU.drive(amx, m, oc, x, steps, out_stream=h, before_call=before_call, export=False)
    running_after = [r["note"] for r in got]
    print("still stalled on return (%s): %s" % (where, running_after))
    if where == "SAME":
        assert running_after == [True, True, True], running_after
    IU.assert_tallies(got, m, oc, [True] * 3, "stalled")
    import test_gpu_programmes as TP
    for s in range(IU.S):
        w, _ = IU.want(omx, oc, x[s], RESAMPLER, 16, IU.EG[s], IU.OG[s], flush=False)
        g = IU.stream_pcm(got, s, oc, 16)
        assert TP.mismatch(g, w) is None, ("stream %d against the oracle" % s, TP.mismatch(g, w))
