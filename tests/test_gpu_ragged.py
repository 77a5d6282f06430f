"""-m gpu: planar f32 of any call length through iamf_hip_batch_render_ragged (render_fast_kernel<.., IL = false, RAG = true>,
iac_amd/csrc/iamf_render_ragged.hip).

Every case is checked three ways (ragged_util.check): (a) against the oracle, bit for bit; (b) against a twin batch driven
through iamf_hip_batch_render_range, after every call — PCM bytes, the value returned and the state
iamf_hip_batch_export_range hands out; (c) by the tallies — exactly one launch of the family's row per fused call and nothing
in the base tally, the twin's base row and an empty family tally where the route falls back — with every byte outside the
emitted runs still 0xA5.  Tolerance 0 everywhere.  3 streams unless a test says otherwise, a few thousand samples each.

Every float of the input that is no sample of the call — the rest of a trimmed frame's rows behind n_samples, the gaps
between frames — is a quiet NaN (ragged_util.place) unless a test names another fill, so every case also shows that nothing
loaded for an absent sample reaches the output.  The programmes burst every 700 samples: the limiter triggers in the first
call and attenuates across every ragged end into the next call (proven from the oracle's trace in
tests/test_ragged_cpu.py for every programme, matrix and call list rendered here: ragged_util.proofs).

The cases of one kind share a test function and run one after the other (each_case): every case runs whatever the ones
before it did, and the test fails with the list of the cases that failed."""
import numpy as np
import pytest

import ragged_util as RU

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_RAGGED_UNFUSED", "IAMF_HIP_INTERLEAVED_UNFUSED", "IAMF_HIP_PROJECTION", "IAMF_HIP_DENSE",
            "IAMF_HIP_NO_WIDE4")
BAD_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


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


def run_case(name, **kw):
    m, oc, fs, calls = RU.CASES[name]
    return RU.check(m, oc, fs, RU.programme(name), calls, what=name, **kw)


# ---- every instance ----

EVERY_INSTANCE = list(RU.INSTANCES)       # (tests/test_ragged_cpu.py: exactly the family's listing)


def test_every_instance():
    """every (m, oc) of EVERY_INSTANCE: a dense matrix whose weights all differ; one frame of 1000 followed by one of 1000
    (positions 0 and 1000)"""
    import iac_amd as A
    launched = []

    def one(case):
        m, oc = case
        _, _, fs, calls = RU.CASES["frame_1000"]
        x = RU.hot(m, sum(RU.sizes(fs, calls)))
        got, _ = RU.check(m, oc, fs, x, calls, routes=[RU.RAG, RU.RAG], what="dense %d -> %d" % (m, oc))
        launched.extend(row for r in got for row in r["fam"])
    each_case([(c,) for c in EVERY_INSTANCE], one)
    # what the walk launched, read from the library's tally, is the library's own listing: a walk cut short fails here
    assert sorted(set(launched)) == sorted(A.route_family_instances(RU.FAM)) and len(launched) == 2 * len(EVERY_INSTANCE), launched


# ---- lengths and frames ----

def test_call_lengths_and_frames():
    """lengths: 1000, 1, 3, 63, 65, 1023, 1025 (one whole chunk plus one sample) and 480 samples of a frame of 2048: shorter
    than a quad, than a block, either side of a block and of a chunk; every call behind the first starts off the 16-grid.
    frames_100: three frames of 100 per call, a chunk spans frames and every lane divides.  frames_1000: five frames of 1000
    per call, several chunks hold a frame boundary inside; 5000 samples = 4 chunks and 904 samples"""
    each_case([("lengths", 8), ("frames_100", 4), ("frames_1000", 2)], lambda name, n: run_case(name, routes=[RU.RAG] * n))


# ---- sequences ----

def test_sequences_of_ragged_and_aligned_calls():
    """mixed: ragged (new entry); 8 frames = 125 blocks through the OLD entry: the fast kernel at position 1000, off the 16-grid;
    ragged behind it; the same aligned call through the NEW entry: the fast kernel again (the rule leaves whole blocks
    alone); ragged behind that.  first_100: a first call of 100 samples; position 100 is below 240 and no multiple of 16, so
    the second call falls back, and the third (position 1100) is fused"""
    each_case([("mixed", dict(entries=["rag", "range", "rag", "rag", "rag"], routes=[RU.RAG, "FAST", RU.RAG, "FAST", RU.RAG])),
               ("first_100", dict(routes=[RU.RAG, "GENERIC", RU.RAG]))], lambda name, kw: run_case(name, **kw))


def test_flush_reset_and_both_entries():
    import test_gpu_programmes as TP
    m, oc, fs = 16, 2, 1000
    amx, omx = RU.IU.dense_matrices(m, oc)
    steps = [("rag", 1, 0), ("range", 1, 0), ("rag", 1, 0), ("flush",), ("reset",), ("rag", 1, 480)]
    x = RU.hot(m, 3000)
    # (the driver's position restarts with the reset: the last call renders the programme's first 480 again)
    got = RU.drive(amx, m, oc, fs, x, steps)
    ref = RU.drive(amx, m, oc, fs, x, RU.twin(steps))
    RU.assert_tallies(got, m, oc, [RU.RAG, "GENERIC", RU.RAG, "GENERIC", None, RU.RAG], "both entries")
    RU.assert_tallies(ref, m, oc, ["GENERIC"] * 4 + [None, "GENERIC"], "both entries (twin)")
    RU.assert_same(got, ref, "both entries")
    for s in range(RU.S):
        w, _ = RU.want(omx, oc, x[s], [1000] * 3, 16, RU.EG[s], RU.OG[s])
        assert TP.mismatch(RU.stream_pcm(got[:4], s, oc, 16), w) is None, ("stream %d" % s)
        w, _ = RU.want(omx, oc, x[s][:, :480], [480], 16, RU.EG[s], RU.OG[s], flush=False)
        assert TP.mismatch(RU.stream_pcm(got[5:], s, oc, 16), w) is None, ("stream %d behind the reset" % s)


def test_set_gains_export_import_and_restart_between_ragged_calls():
    """four ragged calls of one frame of 1000.  Behind the first: new gains for stream 0.  Behind the second: stream 0 is
    exported and imported into slot 2, which from then on is fed stream 0's programme and must emit what slot 0 emits.
    Behind the third: every slot is restarted (with gains) and renders its fourth frame as a fresh stream."""
    import torch
    import iac_amd as A
    import test_gpu_programmes as TP
    m, oc, fs = 9, 2, 1000
    amx, omx = RU.IU.dense_matrices(m, oc)
    x = RU.hot(m, 4000)
    x[2, :, 2000:3000] = x[0, :, 2000:3000]
    eg, og = [0.8, 1.0, 1.2], [1.0, 0.9, 1.0]

    def new_gains(b, st):
        b.set_gains_range(0, 1, A.stream_gains(element=[1.1], output=[0.7]), st)

    def move(b, st):
        sb = b.stream_state_bytes()
        blob = torch.zeros((1, sb), dtype=torch.uint8, device="cuda")
        tickets = b.export_range(0, 1, blob.data_ptr(), sb, st)
        b.import_range(2, 1, blob.data_ptr(), sb, tickets, st)
        torch.cuda.synchronize()

    def restart(b, st):
        b.restart_range(0, 3, A.stream_gains(element=[0.9] * 3, output=[1.0] * 3), st)

    steps = [("rag", 1, 0), ("do", "gains", new_gains), ("rag", 1, 0), ("do", "move", move), ("rag", 1, 0), ("do", "restart", restart),
             ("rag", 1, 0)]
    got = RU.drive(amx, m, oc, fs, x, steps, eg=eg, og=og)
    ref = RU.drive(amx, m, oc, fs, x, RU.twin(steps), eg=eg, og=og)
    RU.assert_tallies(got, m, oc, [RU.RAG, None, RU.RAG, None, RU.RAG, None, RU.RAG], "lifecycle")
    RU.assert_tallies(ref, m, oc, ["GENERIC", None, "GENERIC", None, "GENERIC", None, "GENERIC"], "lifecycle (twin)")
    RU.assert_same(got, ref, "lifecycle")
    w, _ = RU.want(omx, oc, x[0][:, :3000], [1000] * 3, 16, [0.8, 1.1, 1.1], [1.0, 0.7, 0.7], flush=False)
    assert TP.mismatch(RU.stream_pcm(got[:6], 0, oc, 16), w) is None
    assert got[4]["pcm"][0].any() and np.array_equal(got[4]["pcm"][2], got[4]["pcm"][0])       # the imported stream continues as its source
    w, _ = RU.want(omx, oc, x[1][:, :3000], [1000] * 3, 16, eg[1], og[1], flush=False)
    assert TP.mismatch(RU.stream_pcm(got[:6], 1, oc, 16), w) is None
    for s in range(3):       # fresh streams behind the restart
        w, _ = RU.want(omx, oc, x[s][:, 3000:], [1000], 16, 0.9, 1.0, flush=False)
        assert TP.mismatch(RU.stream_pcm(got[6:], s, oc, 16), w) is None, s


# ---- what lies behind n_samples and between the rows ----

def test_a_partial_last_quad_fills_and_pcm_formats():
    """calls with total & 3 of 1, 2 and 3.  The rest of the trimmed frame and the gaps hold NaN, +Inf or 3e38: the last quad
    of every channel's row reads 3, 2 and 1 floats of the fill, and the lanes behind it whole quads of it.  Then every PCM
    format, mono and stereo: the last quad is stored piece by piece"""
    m, _, fs, calls = RU.CASES["mod4"]

    def one(what, kw):
        oc = kw.pop("oc", 2)
        RU.check(m, oc, fs, RU.programme("mod4"), calls, routes=[RU.RAG] * 3, what=what, **kw)
    each_case([("fill %s" % f, dict(fill=f)) for f in (np.nan, np.inf, 3e38)] +
              [("bd %d oc %d" % (bd, oc), dict(bd=bd, oc=oc)) for oc in (1, 2) for bd in (16, 24, 32, -32)], one)


# ---- layouts, ranges ----

def test_layouts_the_kernel_takes_and_a_range_of_streams():
    import gpu_util as G
    each_case([(name,) for name in ("DENSE", "PAD16", "FRAME_MAJOR")],
              lambda name: run_case("frames_100", routes=[RU.RAG] * 4, layout=getattr(G, name)))
    # a range of streams leaves the others untouched
    m, oc, fs, calls = RU.CASES["frame_1000"]
    x = RU.hot(m, 2000, streams=4)
    got, ref = RU.check(m, oc, fs, x, calls, rng=(1, 2), what="range")
    for r in got:
        for s in (0, 3):
            assert r["pcm"][s].size == 0
        # the neighbours' exported state: unchanged from call to call, and not what a rendered stream holds
        assert np.array_equal(r["state"][0][[0, 3]], got[0]["state"][0][[0, 3]])
        assert not np.array_equal(r["state"][0][1], r["state"][0][0])


# ---- fall-backs: the same bytes and state as the twin, the twin's base tally, an empty family tally ----

def fallback(m, oc, fs, calls, routes, what, **kw):
    x = RU.hot(m, sum(RU.sizes(fs, calls)))
    got, _ = RU.check(m, oc, fs, x, calls, routes=routes, what=what, oracle=False, **kw)
    assert any(r["pcm"][0].any() for r in got), what
    return got


def test_fallbacks():
    """one case per rule that sends the call elsewhere; limiter off: 1001 samples of a frame of 1004 — no whole quads, so
    not the kernel without limiter either"""
    import gpu_util as G
    import route_cases as R
    two = [(1, 0), (1, 0)]
    second = (RU.IU.identity_matrices(2)[0], RU.hot(2, 2000, seed=77))

    def one(what, m, oc, fs, calls, kw):
        env = kw.pop("env", {})
        with R.environment(env):
            fallback(m, oc, fs, calls, ["GENERIC"] * 2, what, **kw)
    each_case([("a second element", 16, 2, 1000, two, dict(second=second)),
               ("a ramp", 16, 2, 1000, two, dict(out_ramp=True)),
               ("limiter off", 16, 2, 1004, [(1, 1001), (1, 1001)], dict(limiter=False, flush=False)),
               ("6 output channels", 16, 6, 1000, two, {}),
               ("M = 14", 14, 2, 1000, two, {}),
               ("an input 4 bytes off", 16, 2, 1000, two, dict(layout=G.OFF_IN)),
               ("a PCM stride off 16", 16, 2, 1000, two, dict(layout=G.OFF_PCM)),
               ("IAMF_HIP_RAGGED_UNFUSED=1", 16, 2, 1000, two, dict(env={"IAMF_HIP_RAGGED_UNFUSED": "1"}))], one)


# ---- refusals ----

def test_refusals_leave_the_batch_and_the_pcm_untouched():
    import torch
    import iac_amd as A
    amx, _ = RU.IU.dense_matrices(2, 2)
    fs = 1000
    d_x = torch.zeros((3, 2 * fs), dtype=torch.float32, device="cuda")
    pcm = torch.full((3, 4096), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def args(**kw):
        a = A.RenderArgs()
        a.d_in, a.in_stream_stride, a.in_frame_stride = d_x.data_ptr(), 2 * fs, 2 * fs
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 1, pcm.data_ptr(), pcm.shape[1], st
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(b, a, s0=0, cnt=3, reserved=None):
        call = A.RaggedCall()
        call.args = a
        if reserved is not None:
            call.reserved[reserved] = 1
        r = A.lib().iamf_hip_batch_render_ragged(b.h, call, s0, cnt)
        old = BAD_ARG if reserved is not None else A.lib().iamf_hip_batch_render_range(b.h, a, s0, cnt)
        assert r == old and r < 0, (r, old)
        torch.cuda.synchronize()
        assert bool((pcm == 0xA5).all())

    b = A.Batch(3, amx, 2, frame_size=fs)
    try:
        A.route_reset()
        A.route_family_tally(RU.FAM, reset=True)
        for i in range(4):
            refused(b, args(), reserved=i)
        refused(b, args(d_in=None))
        refused(b, args(d_pcm=None))
        refused(b, args(n_frames=-1))
        refused(b, args(n_frames=2, n_samples=100))
        refused(b, args(n_samples=fs + 1))
        refused(b, args(), 0, 4)
        refused(b, args(), -1, 2)
        refused(b, args(), 2, 0)
        refused(b, args(pcm_stream_stride_bytes=64))       # IAMF_HIP_ERR_BUFFER_TOO_SMALL, as the old entry says
        assert A.lib().iamf_hip_batch_render_ragged(b.h, None, 0, 3) == BAD_ARG
        assert A.route_family_tally(RU.FAM, reset=True) == {} and A.route_tally() == {}
        assert b.render_ragged(args(n_frames=0)) == 0
        assert b.render_ragged(args()) == fs - 240     # the batch stands where it stood: a first call
        assert A.route_family_tally(RU.FAM, reset=True) == {RU.inst(2, 2): 1}
        # streams at different positions: a call over all of them is refused as the old entry refuses it
        assert b.render_ragged(args(), 0, 1) == fs
        torch.cuda.synchronize()
        pcm.fill_(0xA5)
        refused(b, args())
    finally:
        b.close()


# ---- a caller-owned stream ----

def test_on_a_stalled_non_blocking_stream():
    """the entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call: on the legacy null
    stream (the call must neither wait for it nor leave work there that its own stream needs) and on the call's own stream
    (the call must return while the stall still runs).  Three ragged calls of one frame of 1000: the family's row once per
    call, PCM and state against a twin through iamf_hip_batch_render_range on the same stream, PCM against the oracle"""
    import stream_util as SU
    import test_gpu_programmes as TP
    m, oc, fs = 16, 2, 1000
    amx, omx = RU.IU.dense_matrices(m, oc)
    x = RU.hot(m, 3000)
    steps = [("rag", 1, 0)] * 3

    def one(where):
        with SU.side_stream() as side:
            h = side.cuda_stream

            def before_call(k, st):
                assert st == h
                SU.assert_non_blocking(st)
                ev = SU.stall(SU.torch_stream(0 if where == "NULL" else st))
                assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
                return lambda: not ev.query()

            RU.drive(amx, m, oc, fs, x, steps, out_stream=h, export=False)      # (the kernels are loaded: the steady state is observed)
            got = RU.drive(amx, m, oc, fs, x, steps, out_stream=h, before_call=before_call, export=False)
            ref = RU.drive(amx, m, oc, fs, x, RU.twin(steps), out_stream=h, export=False)
        running_after = [r["note"] for r in got]
        print("still stalled on return (%s): %s" % (where, running_after))
        if where == "SAME":
            assert running_after == [True, True, True], running_after
        RU.assert_tallies(got, m, oc, [RU.RAG] * 3, "stalled " + where)
        RU.assert_tallies(ref, m, oc, ["GENERIC"] * 3, "stalled " + where + " (twin)")
        RU.assert_same(got, ref, "stalled " + where)
        for s in range(RU.S):
            w, _ = RU.want(omx, oc, x[s], [1000] * 3, 16, RU.EG[s], RU.OG[s], flush=False)
            assert TP.mismatch(RU.stream_pcm(got, s, oc, 16), w) is None, (where, "stream %d against the oracle" % s)
    each_case([("NULL",), ("SAME",)], one)
