"""-m gpu: iamf_hip_batch_render_packets_ragged — one element as LPCM packets of any call length in the four-samples-per-lane
kernel (render_fast_kernel<.., LP, true, LPB, LPC, 0, IL = false, RAG = true>, iac_amd/csrc/iamf_render_packets_ragged*.hip).

Every fused case asserts three ways (packets_ragged_util.check): (a) the oracle, bit for bit, on the packets' integer grid
(ints / 2^15 or / 2^23 is exact in f32); (b) a twin batch through iamf_hip_batch_render_packets, compared after EVERY call — the
PCM bytes (every byte outside the emitted runs still 0xA5), the value returned and the state iamf_hip_batch_export_range hands
out; (c) the tallies: the family's row exactly once per fused call, no other packet-fed family and no table with a packet row,
the twin with its GENERIC rows (the unpacker has none).  Tolerance 0 everywhere.  3 or 4 streams (12 for the boundary
programmes), at most a few thousand samples per stream.  tests/test_packets_ragged_cpu.py proves, from the oracle's limiter trace,
that the programme of every case drives the limiter across every call boundary.

Without the feature every test fails at the missing symbol.

(The file's name sorts it behind the other GPU test files: the tests that were there run first, in the order and under the
numbers they had in a run's report.)"""
import functools

import numpy as np
import pytest

import packets_ragged_util as PU
import route_cases as R

pytestmark = pytest.mark.gpu

SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION", "IAMF_HIP_NO_WIDE4",
            "IAMF_HIP_RAGGED_UNFUSED", "IAMF_HIP_INTERLEAVED_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED")
P, W, G_ = PU.PRAG, PU.WHOLE_ROW, "GENERIC"


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
    form, m, oc, fs, calls = PU.CASES[name]
    return PU.check(form, m, oc, fs, PU.programme(name), calls, what=name, **kw)


# ---- every instance ----

EVERY_INSTANCE = list(PU.INSTANCES)       # (tests/test_packets_ragged_cpu.py: exactly the family's listing)


def _walk(forms):
    """every (form, m, oc) of EVERY_INSTANCE among `forms`: a dense matrix whose weights all differ (left and right of a pair are
    told apart); one frame of 1000 followed by one of 1000 (positions 0 and 1000) -> the family's rows launched"""
    launched = []

    def one(case):
        form, m, oc = case
        got, _ = PU.check(form, m, oc, 1000, PU.hot_ints(form, m, 2000), [(1, 0), (1, 0)], routes=[P, P], what="dense %s %d -> %d" % case)
        launched.extend(row for r in got for row in r["fam"])
    each_case([(c,) for c in EVERY_INSTANCE if c[0] in forms], one)
    return launched


@pytest.mark.parametrize("forms", [("s16", "s16c"), ("s24", "s24c")], ids=["16_bit", "24_bit"])
def test_every_instance(forms):
    import iac_amd as A
    launched = _walk(forms)
    # what the walk launched, read from the library's tally, is the library's own listing: a walk cut short fails here
    want = [r for r in A.route_family_instances(PU.FAM) if r[4] == PU.FORMS[forms[0]][0]]
    assert len(want) == 18 and sorted(set(launched)) == sorted(want) and len(launched) == 2 * len(want), launched


def test_the_dense_matrix_tells_left_from_right():
    for _, m, oc in EVERY_INSTANCE:
        if m == 1:      # (one channel: nothing to swap)
            continue
        mx, _ = PU.IU.dense_matrices(m, oc)
        w = np.ctypeslib.as_array(mx.mat, shape=(m * oc,))
        assert len(set(np.abs(w).tolist())) == m * oc, (m, oc)


# ---- lengths and frames ----

def test_call_lengths_and_frames():
    """lengths: 1000, 1, 3, 63, 65, 1023, 1025 (one whole chunk plus one sample) and 480 samples of a frame of 2048, 24-bit
    mono-coded and 16-bit coupled: shorter than a quad, than a block, either side of a block and of a chunk; every call behind
    the first starts off the 16-grid.  frames_100: three frames of 100 per call, a chunk spans frames and every lane divides.
    frames_1000: five frames of 1000 per call; 5000 samples = 4 chunks and 904 samples.  mod4: total & 3 of 1, 2 and 3 in
    all four forms."""
    names = ["lengths", "lengths_coupled", "frames_100", "frames_100_mono", "frames_1000", "frames_1000_s24", "mod4_s16", "mod4_s16c", "mod4_s24",
             "mod4_s24c"]
    each_case([(n,) for n in names], lambda name: run_case(name, routes=[P] * len(PU.CASES[name][4])))


# ---- what lies behind n_samples and between the runs ----

def _gap(name):
    """head and pad of the rows: the form's own grid (8 bytes with 16-bit samples, 4 with 24-bit ones), off the 16-byte one"""
    return 8 if PU.FORMS[PU.CASES[name][0]][0] == 2 else 4


@functools.lru_cache(maxsize=None)
def _zero_filled(name):
    got, _ = run_case(name, routes=[P] * 3, fill=0, head=_gap(name), pad=_gap(name))
    return got


@pytest.mark.parametrize("name", ["mod4_s16", "mod4_s16c", "mod4_s24", "mod4_s24c"])
def test_what_lies_behind_n_samples_and_between_the_runs_changes_nothing(name):
    """calls with total & 3 of 1, 2 and 3; every byte that is no sample of the call — the rest of every run behind n_samples,
    the heads, the gaps (head and pad of 8 or 4 bytes: runs on the form's grid only) and the rows' padding — is 0x7F, 0x80 or 0xA5: full-scale samples in both widths.  The
    last quad of every run reads 3, 2 and 1 samples of it.  The results equal the zero-filled run's and the oracle's."""
    ref = _zero_filled(name)

    def one(fill):
        got, _ = run_case(name, routes=[P] * 3, fill=fill, head=_gap(name), pad=_gap(name))
        PU.assert_same(got, ref, "fill 0x%02X against the zero-filled run" % fill)
    each_case([(f,) for f in (0x7F, 0x80, 0xA5)], one)


# ---- trimmed starts ----

def test_trimmed_starts():
    """first_sample of 4, 100 and 240 in all four forms: the rest of a frame of 1000 from there, then a whole frame; what lies
    in front of first_sample is 0x80 bytes"""
    cases = [(form, m, first) for form, m in (("s16", 4), ("s16c", 6), ("s24", 4), ("s24c", 6)) for first in (4, 100, 240)]

    def one(form, m, first):
        calls = [(1, 1000 - first, first), (1, 0)]
        PU.check(form, m, 2, 1000, PU.hot_ints(form, m, 2000 - first), calls, routes=[P, P], fill=0x80, what="%s first %d" % (form, first))
    each_case(cases, one)


@pytest.mark.parametrize("form", ["s16c", "s24c"])
def test_a_coupled_pair_from_an_even_first_sample_on_both_sides_of_the_bound(form):
    """stereo (no mono run: a pair's run is on its grid from every even sample), first_sample 2 of a frame of 1000: 996 samples
    — 2 + 996 <= 1000 — are fused; 997 — the last quad would end 2 samples behind the run — are unpacked by the library; the same
    bytes either way (the twin's and the oracle's)"""
    def one(n, route):
        PU.check(form, 2, 2, 1000, PU.hot_ints(form, 2, n + 1000), [(1, n, 2), (1, 0)], routes=[route, P], fill=0x7F, what="%d samples" % n)
    each_case([(996, P), (997, G_), (998, G_), (993, P)], one)


# ---- cuts at the extremes ----

@pytest.mark.parametrize("form", sorted(PU.FORMS))
def test_the_extremes_in_the_last_partial_quad(form):
    """the last three samples of every call (total & 3 of 1, 2, 3: the partial quad holds 1, 2, 3 of them) and the first one are
    2^(b-1) - 1, -2^(b-1) and -(2^(b-1) - 1), one per stream, alternating by channel; behind them 0x80 bytes"""
    name = "mod4_" + form
    _, m, oc, fs, calls = PU.CASES[name]
    bps = PU.FORMS[form][0]
    full = 1 << (8 * bps - 1)
    ints = PU.programme(name).copy()
    pos = 0
    for _, n in calls:
        for s, v in enumerate((full - 1, -full, -(full - 1))):
            for k in (pos, pos + n - 3, pos + n - 2, pos + n - 1):
                ints[s, 0::2, k] = v
                ints[s, 1::2, k] = -v - 1 if v != -full else full - 1
        pos += n
    PU.check(form, m, oc, fs, ints, calls, routes=[P] * 3, fill=0x80, head=_gap(name), pad=_gap(name), what="extremes")


# ---- PCM formats ----

def test_pcm_formats_mono_and_stereo():
    """s24, s32 and f32 PCM (s16: every other test), a coupled 5.1 into stereo and a 24-bit first-order element into mono, calls with
    total & 3 of 1, 2, 3: the last quad is stored piece by piece"""
    mod4 = [(1, 1001), (1, 1002), (1, 1003)]

    def one(form, m, oc, bd):
        PU.check(form, m, oc, 2048, PU.hot_ints(form, m, 3006), mod4, bd=bd, routes=[P] * 3, what="%s %d -> %d, bd %d" % (form, m, oc, bd))
    each_case([(form, m, oc, bd) for form, m, oc in PU.PCM_SHAPES for bd in (16, 24, 32, -32)], one)


# ---- placement ----

def test_the_packet_layouts_the_forms_take_and_one_they_refuse():
    """PK_DENSE, PK_PAD16 and PK_GRID (strides on the form's grid only) are fused; PK_OFF_BASE (d_raw 8 bytes off the 16-byte
    rule) is unpacked by the library: the same bytes, the general kernel's row"""
    import gpu_util as G

    def one(form, m, pk, route):
        PU.check(form, m, 2, 1000, PU.hot_ints(form, m, 2000, streams=4), [(1, 0), (1, 0)], routes=[route, route], packets=pk,
                 what="%s %s" % (form, pk.name))
    each_case([(form, m, pk, G_ if pk is G.PK_OFF_BASE else P) for form, m in PU.PLACED for pk in (G.PK_DENSE, G.PK_PAD16, G.PK_GRID, G.PK_OFF_BASE)],
              one)


def test_a_range_of_streams_leaves_its_neighbours_alone():
    form, m = PU.PLACED[1]
    got, ref = PU.check(form, m, 2, 1000, PU.hot_ints(form, m, 2000, streams=4), [(1, 0), (1, 0)], rng=(1, 2), what="range")
    for r in got:
        for s in (0, 3):
            assert r["pcm"][s].size == 0
        # the neighbours' exported state: unchanged from call to call, and not what a rendered stream holds
        assert np.array_equal(r["state"][0][[0, 3]], got[0]["state"][0][[0, 3]])
        assert not np.array_equal(r["state"][0][1], r["state"][0][0])


# ---- sequences on one batch ----

def test_sequences_with_gains_export_import_flush_and_reset():
    """on one batch: ragged through the new entry; new gains for stream 0; whole blocks through the new entry (8 frames of 1000
    at position 1000, off the 16-grid: the form's whole-block family); stream 0 exported and imported into slot 2, which is fed
    stream 0's programme from there on; ragged again; planar f32 through iamf_hip_batch_render_ragged; the flush; reset; a
    ragged call of a fresh stream; restart of every slot and one more"""
    import torch
    import iac_amd as A
    import test_gpu_programmes as TP
    form, m, oc, fs = "s16", 4, 2, 1000
    amx, omx = PU.IU.dense_matrices(m, oc)
    ints = PU.hot_ints(form, m, 11000)
    ints[2, :, 9000:] = ints[0, :, 9000:]
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

    steps = [("prag", 1, 0), ("do", "gains", new_gains), ("prag", 8, 0), ("do", "move", move), ("prag", 1, 0), ("rag", 1, 0), ("flush",),
             ("reset",), ("prag", 1, 480), ("do", "restart", restart), ("prag", 1, 0)]
    routes = [P, None, W, None, P, "RAG", G_, None, P, None, P]
    got = PU.drive(amx, form, oc, fs, ints, steps, eg=eg, og=og)
    ref = PU.drive(amx, form, oc, fs, ints, PU.twin(steps), eg=eg, og=og)
    PU.assert_tallies(got, form, m, oc, routes, "sequence")
    PU.assert_tallies(ref, form, m, oc, routes, "sequence (twin)", is_twin=True)
    PU.assert_same(got, ref, "sequence")
    sz = [1000, 8000, 1000, 1000]
    w, _ = PU.want(omx, oc, ints[0], 2, sz, 16, [0.8, 1.1, 1.1, 1.1], [1.0, 0.7, 0.7, 0.7])
    assert TP.mismatch(PU.stream_pcm(got[:7], 0, oc, 16), w) is None
    w, _ = PU.want(omx, oc, ints[1], 2, sz, 16, eg[1], og[1])
    assert TP.mismatch(PU.stream_pcm(got[:7], 1, oc, 16), w) is None
    assert got[4]["pcm"][0].any() and np.array_equal(got[4]["pcm"][2], got[4]["pcm"][0])       # the imported stream continues as its source
    # behind the reset the driver's position restarts: the programme's first 480 again
    w, _ = PU.want(omx, oc, ints[1], 2, [480], 16, eg[1], og[1], flush=False)      # (stream 1 holds the gains it was created with)
    assert TP.mismatch(PU.stream_pcm(got[8:9], 1, oc, 16), w) is None, "stream 1 behind the reset"
    for s in range(3):
        w, _ = PU.want(omx, oc, ints[s][:, 480:], 2, [1000], 16, 0.9, 1.0, flush=False)
        assert TP.mismatch(PU.stream_pcm(got[10:], s, oc, 16), w) is None, ("stream %d behind the restart" % s)


# ---- hand-over ----

@pytest.mark.parametrize("fs", sorted(PU.HANDOVER_CALLS))
@pytest.mark.parametrize("form,m", PU.HANDOVER)
def test_state_hand_over_to_and_from_the_other_families(form, m, fs):
    """new family -> X -> new family at boundaries of 1000 and of 100 samples, X = the whole-block packet family of the same
    form (through the new entry), FAST (iamf_hip_batch_render_range over whole blocks), FAST_RAGGED
    (iamf_hip_batch_render_ragged) and GENERIC (iamf_hip_batch_render_range over a ragged length): both directions each"""
    whole, ragged = PU.HANDOVER_CALLS[fs]["whole"], PU.HANDOVER_CALLS[fs]["ragged"]

    def one(what, calls, entry, route):
        ints = PU.hot_ints(form, m, sum(PU.sizes(fs, calls)))
        PU.check(form, m, 2, fs, ints, calls, entries=["prag", entry, "prag"], routes=[P, route, P], what=what)
    each_case([("whole-block packets", whole, "prag", W), ("FAST", whole, "range", "FAST"), ("FAST_RAGGED", ragged, "rag", "RAG"),
               ("GENERIC", ragged, "range", G_)], one)


# ---- boundary programmes ----

@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("form,m", [("s16", 4), ("s24c", 6)])
def test_the_boundary_programmes_on_the_packet_grid(form, m, rate):
    """the programmes of tests/programmes.py (the eight re-trigger sweeps, release_to_idle, onset_after_silence,
    loud_then_silence, silence) divided by 4 on the packets' grid, through a selection matrix of weight 4, one frame of 1000
    per call"""
    import programmes as PR
    import test_gpu_programmes as TP
    bps = PU.FORMS[form][0]
    fs = 1000
    nf = (PR.frames(rate) * 1024 + fs - 1) // fs
    progs = PR.boundary_set(m, nf * fs, rate)
    ints = np.stack([PR.to_packet_grid(x, 8 * bps) for _, x in progs])
    mats = TP.selection(m, 2, weight=PR.PACKET_WEIGHT)
    PU.check(form, m, 2, fs, ints, [(1, 0)] * nf, routes=[P] * nf, mats=mats, eg=[1.0], og=[1.0], rate=rate, what="%d Hz" % rate)


# ---- fall-backs: the same bytes and state as the twin, the twin's tallies, an empty family tally ----

def test_fallbacks():
    """one case per rule that sends the call elsewhere: the new entry's batch runs what the twin runs"""
    import iac_amd as A
    two = [(1, 0), (1, 0)]

    def one(what, form, m, oc, kw):
        env = kw.pop("env", {})
        oracle = kw.pop("oracle", True)
        emits = kw.pop("emits", True)
        with R.environment(env):
            ints = PU.hot_ints(form, m, 2000)
            got, _ = PU.check(form, m, oc, 1000, ints, two, routes=kw.pop("routes", [G_, G_]), what=what, oracle=oracle, **kw)
        assert any(r["pcm"][0].any() for r in got) == emits and all(r["fam"] == {} for r in got), what

    tiny = np.random.default_rng(3354).uniform(0.1, 0.5, (4, 2)).astype(np.float32)
    tiny[2, 0] = np.float32(2.0 ** -110)
    each_case([("big-endian packets", "s24", 4, 2, dict(le=False)),
               ("a pairing no form has: 5.1 as six mono runs", "s16", 6, 2, dict(oracle=True)),
               ("limiter off", "s16c", 6, 2, dict(limiter=False, oracle=False, flush=False, routes=[("NOLIM", 0, 6, 0, 0)] * 2)),
               ("six output channels", "s24", 16, 6, dict(oracle=False)),
               ("a second element on the batch: refused as the older entry refuses it", "s16", 4, 2,
                dict(second=PU.IU.identity_matrices(2)[0], oracle=False, routes=[None, None], flush=False, emits=False)),
               ("a fixed PCM channel stride", "s16c", 6, 2, dict(batch_kw={"pcm_stride_channels": 4}, oracle=False)),
               ("a weight of 2^-110", "s16", 4, 2, dict(mats=R._custom(A, __import__("oracle_lib"), A.KIND_M2M, 4, 2, tiny, 2))),
               ("IAMF_HIP_PACKETS_RAGGED_UNFUSED=1", "s24c", 6, 2, dict(env={"IAMF_HIP_PACKETS_RAGGED_UNFUSED": "1"})),
               ("IAMF_HIP_LPCM_UNFUSED=1", "s16", 4, 2, dict(env={"IAMF_HIP_LPCM_UNFUSED": "1"})),
               ("IAMF_HIP_FORCE_GENERIC=1", "s24", 4, 2, dict(env={"IAMF_HIP_FORCE_GENERIC": "1"}))], one)


def test_32_bit_packets_are_unpacked():
    import iac_amd as A
    import lpcm_util as LP
    import torch
    m, oc, fs, S = 4, 2, 1000, 3
    amx, omx = PU.IU.dense_matrices(m, oc)
    ints = PU.hot_ints("s16", m, fs).astype(np.int64) << 16
    raw, L, row = LP.rows(np.ascontiguousarray(ints.reshape(S, m, 1, fs).transpose(0, 2, 1, 3)), 4, True, [1] * m, list(range(m)), head=16, pad=0,
                          frame_size=fs)
    outs = []
    for entry in ("render_packets_ragged", "render_packets"):
        PU._reset(A)
        b = A.Batch(S, amx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
        try:
            d_raw = torch.from_numpy(raw).cuda()
            pcm = torch.full((S, fs * oc * 2), 0xA5, dtype=torch.uint8, device="cuda")
            inp, a = A.LpcmInput(), A.RenderArgs()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), row, row, L
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 1, pcm.data_ptr(), fs * oc * 2, torch.cuda.current_stream().cuda_stream
            n = getattr(b, entry)(inp, a)
            torch.cuda.synchronize()
            outs.append((n, pcm.cpu().numpy(), PU._tallies(A)))
        finally:
            b.close()
    assert outs[0][0] == outs[1][0] == fs - 240 and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2] == ({}, {PU.gen(m): 1}, {})
    import oracle_lib as O
    want = O.stream_run(omx, oc, PU.as_f32(ints[0] >> 16, 2), fs)
    assert np.array_equal(outs[0][1][0, :(fs - 240) * oc * 2].view(np.int16).reshape(-1, oc), want[:fs - 240])


# ---- refusals ----

def test_refusals_leave_the_batch_and_the_pcm_untouched_and_answer_as_the_older_entry():
    import ctypes as C
    import torch
    import iac_amd as A
    form, m, oc, fs, S = "s16c", 6, 2, 1000, 3
    amx, _ = PU.IU.dense_matrices(m, oc)
    raw, L, row = PU.packets_of(form, PU.hot_ints(form, m, fs), 1, fs)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    pcm = torch.full((S, fs * oc * 2), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lib = A.lib()

    def call(**kw):
        c = A.PacketCall()
        c.in_.d_raw, c.in_.raw_stream_stride, c.in_.raw_frame_stride, c.in_.layout = d_raw.data_ptr(), row, row, L
        c.args.n_frames, c.args.d_pcm, c.args.pcm_stream_stride_bytes, c.args.stream = 1, pcm.data_ptr(), pcm.shape[1], st
        for k, v in kw.items():
            obj, name = (c.in_, k[3:]) if k.startswith("in_") else ((c.in_.layout, k[4:]) if k.startswith("lay_") else (c.args, k))
            setattr(obj, name, v)
        return c

    def state(b):
        sb = b.stream_state_bytes()
        d = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
        b.export_range(0, S, d.data_ptr(), sb, st)
        torch.cuda.synchronize()
        return d.cpu().numpy()

    b = A.Batch(S, amx, oc, frame_size=fs)
    try:
        before = state(b)
        PU._reset(A)

        def refused(c, s0=0, cnt=S, reserved=None):
            if reserved is not None:
                c.reserved[reserved] = 1
            r = lib.iamf_hip_batch_render_packets_ragged(b.h, C.byref(c), s0, cnt)
            old = lib.iamf_hip_batch_render_packets(b.h, C.byref(c), s0, cnt)
            assert r == old and r < 0, (r, old)
            torch.cuda.synchronize()
            assert bool((pcm == 0xA5).all()) and np.array_equal(state(b), before)

        for i in range(4):
            refused(call(), reserved=i)
        refused(call(d_in=d_raw.data_ptr()))
        refused(call(d_in2=d_raw.data_ptr()))
        refused(call(in_d_raw=None))
        refused(call(d_pcm=None))
        refused(call(n_frames=-1))
        refused(call(n_frames=2, n_samples=100))
        refused(call(n_samples=fs + 1))
        refused(call(in_first_sample=8))                    # a first sample needs n_samples
        refused(call(in_first_sample=8, n_samples=fs - 4))  # and must leave room for them
        refused(call(in_first_sample=-4, n_samples=100))
        refused(call(lay_channels=5))
        refused(call(lay_frame_size=fs + 4))
        refused(call(in_raw_frame_stride=row - 16))         # a run would leave its row
        refused(call(), 0, S + 1)
        refused(call(), -1, 2)
        refused(call(), 2, 0)
        refused(call(pcm_stream_stride_bytes=64))           # IAMF_HIP_ERR_BUFFER_TOO_SMALL, as the older entry says
        assert lib.iamf_hip_batch_render_packets_ragged(b.h, None, 0, S) == -1
        assert PU._tallies(A) == ({}, {}, {})
        assert b.render_packets_ragged(call().in_, call(n_frames=0).args) == 0
        assert b.render_packets_ragged(call().in_, call().args) == fs - 240     # the batch stands where it stood: a first call
        assert PU._tallies(A) == ({PU.inst(form, m, oc): 1}, {}, {})
        # streams at different positions: a call over all of them is refused as the older entry refuses it
        assert b.render_packets_ragged(call().in_, call().args, 0, 1) == fs
        torch.cuda.synchronize()
        pcm.fill_(0xA5)
        before = state(b)
        refused(call())
    finally:
        b.close()


# ---- a caller-owned stream ----

def test_on_a_stalled_non_blocking_stream():
    """the entry on a stream proven hipStreamNonBlocking, with stream_util's stall in front of every call: on the legacy null
    stream (the call must neither wait for it nor leave work there that its own stream needs) and on the call's own stream (the
    call must return while the stall still runs).  Three calls of one frame of 1000"""
    import stream_util as SU
    import test_gpu_programmes as TP
    form, m, oc, fs = "s16c", 6, 2, 1000
    amx, omx = PU.IU.dense_matrices(m, oc)
    ints = PU.hot_ints(form, m, 3000)
    steps = [("prag", 1, 0)] * 3

    def one(where):
        with SU.side_stream() as side:
            h = side.cuda_stream

            def before_call(k, st):
                assert st == h
                SU.assert_non_blocking(st)
                ev = SU.stall(SU.torch_stream(0 if where == "NULL" else st))
                assert not ev.query(), "the stall in front of call %d had finished before the call was made" % k
                return lambda: not ev.query()

            PU.drive(amx, form, oc, fs, ints, steps, out_stream=h, export=False)      # (the kernels are loaded: the steady state is observed)
            got = PU.drive(amx, form, oc, fs, ints, steps, out_stream=h, before_call=before_call, export=False)
            ref = PU.drive(amx, form, oc, fs, ints, PU.twin(steps), out_stream=h, export=False)
        running_after = [r["note"] for r in got]
        print("still stalled on return (%s): %s" % (where, running_after))
        if where == "SAME":
            assert running_after == [True, True, True], running_after
        PU.assert_tallies(got, form, m, oc, [P] * 3, "stalled " + where)
        PU.assert_tallies(ref, form, m, oc, [P] * 3, "stalled " + where + " (twin)", is_twin=True)
        PU.assert_same(got, ref, "stalled " + where)
        for s in range(PU.S):
            w, _ = PU.want(omx, oc, ints[s], 2, [1000] * 3, 16, PU.EG[s], PU.OG[s], flush=False)
            assert TP.mismatch(PU.stream_pcm(got, s, oc, 16), w) is None, (where, "stream %d against the oracle" % s)
    each_case([("NULL",), ("SAME",)], one)
