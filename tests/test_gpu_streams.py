"""-m gpu: every device entry point on caller-owned NON-BLOCKING streams, and from several host threads.

include/iamf_hip.h hands a `void *stream` to every entry that touches the device: "asynchronous on that stream unless
stated otherwise", the lifecycle entries "STREAM-ORDERED and never make the host wait", ordered behind the batch's own
event "whatever stream that used".  Every other GPU test runs on torch's current stream, the legacy null stream, where
everything serialises by itself and a missing dependency cannot show.  Here (tests/stream_util.py):

  a. every kernel family's case of tests/test_gpu_layouts.py (IDS) runs through its own builder, unchanged, on a side
     stream — once with a stall on the NULL stream in front of every library call (the call must neither wait for the
     null stream nor leave work on it that its own stream overtakes), once with the stall on the call's SAME stream
     (nothing the call queues elsewhere may run ahead of its stream) — plus the calls with a second launch beside the
     main one that IDS does not hold: a fixed PCM channel stride, an unfused packet call with a channel no sub-stream
     carries, the packet-fed fan-out's shared unpack pass, iamf_hip_batch_reset between two programmes, and the two
     creates behind a busy null stream, which they are asserted to wait for;
  b. three calls and the flush queued back to back, one host synchronisation at the end;
  c. the lifecycle entries on ANOTHER stream than the renders, the synchronous setters, reset and destroy while the
     render stream is stalled, the resampler's lifecycle on its stream;
  d. the table of entries: which return while a stall in front of them still runs (every one the header calls
     asynchronous must), which wait (the ones it calls synchronous must);
  e. four host threads with a stream and an object each, in this process and as the first device work of a fresh one.

Every comparison is the builders' own: bit for bit with the oracle (the HRTF cases with route_cases.py's tolerance).  The
stall is an input, not a threshold (stream_util: 10 ms each)."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lifecycle_util as LU
import route_cases as R
import stream_util as SU

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WHERE = [SU.NULL, SU.SAME]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()
    SU.calibrate()


def _stalled_calls(log, least):
    """the wrapper saw the calls: every one of them entered behind a running stall"""
    assert len(log) >= least, [r.entry for r in log]
    print("stalled %d calls; still stalled on return: %s" % (len(log), [(r.entry[9:], r.running_after) for r in log]))


# ------------------------------------------------------------------------------------------
# a. every kernel family off the null stream
# ------------------------------------------------------------------------------------------

def _layout_ids():
    import test_gpu_layouts as TL
    return TL.IDS


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("cid", _layout_ids())
def test_every_family_on_a_side_stream(cid, where, monkeypatch):
    import test_gpu_layouts as TL
    case = TL.BY_ID[cid]
    TL._clean_env(case, monkeypatch)
    with SU.side_stream(), SU.stalled(where) as log:
        case.build(case)
    _stalled_calls(log, 3)          # at least two calls and a flush (most: three calls and a flush per batch)


@pytest.mark.parametrize("where", WHERE)
def test_fixed_pcm_channel_stride_on_a_side_stream(where):
    """pcm_stride_channels = 12: the kernel packs into scratch of the batch and restride_kernel, a second launch behind
    it, re-lays that into the caller's rows.  7.1.4 -> 5.1, three streams, calls of 1, 3, 2 frames and the flush; the
    re-laid rows against the oracle's PCM: slot c of sample-frame i at element 12 i + c, slots 6 .. 11 zero."""
    import torch
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    m, oc, sc, fs, calls = 12, 6, 12, 1024, [1, 3, 2]
    mx, omx = R.matrices(m, oc)
    x = R.drive_limiter(O, omx, oc, R.hot(m, sum(calls), fs))
    xf = G.to_frames(x, fs)
    outs = [[] for _ in range(R.S)]
    with SU.side_stream(), SU.stalled(where) as log:
        st = torch.cuda.current_stream().cuda_stream
        b = A.Batch(R.S, mx, oc, frame_size=fs, projection=A.PROJ_EXACT, pcm_stride_channels=sc)
        b.set_gains(element=R.EG, output=R.OG)
        keep, f0 = None, 0
        for nf in calls + [0]:
            cap = max(nf * fs, 240) * sc * 2
            rows, d_pcm, stride = G.pcm_rows(R.S, cap, G.PAD16)
            if nf:
                pl = G.place_input(xf, G.PAD16, f0, nf, keep=keep)
                keep = pl.keep
                n = b.render(pl.d_in, pl.stream_stride, pl.frame_stride, nf, d_pcm, stride, st)
            else:
                n = b.flush(d_pcm, stride, st)
            torch.cuda.synchronize()
            h = G.rows_and_rest(rows, G.PAD16, n * sc * 2)
            for s in range(R.S):
                outs[s].append(h[s].view(np.int16).reshape(n, sc).copy())
            f0 += nf
        b.close()
    _stalled_calls(log, len(calls) + 1)
    for s in range(R.S):
        got = np.concatenate(outs[s])
        want = O.stream_run(omx, oc, x[s], fs, element_gain=R.EG[s], output_gain=R.OG[s])
        R.compare(got[:, :oc], want, 0, ("restride", s))
        assert not got[:, oc:].any(), ("slots beyond the layout's channels", s)


@pytest.mark.parametrize("where", WHERE)
def test_unfused_packets_with_an_absent_channel_on_a_side_stream(where):
    """a 5.1 element whose pairs are coupled sub-streams (never fused) and whose LFE no sub-stream carries: the first call
    allocates the batch's f32 buffer and zeroes it — the absent channel's rows are written by nothing else — in front of
    the unpack kernel and the render kernel; the second call (three frames) grows it.  A dense seeded matrix, so that the
    absent channel's row counts.  Bit for bit against the oracle fed a zero LFE."""
    import iac_amd as A
    import fanout_lpcm_util as U
    import lpcm_util as LP
    import oracle_lib as O
    m, oc, fs, calls = 6, 2, 1024, [1, 3, 2]
    ints = LP.ints(np.random.default_rng(4242), R.S, sum(calls), m, fs, 2)
    perm = [0, 1, 4, 5, 2, 3]
    raw, L, row = LP.rows(ints, 2, True, [2, 2, 1, 1], perm, head=16, pad=0, frame_size=fs)
    absent = 3
    L.src_offset[absent] = -1
    x = U.decoded(ints, perm)
    x[:, absent, :] = 0.0
    mx, omx = R.matrices(m, oc, table=False)
    with SU.side_stream(), SU.stalled(where) as log:
        got = LP.render_lpcm(mx, oc, raw, L, row, fs, calls)
    _stalled_calls(log, len(calls) + 1)
    for s in range(R.S):
        assert float(np.abs(O.render(omx, x[s], oc)).max()) > 0.95, "the programme does not drive the limiter"
        R.compare(got[s].view(np.int16).reshape(-1, oc), O.stream_run(omx, oc, x[s], fs), 0, ("absent channel", s))


@pytest.mark.parametrize("where", WHERE)
def test_fanout_lpcm_shared_unpack_pass_on_a_side_stream(where):
    """iamf_hip_batch_render_fanout_lpcm with a coupled 5.1 element into {A, MONO}: one unpack pass into the first member's
    buffer, then the f32 fan-out launch that both members share — three launches on the call's stream"""
    import fanout_lpcm_util as U
    import lpcm_util as LP
    import test_gpu_fanout_lpcm as TF
    S, fs, calls = 4, 1024, [2, 1]
    specs = [U.A_S16, U.MONO_S16_M6]
    ints = U.ints16(S, sum(calls), 6, fs)
    perm = [0, 1, 4, 5, 2, 3]
    raw, L, row = LP.rows(ints, 2, True, [2, 2, 1, 1], perm, head=8, pad=8, frame_size=fs)
    x = U.decoded(ints, perm)
    TF.assert_condition("L51", specs, x)
    mxs = [TF.mats("L51", sp["layout"])[0] for sp in specs]
    with SU.side_stream(), SU.stalled(where) as log:
        d = U.Drive(mxs, specs, raw, L, row, None, fs)
        reports = [d.fan(nf) for nf in calls]
        d.flush()
        d.close()
    assert reports == [(2, 0, 1)] * len(calls), reports
    _stalled_calls(log, len(calls) + 2)
    TF.assert_oracle(d, "L51", specs, x, fs)


@pytest.mark.parametrize("where", WHERE)
def test_reset_between_two_programmes_on_a_side_stream(where):
    """iamf_hip_batch_reset takes no stream: it uploads the fresh limiter state and zeroes the rings on the null stream,
    behind renders on a side stream and in front of the next"""
    S, W = 3, 5
    with SU.side_stream(), SU.stalled(where) as log:
        rig = LU.Rig("fast", S, W)
        p1 = [LU.hot(3100 + s, rig.m, 2, rig.fs) for s in range(S)]
        p2 = [LU.hot(3150 + s, rig.m, 3, rig.fs, cut_frames=1) for s in range(S)]
        for s in range(S):
            rig.put(s, 0, p1[s])
            rig.put(s, 2, p2[s])
        rig.render(0, 0, S, 2)
        rig.b.reset()
        rig.render(2, 0, S, 3)
        rig.flush(0, S)
        got = [rig.take(s) for s in range(S)]
        rig.close()
    _stalled_calls(log, 3)
    head = 2 * rig.fs - 240
    for s in range(S):
        LU.same(got[s][:head], rig.want(p1[s], flush=False), ("first programme", s))
        LU.same(got[s][head:], rig.want(p2[s]), ("second programme", s))


def test_batch_create_behind_a_busy_null_stream():
    """iamf_hip_batch_create uploads and zeroes its state on the null stream and is documented synchronous: called with the
    null stream busy it returns after that work (asserted), and a first render on a side stream — queued at once, nothing
    waited for in between — finds the state."""
    import torch
    import iac_amd as A
    S, W = 3, 2
    with SU.side_stream() as side:
        rig = LU.Rig("fast", S, W)              # the input, the rows and the oracle's matrix; its batch is replaced below
        p = [LU.hot(3200 + s, rig.m, W, rig.fs, cut_frames=1) for s in range(S)]
        for s in range(S):
            rig.put(s, 0, p[s])
        q = Queue(rig, 2)
        c = LU.CASES["fast"]
        mx = A.get_h2m_matrix(3, A.SS[c["out"]])
        rig.close()
        torch.cuda.synchronize()
        ev = SU.stall(torch.cuda.default_stream())
        assert not ev.query()
        rig.b = A.Batch(S, mx, rig.ch, frame_size=rig.fs, out_format=A.FMT_S16, limiter=True, loudness=True,
                        projection=A.PROJ_EXACT)
        assert ev.query(), "iamf_hip_batch_create returned with its null-stream work still queued"
        q.render(0, 0, S, W, side.cuda_stream)
        q.flush(0, S, side.cuda_stream)
        side.synchronize()
        got = q.collect()
        rig.close()
    for s in range(S):
        LU.same(_cat(got[s]), rig.want(p[s]), ("create", s))


def test_resampler_create_behind_a_busy_null_stream():
    """the same for iamf_hip_resampler_create: the first process call follows it at once on a side stream"""
    import torch
    import iac_amd as A
    import oracle_lib as O
    S, n_in = 3, 1000
    x = (np.random.default_rng(77).standard_normal((S, n_in, 2)) * 0.3).astype(np.float32)
    with SU.side_stream() as side:
        d_in = torch.from_numpy(x).cuda()
        cap = n_in * (48000 // 44100 + 1)        # iamf_hip_resampler_out_capacity's formula
        d_out = torch.zeros((S, cap, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ev = SU.stall(torch.cuda.default_stream())
        assert not ev.query()
        r = A.Resampler(S, 2, 44100, 48000)
        assert ev.query(), "iamf_hip_resampler_create returned with its null-stream work still queued"
        assert r.out_capacity(n_in) == cap
        n = r.process(d_in.data_ptr(), n_in * 2, n_in, d_out.data_ptr(), cap * 2, side.cuda_stream)
        side.synchronize()
        got = d_out.cpu().numpy()
        r.close()
    for s in range(S):
        want, _ = O.resample_run(np.ascontiguousarray(x[s].T), 44100, 48000, [n_in], flush=False)
        assert n == want.shape[1]
        assert np.array_equal(np.ascontiguousarray(got[s, :n].T).view(np.uint32), want.view(np.uint32)), ("resampler create", s)


# ------------------------------------------------------------------------------------------
# b. no host synchronisation between calls
# ------------------------------------------------------------------------------------------

class Queue:
    """a lifecycle_util.Rig whose calls are only QUEUED: every call gets PCM rows of its own, made (and zeroed) before
    anything is stalled, and nothing is read before collect()"""

    def __init__(self, rig, n_calls):
        self.rig, t = rig, rig.torch
        self.cap = max(3 * rig.fs, 240) * rig.ch * 2
        self.pcms = [t.zeros((rig.S, self.cap), dtype=t.uint8, device="cuda") for _ in range(n_calls)]
        self.calls = []           # (pcm, n, s0, cnt)

    def _pcm(self):
        return self.pcms[len(self.calls)]

    def render(self, wall, s0, cnt, nf, stream):
        rig, A = self.rig, self.rig.A
        assert nf <= 3
        pcm = self._pcm()
        a = A.RenderArgs()
        a.d_in = rig.xin.data_ptr() + 4 * wall * rig.m * rig.fs
        a.in_stream_stride, a.in_frame_stride = rig.W * rig.m * rig.fs, rig.m * rig.fs
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), self.cap, stream
        self.calls.append((pcm, rig.b.render_range(a, s0, cnt), s0, cnt))

    def flush(self, s0, cnt, stream):
        pcm = self._pcm()
        self.calls.append((pcm, self.rig.b.flush_range(pcm.data_ptr(), self.cap, stream, s0, cnt), s0, cnt))

    def collect(self):
        """after the one synchronisation: per slot the PCM of its calls, in order; rows outside a call's range untouched"""
        rig = self.rig
        out = [[] for _ in range(rig.S)]
        for pcm, n, s0, cnt in self.calls:
            h = pcm.cpu().numpy()
            for s in range(rig.S):
                if s0 <= s < s0 + cnt:
                    out[s].append(h[s][:n * rig.ch * 2].view(np.int16).reshape(n, rig.ch).copy())
                    assert not h[s][n * rig.ch * 2:].any(), "written past the emitted run"
                else:
                    assert not h[s].any(), "a stream outside the range was written"
        return out


def _cat(parts):
    return np.concatenate(parts, axis=0)


@pytest.mark.parametrize("case", list(LU.CASES))
def test_calls_queued_back_to_back(case):
    """three calls (the first the largest) and the flush behind a stall each, nothing read in between"""
    import torch
    S, W = 3, 5
    with SU.side_stream() as side:
        rig = LU.Rig(case, S, W)
        x = [LU.hot(3300 + s, rig.m, W, rig.fs) for s in range(S)]
        for s in range(S):
            rig.put(s, 0, x[s])
        q = Queue(rig, 4)
        torch.cuda.synchronize()
        with SU.stalled(SU.SAME) as log:
            q.render(0, 0, S, 3, side.cuda_stream)
            q.render(3, 0, S, 1, side.cuda_stream)
            q.render(4, 0, S, 1, side.cuda_stream)
            q.flush(0, S, side.cuda_stream)
        torch.cuda.synchronize()
        got = q.collect()
        rig.close()
    _stalled_calls(log, 4)
    for s in range(S):
        LU.same(_cat(got[s]), rig.want(x[s]), (case, s))


def test_resampler_calls_queued_back_to_back():
    import torch
    import iac_amd as A
    import oracle_lib as O
    S, ch, rates, sizes = 3, 2, (44100, 48000), [1300, 700, 333]
    x = (np.random.default_rng(3400).standard_normal((S, sum(sizes), ch)) * 0.3).astype(np.float32)
    with SU.side_stream() as side:
        r = A.Resampler(S, ch, rates[0], rates[1])
        d_in = torch.from_numpy(x).cuda()
        caps = [max(r.out_capacity(n), 1) for n in sizes] + [max(r.flush_capacity(), 1)]
        outs = [torch.zeros((S, c, ch), dtype=torch.float32, device="cuda") for c in caps]
        torch.cuda.synchronize()
        ns, pos = [], 0
        with SU.stalled(SU.SAME) as log:
            for k, n_in in enumerate(sizes):
                ns.append(r.process(d_in.data_ptr() + 4 * pos * ch, sum(sizes) * ch, n_in, outs[k].data_ptr(), caps[k] * ch,
                                    side.cuda_stream))
                pos += n_in
            ns.append(r.flush(outs[3].data_ptr(), caps[3] * ch, side.cuda_stream))
        torch.cuda.synchronize()
        got = np.concatenate([o.cpu().numpy()[:, :n] for o, n in zip(outs, ns)], axis=1)
        r.close()
    _stalled_calls(log, 4)
    for s in range(S):
        want, _ = O.resample_run(np.ascontiguousarray(x[s].T), rates[0], rates[1], sizes)
        g = np.ascontiguousarray(got[s].T)
        assert g.shape == want.shape, (s, g.shape, want.shape)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), s


# ------------------------------------------------------------------------------------------
# c. the cross-stream contract of the lifecycle entries
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(LU.CASES))
def test_lifecycle_entries_on_another_stream_than_the_renders(case):
    """Batch A (5 slots) renders two frames on S1 behind a stall.  With the host never waiting, S2 takes: a restart of slot 3
    (new gains, a new programme), new gains for slot 1 (silent so far: the oracle with the new gains holds for all of it)
    and for slot 4 (loud: its first two frames must be the old gains'), an export of slot 2 and its import into slot 0 of batch B.  S1 then
    waits for an event recorded on S2 — what the header tells callers to do — and renders on; B renders on S2.  Every slot
    must be the oracle's for its own programme: the lifecycle kernels ran behind the two frames (the batch's event), the
    later renders behind them (the caller's), and touched no slot outside their range."""
    import torch
    import iac_amd as A
    W = 5
    with SU.side_stream() as s1:
        s2 = torch.cuda.Stream()
        SU.assert_non_blocking(s2.cuda_stream)
        assert s2.cuda_stream != s1.cuda_stream
        a, b = LU.Rig(case, 5, W), LU.Rig(case, 3, W)
        fs, m = a.fs, a.m
        x = [LU.hot(3500 + s, m, W, fs) for s in range(5)]
        x[1][:, :2 * fs] = 0.0        # silent until its gains change: the oracle opened with the new gains holds for all of it
        second = LU.hot(3553, m, 3, fs, cut_frames=1)
        for s in range(5):
            a.put(s, 0, x[s][:, :(2 if s == 3 else W) * fs])
        a.put(3, 2, second)
        b.put(0, 2, x[2][:, 2 * fs:])
        nbytes = a.b.stream_state_bytes()
        blob = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
        for rig in (a, b):            # scratch that grows with the largest call (and waits for the stream when it does) has grown
            rig.render(0, 0, rig.S, 3)
            rig.b.restart_range(0, rig.S, None, s1.cuda_stream)
            rig.out = [[] for _ in range(rig.S)]
        qa, qb = Queue(a, 8), Queue(b, 2)
        torch.cuda.synchronize()

        ev = SU.stall(s1)
        assert not ev.query()
        qa.render(0, 0, 5, 2, s1.cuda_stream)
        assert not ev.query(), "the render stream's stall ended before the lifecycle calls were made"
        a.b.restart_range(3, 1, LU.gains_of(A, (3,)), s2.cuda_stream)
        a.b.set_gains_range(1, 1, LU.gains_of(A, (1,)), s2.cuda_stream)
        a.b.set_gains_range(4, 1, LU.gains_of(A, (4,)), s2.cuda_stream)
        tickets = a.b.export_range(2, 1, blob.data_ptr(), nbytes, s2.cuda_stream)
        b.b.import_range(0, 1, blob.data_ptr(), nbytes, tickets, s2.cuda_stream)
        # "never make the host wait for the device": the batch's event, which the entries wait for ON THE DEVICE, is
        # still behind the stall
        assert not ev.query(), "a lifecycle entry made the host wait for the render queued on the other stream"
        done2 = torch.cuda.Event()
        done2.record(s2)
        s1.wait_event(done2)
        for s0, cnt in ((0, 3), (3, 1), (4, 1)):
            qa.render(2, s0, cnt, 3, s1.cuda_stream)
        for s0, cnt in ((0, 3), (3, 1), (4, 1)):
            qa.flush(s0, cnt, s1.cuda_stream)
        qb.render(2, 0, 1, 3, s2.cuda_stream)
        qb.flush(0, 1, s2.cuda_stream)
        torch.cuda.synchronize()
        ga, gb = qa.collect(), qb.collect()
        assert tickets[0].cursor[0] == 2 * fs and tickets[0].cursor[1] == 0
        a.close()
        b.close()
    head = 2 * fs - (240 if a.limiter else 0)
    for s in (0, 2):
        LU.same(_cat(ga[s]), a.want(x[s]), ("ran through", s))
    LU.same(_cat(ga[1]), a.want(x[1], LU.new_gains(1)), "gains set from S2")
    # slot 4 is loud while its gains are set: a setter that overtook the two frames would show in them
    LU.same(ga[4][0], a.want(x[4][:, :2 * fs], flush=False), "the frames queued before the gains were set")
    assert not np.array_equal(_cat(ga[4]), a.want(x[4])), "the gains set from S2 never reached slot 4"
    LU.same(ga[3][0], a.want(x[3][:, :2 * fs], flush=False), "first life of the restarted slot")
    LU.same(_cat(ga[3][1:]), a.want(second, LU.new_gains(3)), "second life of the restarted slot")
    LU.same(_cat([ga[2][0][:head]] + gb[0]), a.want(x[2]), "migrated to the second batch")
    assert gb[1] == [] and gb[2] == []


def test_synchronous_setters_reset_and_destroy_while_the_render_stream_is_stalled():
    """iamf_hip_batch_set_gains, _reset and _destroy take no stream and are documented synchronous: issued while the render
    they follow has not even started, they wait for it.  PCM queued before them is the oracle's for the old gains and the
    old state, PCM queued after them for the new."""
    import torch
    S, W = 3, 5
    with SU.side_stream() as s1:
        rigs = [LU.Rig("fast", S, W) for _ in range(3)]
        fs, m = rigs[0].fs, rigs[0].m
        p1 = [LU.hot(3600 + s, m, 2, fs) for s in range(S)]
        p2 = [LU.hot(3650 + s, m, 3, fs, cut_frames=1) for s in range(S)]
        old, new = (0.9, 1.1, 0.95), (1.15, 0.85, 1.05)
        for rig in rigs:
            for s in range(S):
                rig.put(s, 0, p1[s])
                rig.put(s, 2, p2[s])
            rig.b.set_gains(element=[old[0]] * S, output=[old[1]] * S, loudness=[old[2]] * S)
        qs = [Queue(rig, 3) for rig in rigs]
        torch.cuda.synchronize()
        waited = {}

        # set_gains, then reset, behind a stalled render
        ev = SU.stall(s1)
        qs[0].render(0, 0, S, 2, s1.cuda_stream)
        assert not ev.query()
        rigs[0].b.set_gains(element=[new[0]] * S, output=[new[1]] * S, loudness=[new[2]] * S)
        waited["iamf_hip_batch_set_gains"] = ev.query()
        rigs[0].b.reset()
        qs[0].render(2, 0, S, 3, s1.cuda_stream)
        qs[0].flush(0, S, s1.cuda_stream)

        # reset alone behind a stalled render
        ev = SU.stall(s1)
        qs[1].render(0, 0, S, 2, s1.cuda_stream)
        assert not ev.query()
        rigs[1].b.reset()
        waited["iamf_hip_batch_reset"] = ev.query()
        qs[1].render(2, 0, S, 3, s1.cuda_stream)
        qs[1].flush(0, S, s1.cuda_stream)

        # destroy behind a stalled render
        ev = SU.stall(s1)
        qs[2].render(0, 0, S, 2, s1.cuda_stream)
        assert not ev.query()
        rigs[2].close()
        waited["iamf_hip_batch_destroy"] = ev.query()

        torch.cuda.synchronize()
        got = [q.collect() for q in qs]
        rigs[0].close()
        rigs[1].close()
    print("waited for the stalled render:", waited)
    assert all(waited.values()), waited
    rig = rigs[0]
    for s in range(S):
        first = rig.want(p1[s], old, flush=False)
        LU.same(got[0][s][0], first, ("before set_gains", s))
        LU.same(_cat(got[0][s][1:]), rig.want(p2[s], new), ("after set_gains and reset", s))
        LU.same(got[1][s][0], first, ("before reset", s))
        LU.same(_cat(got[1][s][1:]), rig.want(p2[s], old), ("after reset", s))
        LU.same(got[2][s][0], first, ("before destroy", s))


def test_resampler_lifecycle_on_its_stream_without_a_host_wait():
    """the resampler keeps no event: restart, export and import are ordered by the stream of the process calls alone.  Four
    stereo streams, 44.1 -> 48 kHz; after two calls stream 1 is restarted and stream 2 moves to a second resampler; every
    call behind a stall, one synchronisation at the end."""
    import torch
    import iac_amd as A
    import oracle_lib as O
    import synth
    S, ch, rates = 4, 2, (44100, 48000)
    sizes = [1024, 700, 1024, 512]
    x = [synth.uniform(3700 + s, ch, sum(sizes), amp=0.9) for s in range(S)]
    y = synth.uniform(3750, ch, sizes[2] + sizes[3], amp=0.9)      # stream 1's second programme
    offs = np.cumsum([0] + sizes)

    def rows_of(k, who):
        t = np.zeros((S, 1024, ch), dtype=np.float32)
        for s in range(S):
            src = y[:, offs[k] - offs[2]:offs[k + 1] - offs[2]] if (s == 1 and k >= 2) else x[s][:, offs[k]:offs[k + 1]]
            t[s, :sizes[k]] = src.T
        if who == "b":       # the second resampler: its slot 0 continues stream 2
            t[0] = t[2]
        return torch.from_numpy(t).cuda()

    with SU.side_stream() as side:
        st = side.cuda_stream
        ra, rb = A.Resampler(S, ch, *rates), A.Resampler(S, ch, *rates)
        ins_a = [rows_of(k, "a") for k in range(4)]
        ins_b = [rows_of(k, "b") for k in (2, 3)]
        cap, fcap = ra.out_capacity(1024), max(ra.flush_capacity(), 1)
        nbytes = ra.stream_state_bytes()
        blob = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
        calls = []                # (who, out tensor, {s0: n}, ranges)

        def process(r, who, inter, ns, ranges):
            o = torch.zeros((S, cap, ch), dtype=torch.float32, device="cuda")
            n = {}
            for s0, cnt in ranges:
                n[s0] = r.process_range(inter.data_ptr(), 1024 * ch, ns, o.data_ptr(), cap * ch, s0, cnt, st)
                assert n[s0] >= 0, (who, s0, n[s0])
            calls.append((who, o, n, ranges))

        def flush(r, who, ranges):
            o = torch.zeros((S, fcap, ch), dtype=torch.float32, device="cuda")
            n = {}
            for s0, cnt in ranges:
                n[s0] = r.flush_range(o.data_ptr(), fcap * ch, s0, cnt, st)
                assert n[s0] >= 0, (who, s0, n[s0])
            calls.append((who, o, n, ranges))

        torch.cuda.synchronize()
        with SU.stalled(SU.SAME) as log:
            process(ra, "a", ins_a[0], sizes[0], [(0, S)])
            process(ra, "a", ins_a[1], sizes[1], [(0, S)])
            ra.restart_range(1, 1, st)
            tickets = ra.export_range(2, 1, blob.data_ptr(), nbytes, st)
            rb.import_range(0, 1, blob.data_ptr(), nbytes, tickets, st)
            groups = [(1, 1), (0, 1), (2, 2)]
            process(ra, "a", ins_a[2], sizes[2], groups)
            process(ra, "a", ins_a[3], sizes[3], groups)
            flush(ra, "a", groups)
            process(rb, "b", ins_b[0], sizes[2], [(0, 1)])
            process(rb, "b", ins_b[1], sizes[3], [(0, 1)])
            flush(rb, "b", [(0, 1)])
        torch.cuda.synchronize()
        out = {"a": [[] for _ in range(S)], "b": [[] for _ in range(S)]}
        for who, o, n, ranges in calls:
            h = o.cpu().numpy()
            served = set()
            for s0, cnt in ranges:
                for s in range(s0, s0 + cnt):
                    out[who][s].append(h[s, :n[s0]].T.copy())
                    served.add(s)
            for s in range(S):
                assert s in served or not h[s].any(), "a stream outside the ranges was written"
        ra.close()
        rb.close()
    _stalled_calls(log, 14)

    def same(got, want, what):
        got = np.concatenate(got, axis=1)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what

    same(out["a"][1][:2], O.resample_run(x[1][:, :offs[2]], rates[0], rates[1], sizes[:2], flush=False)[0], "first life")
    same(out["a"][1][2:], O.resample_run(y, rates[0], rates[1], sizes[2:])[0], "second life")
    for s in (0, 2, 3):
        same(out["a"][s], O.resample_run(x[s], rates[0], rates[1], sizes)[0], ("ran through", s))
    same(out["a"][2][:2] + out["b"][0], O.resample_run(x[2], rates[0], rates[1], sizes)[0], "migrated")


# ------------------------------------------------------------------------------------------
# d. asynchrony as documented
# ------------------------------------------------------------------------------------------

def test_asynchronous_entries_return_under_a_stall_and_synchronous_ones_wait():
    """Steady state: every entry has been called once at the test's largest size and the device is idle, so no kernel is
    loaded and no scratch grows in the call that is observed.  Then a stall on the call's own stream in front of it: an
    entry the header calls asynchronous or stream-ordered has returned while the stall still runs; an entry it calls
    synchronous returns after it.  The table is printed."""
    import torch
    import fanout_lpcm_util as U
    import iac_amd as A
    import lpcm_util as LP
    L = A.lib()
    table, observed = {}, set()

    with SU.side_stream() as side:
        st = side.cuda_stream

        def observe(what, fn, warm=True):
            """fn() once unobserved (and waited for), then behind a stall; what returned first?"""
            if warm:
                fn()
                torch.cuda.synchronize()
            with SU.stalled(SU.SAME) as log:
                fn()
            torch.cuda.synchronize()
            assert log, what
            observed.update(r.entry for r in log)
            for r in log:
                assert isinstance(r.result, int) and r.result >= 0, (what, r)
                table[what if len(log) == 1 else "%s (%s)" % (what, r.entry)] = r.running_after

        S, W, fs = 3, 8, 1024
        rig = LU.Rig("fast", S, W)           # TOA -> binaural, render_fast_kernel
        m, ch = rig.m, rig.ch
        for s in range(S):
            rig.put(s, 0, LU.hot(3800 + s, m, W, fs))
        cap = 2 * fs * ch * 2
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")

        def args(nf=2):
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = rig.xin.data_ptr(), W * m * fs, m * fs
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), cap, st
            return a

        observe("iamf_hip_batch_render", lambda: rig.b.render(rig.xin.data_ptr(), W * m * fs, m * fs, 2, pcm.data_ptr(), cap, st))
        observe("iamf_hip_batch_render_ex", lambda: rig.b.render_ex(args()))
        observe("iamf_hip_batch_render_range", lambda: rig.b.render_range(args(), 0, S))
        gains = LU.gains_of(A, range(S))

        def ok(r):
            return 0 if r is None else r

        observe("iamf_hip_batch_set_gains_range", lambda: ok(rig.b.set_gains_range(0, S, gains, st)))
        nbytes = rig.b.stream_state_bytes()
        blob = torch.zeros((S, nbytes), dtype=torch.uint8, device="cuda")
        tickets = []
        observe("iamf_hip_batch_export_range", lambda: ok(tickets.append(rig.b.export_range(0, S, blob.data_ptr(), nbytes, st))))
        observe("iamf_hip_batch_import_range", lambda: ok(rig.b.import_range(0, S, blob.data_ptr(), nbytes, tickets[-1], st)))
        # a flush ends a stream: restart between the warm flush and the observed one
        rig.b.flush(pcm.data_ptr(), cap, st)
        observe("iamf_hip_batch_restart_range", lambda: ok(rig.b.restart_range(0, S, None, st)))
        rig.b.render_ex(args())
        torch.cuda.synchronize()
        observe("iamf_hip_batch_flush", lambda: rig.b.flush(pcm.data_ptr(), cap, st), warm=False)
        rig.b.restart_range(0, S, None, st)
        rig.b.render_ex(args())
        torch.cuda.synchronize()
        observe("iamf_hip_batch_flush_range", lambda: rig.b.flush_range(pcm.data_ptr(), cap, st, 0, S), warm=False)
        rig.b.restart_range(0, S, None, st)

        # the synchronous entries: behind a stalled render they wait for it
        def waits(what, fn):
            ev = SU.stall(side)
            rig.b.render_ex(args())
            assert not ev.query(), what
            fn()
            table[what + " [synchronous]"] = not ev.query()
            torch.cuda.synchronize()

        waits("iamf_hip_batch_set_gains", lambda: rig.b.set_gains(element=[1.0] * S))
        waits("iamf_hip_batch_reset", lambda: rig.b.reset())

        # the second batch of the fan-outs: the same element into mono
        mono = A.Batch(S, A.get_h2m_matrix(3, A.SS["MONO"]), 1, frame_size=fs, threshold_db=-6.0)
        pcm2 = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        both = [rig.b, mono]
        observe("iamf_hip_batch_render_fanout", lambda: sum(A.render_fanout(
            both, rig.xin.data_ptr(), W * m * fs, m * fs, 2, [pcm.data_ptr(), pcm2.data_ptr()], [cap, cap], st)[0]))
        observe("iamf_hip_batch_render_fanout_range", lambda: sum(A.render_fanout_range(
            both, rig.xin.data_ptr(), W * m * fs, m * fs, 2, [pcm.data_ptr(), pcm2.data_ptr()], [cap, cap], 0, S, st)[0]))

        # packets: 16-bit mono sub-streams (the fused kernel), 32-bit (unpacked first)
        for bps, what in ((2, "fused"), (4, "unfused")):
            ints = LP.ints(np.random.default_rng(3900 + bps), S, 2, m, fs, bps)
            raw, lay, row = LP.rows(ints, bps, True, [1] * m, list(range(m)), head=16, pad=0, frame_size=fs)
            d_raw = torch.from_numpy(raw).cuda()
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), 2 * row, row, lay

            def pargs():
                a = args()
                a.d_in = None
                return a

            A.route_reset()
            observe("iamf_hip_batch_render_lpcm, " + what, lambda: rig.b.render_lpcm(inp, pargs()))
            assert any(k[0] == "LPCM" for k in A.route_tally()) == (what == "fused")
            observe("iamf_hip_batch_render_lpcm_range, " + what, lambda: rig.b.render_lpcm_range(inp, pargs(), 0, S))
            rig.b.restart_range(0, S, None, st)      # the members of a fan-out stand at one position
            mono.restart_range(0, S, None, st)
            observe("iamf_hip_batch_render_fanout_lpcm, " + what, lambda: sum(A.render_fanout_lpcm(
                both, inp, 2, [pcm.data_ptr(), pcm2.data_ptr()], [cap, cap], st)[0]))
            d_f32 = torch.zeros((S, m * fs), dtype=torch.float32, device="cuda")
            fc = torch.tensor([0, fs], dtype=torch.int32, device="cuda")
            observe("iamf_hip_lpcm_unpack, %d bit" % (8 * bps), lambda: A.lpcm_unpack(
                lay, d_raw.data_ptr(), 2 * row, fc.data_ptr(), d_f32.data_ptr(), m * fs, S, st, first_count_stride=0))
        waits("iamf_hip_batch_destroy", lambda: rig.close())
        mono.close()

        # the HOA LFE generator's filter over a frame that is trimmed away
        lfe = LU.Rig("lfe", S, W)
        for s in range(S):
            lfe.put(s, 0, LU.hot(3950 + s, lfe.m, W, fs))
        observe("iamf_hip_batch_lfe_advance", lambda: L.iamf_hip_batch_lfe_advance(
            lfe.b.h, lfe.xin.data_ptr(), W * lfe.m * fs, fs, st, 0, S))
        lfe.close()

        # the resampler
        r, r2 = A.Resampler(S, 2, 44100, 48000), A.Resampler(S, 2, 44100, 48000)
        n_in = 1024
        rin = torch.zeros((S, n_in, 2), dtype=torch.float32, device="cuda")
        rcap = max(r.out_capacity(n_in), r.flush_capacity(), 1)
        rout = torch.zeros((S, rcap, 2), dtype=torch.float32, device="cuda")
        observe("iamf_hip_resampler_process", lambda: r.process(rin.data_ptr(), n_in * 2, n_in, rout.data_ptr(), rcap * 2, st))
        observe("iamf_hip_resampler_process_range", lambda: r.process_range(rin.data_ptr(), n_in * 2, n_in, rout.data_ptr(), rcap * 2, 0, S, st))
        rbytes = r.stream_state_bytes()
        rblob = torch.zeros((S, rbytes), dtype=torch.uint8, device="cuda")
        rt = []
        observe("iamf_hip_resampler_export_range", lambda: ok(rt.append(r.export_range(0, S, rblob.data_ptr(), rbytes, st))))
        observe("iamf_hip_resampler_import_range", lambda: ok(r2.import_range(0, S, rblob.data_ptr(), rbytes, rt[-1], st)))
        r2.flush(rout.data_ptr(), rcap * 2, st)
        torch.cuda.synchronize()
        observe("iamf_hip_resampler_flush", lambda: r.flush(rout.data_ptr(), rcap * 2, st), warm=False)
        observe("iamf_hip_resampler_restart_range", lambda: ok(r.restart_range(0, S, st)))
        r.process(rin.data_ptr(), n_in * 2, n_in, rout.data_ptr(), rcap * 2, st)
        torch.cuda.synchronize()
        observe("iamf_hip_resampler_flush_range", lambda: r.flush_range(rout.data_ptr(), rcap * 2, 0, S, st), warm=False)
        r.close()
        r2.close()

        # the helpers
        src = torch.zeros((S, 512, 6), dtype=torch.float32, device="cuda")
        dst = torch.zeros((S, 6, 512), dtype=torch.float32, device="cuda")
        observe("iamf_hip_deinterleave_f32", lambda: L.iamf_hip_deinterleave_f32(
            src.data_ptr(), 512 * 6, 6, S, 512, dst.data_ptr(), 6 * 512, 512, st))
        flag = torch.zeros(16, dtype=torch.int32).pin_memory()
        observe("iamf_hip_stream_signal", lambda: L.iamf_hip_stream_signal(st, flag.data_ptr(), 7))
        assert int(flag[0]) == 7
        hsrc = torch.arange(4096, dtype=torch.int32).pin_memory()
        ddst = torch.zeros(4096, dtype=torch.int32, device="cuda")
        observe("iamf_hip_upload_by_kernel", lambda: L.iamf_hip_upload_by_kernel(
            C.c_void_p(hsrc.data_ptr()), C.c_void_p(ddst.data_ptr()), C.c_size_t(4096 * 4), C.c_void_p(st)))
        assert torch.equal(ddst.cpu(), hsrc)
        pin = torch.zeros(S * 2 * 4 * 4096, dtype=torch.uint8, device="cuda")
        pout = torch.zeros(S * 2 * 1 * 4096, dtype=torch.uint8, device="cuda")
        observe("iamf_hip_probe_traffic", lambda: L.iamf_hip_probe_traffic(
            S, 2, 4, 1, pin.data_ptr(), 2 * 4 * 4096, pout.data_ptr(), 2 * 4096, st))
        with SU.stalled(SU.SAME) as log:
            A.hipabi.pick_buffer_pair(S, 2, 4, 1, [pin.data_ptr()], 2 * 4 * 4096, [pout.data_ptr()], 2 * 4096, st)
        table["iamf_hip_pick_buffer_pair [synchronous]"] = log[0].running_after
        observed.update(r.entry for r in log)
        torch.cuda.synchronize()

    print("entry: returned while the stall in front of it was still running")
    for k in sorted(table):
        print("  %-60s %s" % (k, table[k]))
    sync = {k for k in table if k.endswith("[synchronous]")}
    assert len(sync) == 4 and len(table) - len(sync) >= 30, sorted(table)
    # every stream-taking entry of the header (tests/test_streams_cpu.py holds ENTRIES against it) is in the table
    assert observed == set(SU.ENTRIES), (sorted(set(SU.ENTRIES) - observed), sorted(observed - set(SU.ENTRIES)))
    assert not [k for k in sync if table[k]], "documented synchronous, returned under the stall"
    assert not [k for k in table if k not in sync and not table[k]], "documented asynchronous, waited for the stall"


def test_a_call_that_grows_the_batch_scratch_waits_and_an_equal_one_does_not():
    """the header's one exception to "asynchronous on that stream": the call in which scratch of the batch grows (here the
    output of the HOA LFE generator's pre-pass) waits for its stream before it re-allocates; a call no larger than an
    earlier one does not.  Calls of 1, 1 and 3 frames and the flush behind a stall each; the PCM is the oracle's all the same."""
    import torch
    S, W = 3, 5
    with SU.side_stream() as side:
        rig = LU.Rig("lfe", S, W)
        x = [LU.hot(4000 + s, rig.m, W, rig.fs) for s in range(S)]
        for s in range(S):
            rig.put(s, 0, x[s])
        q = Queue(rig, 4)
        torch.cuda.synchronize()
        with SU.stalled(SU.SAME) as log:
            q.render(0, 0, S, 1, side.cuda_stream)
            q.render(1, 0, S, 1, side.cuda_stream)
            q.render(2, 0, S, 3, side.cuda_stream)
            q.flush(0, S, side.cuda_stream)
        torch.cuda.synchronize()
        got = q.collect()
        rig.close()
    _stalled_calls(log, 4)
    assert [r.running_after for r in log[:3]] == [False, True, False], log      # (the flush reads no input: no pre-pass)
    for s in range(S):
        LU.same(_cat(got[s]), rig.want(x[s]), ("lfe", s))


# ------------------------------------------------------------------------------------------
# e. host threads
# ------------------------------------------------------------------------------------------

THREAD_CALLS = [1, 3, 2]
THREAD_JOBS = {"fast": (16, 2, 1024), "wide4": (12, 12, 1024), "general": (2, 2, 1000)}
RS = dict(rates=(44100, 48000), ch=2, streams=3, sizes=[700, 1300, 333])


def test_four_threads_each_with_a_stream_and_an_object():
    """fast, wide4, the general kernel and a resampler, each driven by a thread of its own on a side stream of its own
    (torch's current stream is per thread), three calls and the flush, all four at once from a barrier"""
    import torch
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    progs = {}
    for job, (m, oc, fs) in THREAD_JOBS.items():
        mx, omx = R.matrices(m, oc)
        progs[job] = (mx, omx, R.drive_limiter(O, omx, oc, R.hot(m, sum(THREAD_CALLS), fs)))
    xr = (np.random.default_rng(4100).standard_normal((RS["streams"], sum(RS["sizes"]), RS["ch"])) * 0.3).astype(np.float32)
    torch.zeros(1, device="cuda")
    SU.calibrate()
    barrier = threading.Barrier(4)
    out, errors = {}, []

    def matrix_job(job):
        m, oc, fs = THREAD_JOBS[job]
        mx, _, x = progs[job]
        with SU.side_stream():
            barrier.wait(timeout=60)
            out[job] = G.hip_render(mx, oc, x, frame_size=fs, frames_per_call=THREAD_CALLS,
                                    gains=dict(element=R.EG, output=R.OG), projection=A.PROJ_EXACT)

    def resampler_job(job):
        ns, ch = RS["streams"], RS["ch"]
        with SU.side_stream() as side:
            r = A.Resampler(ns, ch, *RS["rates"])
            barrier.wait(timeout=60)
            outs, pos = [], 0
            for n_in in RS["sizes"] + [0]:
                cap = max(r.out_capacity(n_in) if n_in else r.flush_capacity(), 1)
                rows, d_out, stride = G.pcm_rows(ns, cap * ch * 4, G.PAD16, bps=4)
                if n_in:
                    inter = G.place_input(xr[:, pos:pos + n_in].reshape(ns, 1, 1, n_in * ch), G.PAD16)
                    n = r.process(inter.d_in, inter.stream_stride, n_in, d_out, stride // 4, side.cuda_stream)
                else:
                    n = r.flush(d_out, stride // 4, side.cuda_stream)
                pos += n_in
                side.synchronize()
                outs.append(np.stack(G.rows_and_rest(rows, G.PAD16, n * ch * 4)).view(np.float32).reshape(ns, n, ch))
            r.close()
            out[job] = np.concatenate(outs, axis=1)

    def guarded(fn, job):
        try:
            fn(job)
        except BaseException as e:
            barrier.abort()
            errors.append((job, repr(e)))

    A.route_reset()
    threads = [threading.Thread(target=guarded, args=(matrix_job, job)) for job in THREAD_JOBS]
    threads.append(threading.Thread(target=guarded, args=(resampler_job, "resampler")))
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    tally = A.route_tally()
    assert not errors, errors
    for job, (m, oc, fs) in THREAD_JOBS.items():
        _, omx, x = progs[job]
        for s in range(R.S):
            R.compare(out[job][s], O.stream_run(omx, oc, x[s], fs, element_gain=R.EG[s], output_gain=R.OG[s]), 0, (job, s))
    for s in range(RS["streams"]):
        want, _ = O.resample_run(np.ascontiguousarray(xr[s].T), RS["rates"][0], RS["rates"][1], RS["sizes"])
        g = np.ascontiguousarray(out["resampler"][s].T)
        assert g.shape == want.shape and np.array_equal(g.view(np.uint32), want.view(np.uint32)), ("resampler", s)
    n = len(THREAD_CALLS)
    R.check_tally(tally, [(("FAST", 0, 16, 2, 0), n), (R.gen(16), 1), (("WIDE4", 0, 12, 12, 0), n), (R.gen(12), 1),
                          (R.gen(2), n + 1), (R.resampler_instance(44100, 48000, 2, 3), n + 1)])


def test_four_threads_as_the_first_device_work_of_a_process():
    """tests/threads_first_use.py in a fresh process: the four threads' first launches are of kernels that opt in to
    more than 64 KiB of LDS (launch_big_lds), two threads on the same instance"""
    import oracle_lib as O
    import threads_first_use as T
    r = subprocess.run([sys.executable, os.path.join(HERE, "threads_first_use.py")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for job, (m, oc, fs, _) in T.JOBS.items():
        _, omx, x = T.programme(job)
        for s in range(R.S):
            want = O.stream_run(omx, oc, x[s], fs, element_gain=R.EG[s], output_gain=R.OG[s])
            assert res["hashes"][job][s] == T.digest(want), (job, s)
    got = {tuple(k): v for k, v in res["tally"]}
    R.check_tally(got, T.expected_tally())
