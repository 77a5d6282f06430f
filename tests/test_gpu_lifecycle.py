"""-m gpu: per-stream lifecycle on the batch ABI — iamf_hip_batch_restart_range, _set_gains_range, _export_range and
_import_range.

Each reference handle is opened, configured and closed on its own (IAMF_decoder.c:3809-3815): nothing couples the life of
one stream to its neighbour's.  Here the slots of ONE batch are restarted, re-gained, exported and imported while their
neighbours keep rendering, and every life of every slot must be, bit for bit, what the oracle gives for that programme
alone with those gains (oracle_lib.stream_run).  No tolerance anywhere.

Input lives in one device tensor indexed by the stream's slot and a wall-clock frame, uploaded BEFORE the calls under test,
so that nothing synchronises the host between a lifecycle call and the render behind it; the host synchronises only to
read PCM."""
import numpy as np
import pytest

from lifecycle_util import BAD_ARG, CASES, UNIMPLEMENTED, Rig, gains_of, hot, new_gains, same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(CASES))
def test_restart_next_to_running_neighbours(case):
    """streams 2..3 are abandoned un-flushed in the middle of a burst after 2 frames, stream 6 is flushed after 3; each is
    restarted with gains of its own and fed a new programme while 0, 1, 4 and 5 run through"""
    import iac_amd as A
    S, W = 7, 6
    rig = Rig(case, S, W)
    m, fs = rig.m, rig.fs
    first = [hot(1100 + s, m, W, fs) for s in range(S)]
    second = {2: hot(1202, m, 4, fs), 3: hot(1203, m, 4, fs), 6: hot(1206, m, 3, fs)}
    life1 = {2: 2, 3: 2, 6: 3}
    for s in range(S):
        rig.put(s, 0, first[s][:, :life1.get(s, W) * fs])
    rig.put(2, 2, second[2])
    rig.put(3, 2, second[3])
    rig.put(6, 3, second[6])
    rig.torch.cuda.synchronize()

    rig.render(0, 0, 7, 2)
    rig.render(2, 6, 1, 1)
    rig.flush(6, 1)
    ended = {s: rig.take(s) for s in (2, 3, 6)}
    rig.b.restart_range(2, 2, gains_of(A, (2, 3)), rig.st)
    rig.b.restart_range(6, 1, gains_of(A, (6,)), rig.st)
    rig.render(2, 2, 2, 1)       # the restarted slots first: nothing but the stream orders them behind their restart
    rig.render(2, 0, 2, 1)
    rig.render(2, 4, 2, 1)
    for wall, nf in ((3, 1), (4, 2)):
        rig.render(wall, 0, 2, nf)
        rig.render(wall, 4, 2, nf)
        rig.render(wall, 2, 2, nf)
        rig.render(wall, 6, 1, nf)
    for s0, cnt in ((0, 2), (4, 2), (2, 2), (6, 1)):
        rig.flush(s0, cnt)

    for s in (0, 1, 4, 5):
        same(rig.take(s), rig.want(first[s]), ("ran through", s))
    for s in (2, 3):
        same(ended[s], rig.want(first[s][:, :2 * fs], flush=False), ("abandoned", s))
    same(ended[6], rig.want(first[6][:, :3 * fs]), ("flushed", 6))
    for s in (2, 3, 6):
        same(rig.take(s), rig.want(second[s], new_gains(s)), ("second life", s))
    rig.close()


def test_restart_of_the_whole_batch_is_reset():
    S, W = 5, 5
    a, b = Rig("fast", S, W), Rig("fast", S, W)
    p1 = [hot(1300 + s, a.m, 2, a.fs) for s in range(S)]
    p2 = [hot(1350 + s, a.m, 3, a.fs, cut_frames=1) for s in range(S)]
    for rig in (a, b):
        for s in range(S):
            rig.put(s, 0, p1[s])
            rig.put(s, 2, p2[s])
        rig.render(0, 0, S, 2)
    a.b.reset()
    b.b.restart_range(0, S, None, b.st)
    for rig in (a, b):
        rig.render(2, 0, S, 3)
        rig.flush(0, S)
    for s in range(S):
        ga, gb = a.take(s), b.take(s)
        same(gb, ga, ("twin", s))
        same(gb[2 * a.fs - 240:], a.want(p2[s]), ("oracle", s))   # (the first life emitted 2 * fs - 240 sample-frames)
    a.close()
    b.close()


def test_fir_restart_against_a_fresh_batch():
    """the HRTF path's parity is unpinned, so batch against batch: a batch whose streams were cut off mid-burst and
    restarted (in pieces, with the history ping-pong at odd parity) renders a new programme as a fresh batch does"""
    import iac_amd as A
    S, m, taps, fs, W = 5, 4, 64, 1024, 5
    rng = np.random.default_rng(77)
    h = (rng.standard_normal((2, m, taps)) * 0.2).astype(np.float32)
    p1 = [hot(1400 + s, m, 2, fs) for s in range(S)]
    p2 = [hot(1450 + s, m, 3, fs, cut_frames=1) for s in range(S)]

    def fir_rig():
        b = A.Batch(S, A.fir_matrix(h), 2, frame_size=fs, out_format=A.FMT_S16, limiter=True, fir_taps=taps)
        return Rig(None, S, W, batch=b, m=m, fs=fs, ch=2)

    used, fresh = fir_rig(), fir_rig()
    for s in range(S):
        used.put(s, 0, p1[s])
        used.put(s, 2, p2[s])
        fresh.put(s, 2, p2[s])
    used.render(0, 0, S, 2)      # one call: the ping-pong now stands at its other buffer
    for s in range(S):
        used.take(s)
    for s0, cnt in ((1, 1), (0, 1), (2, 3)):
        used.b.restart_range(s0, cnt, None, used.st)
    for rig in (used, fresh):
        rig.render(2, 0, S, 3)
        rig.flush(0, S)
    for s in range(S):
        got = used.take(s)
        assert got.any()
        same(got, fresh.take(s), ("fir", s))
    # no export of FIR batches
    blob = used.torch.zeros(4096, dtype=used.torch.uint8, device="cuda")
    with pytest.raises(A.IamfHipError) as e:
        used.b.stream_state_bytes()
    assert e.value.code == UNIMPLEMENTED
    with pytest.raises(A.IamfHipError) as e:
        used.b.export_range(0, 1, blob.data_ptr(), 4096, used.st)
    assert e.value.code == UNIMPLEMENTED
    with pytest.raises(A.IamfHipError) as e:
        used.b.import_range(0, 1, blob.data_ptr(), 4096, [A.StreamState()], used.st)
    assert e.value.code == UNIMPLEMENTED
    used.close()
    fresh.close()


def test_range_gain_setter_against_the_whole_batch_setter():
    """gains of streams 1..2 change after two frames: the stream-ordered range setter against a twin batch driven with
    iamf_hip_batch_set_gains and whole arrays; a later whole-batch set_gains(loudness) keeps the range's other rows.
    Stream 2 is silent until the change (its limiter and rings are then a fresh stream's), so the oracle opened with the
    new gains over the whole programme confirms it as well."""
    import iac_amd as A
    S, W = 4, 5
    a, b = Rig("fast", S, W), Rig("fast", S, W)
    fs, m = a.fs, a.m
    x = [hot(1500 + s, m, W, fs) for s in range(S)]
    x[2][:, :2 * fs] = 0.0
    g = {s: new_gains(s) for s in (1, 2)}
    later = [0.8, 0.7, g[2][2], 0.9]      # the later whole-batch loudness row: stream 2 keeps its value
    for rig in (a, b):
        for s in range(S):
            rig.put(s, 0, x[s])
        rig.render(0, 0, S, 2)
    a.b.set_gains_range(1, 2, gains_of(A, (1, 2)), a.st)
    b.b.set_gains(element=[1.0, g[1][0], g[2][0], 1.0], output=[1.0, g[1][1], g[2][1], 1.0],
                  loudness=[1.0, g[1][2], g[2][2], 1.0])
    for rig in (a, b):
        rig.render(2, 0, S, 2)
        rig.b.set_gains(loudness=later)
        rig.render(4, 0, S, 1)
        rig.flush(0, S)
    got = [a.take(s) for s in range(S)]
    for s in range(S):
        same(got[s], b.take(s), ("twin", s))
    same(got[2], a.want(x[2], g[2]), "oracle, stream 2")
    # a second element's gain on a batch that has none
    with pytest.raises(A.IamfHipError) as e:
        a.b.set_gains_range(0, 1, A.stream_gains(element2=[0.5]), a.st)
    assert e.value.code == BAD_ARG
    a.close()
    b.close()


def migrate(case, trim=0):
    """batch A (5 streams) renders 2 frames, its streams 1..2 move to slots 0..1 of batch B (3 streams), which renders 3
    more and flushes; A itself goes on as well (export only reads).  Returns nothing: asserts."""
    import iac_amd as A
    W = 5
    a, b = Rig(case, 5, W), Rig(case, 3, W)
    fs, m = a.fs, a.m
    x = [hot(1600 + s + trim, m, W, fs) for s in range(5)]
    gains = [new_gains(s) for s in range(5)]
    a.b.set_gains(element=[v[0] for v in gains], output=[v[1] for v in gains], loudness=[v[2] for v in gains])
    for s in range(5):
        a.put(s, 0, x[s])
    for s in (1, 2):
        b.put(s - 1, 2, x[s][:, 2 * fs:])
    a.torch.cuda.synchronize()
    if trim:   # a first frame trimmed at its start: the streams stand off the 16-sample grid for the rest of their lives
        a.render(0, 0, 5, 1, n_samples=fs - trim, skip=trim)
        a.render(1, 0, 5, 1)
    else:
        a.render(0, 0, 5, 2)
    nbytes = a.b.stream_state_bytes()
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes == b.b.stream_state_bytes()
    stride = nbytes + 32
    blob = a.torch.zeros((2, stride), dtype=a.torch.uint8, device="cuda")
    tickets = a.b.export_range(1, 2, blob.data_ptr(), stride, a.st)
    assert [t.kind for t in tickets] == [1, 1] and all(t.bytes == nbytes for t in tickets)
    assert all(t.cursor[0] == 2 * fs - trim and t.cursor[1] == 0 for t in tickets)
    b.b.import_range(0, 2, blob.data_ptr(), stride, tickets, b.st)
    b.render(2, 0, 2, 3)
    b.flush(0, 2)
    a.render(2, 0, 5, 3)
    a.flush(0, 5)
    for s in range(5):
        want = a.want(x[s][:, trim:], gains[s])
        got = a.take(s)
        same(got, want, ("source went on", s))
        if s in (1, 2):
            head = 2 * fs - trim - (240 if a.limiter else 0)     # what A had emitted when the stream left
            same(np.concatenate([got[:head], b.take(s - 1)], axis=0), want, ("migrated", s))
    a.close()
    b.close()


@pytest.mark.parametrize("case,trim", [("fast", 0), ("wide4", 0), ("lfe", 0), ("general", 0), ("fast", 237)])
def test_migrate_a_live_stream_between_batches(case, trim):
    migrate(case, trim)


def test_compaction_lets_the_survivors_share_a_launch():
    """in one batch of 7, streams 1..5 end and stream 6 moves into slot 1: one render_range(0, 2) then serves 0 and 1"""
    S, W = 7, 5
    rig = Rig("fast", S, W)
    fs, m = rig.fs, rig.m
    x = [hot(1700 + s, m, W, fs) for s in range(S)]
    for s in range(S):
        rig.put(s, 0, x[s][:, :(W if s == 0 else 2) * fs])
    rig.put(1, 2, x[6][:, 2 * fs:])
    rig.render(0, 0, S, 2)
    rig.flush(1, 5)
    ended = {s: rig.take(s) for s in range(1, 6)}
    nbytes = rig.b.stream_state_bytes()
    blob = rig.torch.zeros(nbytes, dtype=rig.torch.uint8, device="cuda")
    tickets = rig.b.export_range(6, 1, blob.data_ptr(), nbytes, rig.st)
    rig.b.import_range(1, 1, blob.data_ptr(), nbytes, tickets, rig.st)
    rig.render(2, 0, 2, 3)
    rig.flush(0, 2)
    same(rig.take(0), rig.want(x[0]), "stream 0")
    same(np.concatenate([rig.take(6), rig.take(1)], axis=0), rig.want(x[6]), "stream 6, moved to slot 1")
    for s in range(1, 6):
        same(ended[s], rig.want(x[s][:, :2 * fs]), ("ended", s))
    rig.close()


def test_refused_imports_change_nothing():
    import iac_amd as A
    S, W = 3, 4
    rig, other = Rig("fast", S, W), Rig("wide4", 1, 1)
    fs, m = rig.fs, rig.m
    x = [hot(1800 + s, m, W, fs) for s in range(S)]
    for s in range(S):
        rig.put(s, 0, x[s])
    other.put(0, 0, hot(1850, other.m, 1, other.fs, cut_frames=1))
    rig.render(0, 0, S, 2)
    other.render(0, 0, 1, 1)
    nbytes, obytes = rig.b.stream_state_bytes(), other.b.stream_state_bytes()
    assert obytes > nbytes
    blob = rig.torch.zeros((2, obytes), dtype=rig.torch.uint8, device="cuda")
    foreign = other.b.export_range(0, 1, blob.data_ptr(), obytes, other.st)
    own = rig.b.export_range(0, 2, blob.data_ptr(), obytes, rig.st)
    assert foreign[0].signature != own[0].signature
    rig.torch.cuda.synchronize()
    blob.fill_(0x5a)      # if one of the refused calls wrote, the streams would continue from garbage
    bad_bytes = A.StreamState.from_buffer_copy(bytes(own[0]))
    bad_bytes.bytes += 16
    for what, call in (
            ("another out_channels", lambda: rig.b.import_range(0, 1, blob.data_ptr(), obytes, foreign, rig.st)),
            ("wrong bytes", lambda: rig.b.import_range(0, 1, blob.data_ptr(), obytes, [bad_bytes], rig.st)),
            ("stride below bytes", lambda: rig.b.import_range(0, 2, blob.data_ptr(), nbytes - 16, own, rig.st)),
            ("range past the end", lambda: rig.b.import_range(2, 2, blob.data_ptr(), obytes, own, rig.st))):
        with pytest.raises(A.IamfHipError) as e:
            call()
        assert e.value.code == BAD_ARG, what
    rig.render(2, 0, S, 2)
    rig.flush(0, S)
    for s in range(S):
        same(rig.take(s), rig.want(x[s]), ("after the refusals", s))
    rig.close()
    other.close()


def test_lifecycle_kernels_stay_out_of_the_tally():
    """the tally holds render instances only: migrating streams adds nothing to it, and nothing lands in the NONE slot.
    The migration makes three aligned whole-frame calls (render_fast_kernel<16, 2>) and two flushes (the general kernel)."""
    import iac_amd as A
    A.route_reset()
    migrate("fast")
    tally = A.route_tally()
    assert tally == {("FAST", 0, 16, 2, 0): 3, ("GENERIC", 0, 16, 0, 0): 2}, tally
