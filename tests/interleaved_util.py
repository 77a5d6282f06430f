"""Shared pieces of the tests of iamf_hip_batch_render_interleaved (tests/test_gpu_interleaved.py, tests/test_interleaved_cpu.py):
the programmes, the oracle of a run of ragged calls, and the driver that runs a list of steps on one batch.

A step is ("il", n) — the new entry over n sample-frames —, ("range", n) — iamf_hip_batch_render_range over the same —,
("flush",) or ("reset",).  drive() returns one record per step: the value returned, every stream's emitted bytes (every other
byte of the PCM rows asserted 0xA5: gpu_util.rows_and_rest), the exported stream state behind the step and the tallies of
the step.  twin(steps) is the same list with every "il" turned into "range".  Importing this module needs numpy only."""
import numpy as np

FAM = "FAST_INTERLEAVED"
INSTANCES = [(m, oc) for m in (1, 2) for oc in (1, 2)]        # InterleavedM x InterleavedOC of render_route.hpp
BD_FMT = {16: "FMT_S16", 24: "FMT_S24", 32: "FMT_S32", -32: "FMT_F32"}
S = 3
EG, OG = [0.8, 1.0, 1.2], [1.0, 0.9, 1.0]


def inst(m, oc):
    return (FAM, 0, m, oc, 0)


def gen(m):
    return ("GENERIC", 0, m, 0, 0)


def twin(steps):
    return [("range",) + tuple(s[1:]) if s[0] == "il" else s for s in steps]


def dense_matrices(m, oc):
    """(product matrix, oracle matrix): seeded, dense, every (channel, slot) a weight of its own magnitude — a kernel that
    swapped left and right in its transpose shows"""
    import route_cases as R
    return R.matrices(m, oc, table=False)


def identity_matrices(ch):
    import iac_amd as A
    import oracle_lib as O
    import route_cases as R
    return R._custom(A, O, A.KIND_M2M, ch, ch, np.eye(ch, dtype=np.float32), ch)


def hot(m, total, streams=S, seed=3100):
    """per stream: noise with 1.5 bursts of 240 samples every 700, at a phase of its own — several trigger runs per call of
    1115, across every call boundary of the tests' length sequences"""
    import synth
    return np.stack([synth.hot(seed + 11 * s, m, total, sigma=0.2, burst_phase=90 + 173 * s, burst_period=700) for s in range(streams)])


def want(omx, oc, x, sizes, bd=16, eg=1.0, og=1.0, flush=True, sample_rate=48000, threshold_db=-1.0):
    """the oracle of one stream: x [m][total] rendered, the constant gains, the mixer's 0 + y, the limiter over calls of
    `sizes` (and its flush), packed -> (PCM [n][oc] (s24: [n][oc][3]), the limiter's input [oc][total])"""
    import oracle_lib as O
    y = np.ascontiguousarray(O.render(omx, x, oc), dtype=np.float32)
    n = y.shape[1]
    O.lib().orc_frame_gain_const(O.fp(y), oc, n, float(eg))      # (skips 1.0 and non-positive gains, as the reference)
    z = np.ascontiguousarray(np.zeros_like(y) + y, dtype=np.float32)
    O.lib().orc_frame_gain_const(O.fp(z), oc, n, float(og))
    pre = z.copy()
    with np.errstate(all="ignore"):
        z, _ = O.limiter_run(z, sizes, flush=flush, rate=sample_rate, thr_db=threshold_db)
    return (np.ascontiguousarray(z.T) if bd == -32 else O.pack(z, bd)), pre


# ---- the limiter at the seam: programmes placed by the oracle's trace ----

SEAM_LENGTHS = [1115, 1114, 1115]
# the gain step (= index of the input sample that enters at it) at which each stream's FIRST trigger falls: the last sample
# of the ragged first call, the first sample of the second call, and inside the partial last block of the first call (its
# 64-blocks start at 1088: samples 1088 .. 1114 are real, 1115 .. 1151 absent)
SEAM_TRIGGERS = [1114, 1115, 1100]


def first_trigger(x, sizes):
    import oracle_lib as O
    _, tr = O.limiter_trace(np.ascontiguousarray(x, dtype=np.float32), sizes)
    hits = np.flatnonzero(tr & O.LIM_TRIGGER)
    return int(hits[0]) if hits.size else None, tr


def seam_plateau():
    """per stream: zeros, then programmes.dc_one_ulp_above from an onset chosen so that the first trigger falls on
    SEAM_TRIGGERS[s].  The onset comes from the oracle's trace of a probe (zeros in front: the placement shifts with the onset).
    -> (x [3][2][total], lengths, onsets)"""
    import programmes as P
    total = sum(SEAM_LENGTHS)
    probe = np.zeros((2, total), dtype=np.float32)
    probe[:, 500:] = P.dc_one_ulp_above(2, total - 500)
    lag = first_trigger(probe, SEAM_LENGTHS)[0] - 500
    x, onsets = np.zeros((3, 2, total), dtype=np.float32), []
    for s, t in enumerate(SEAM_TRIGGERS):
        x[s, :, t - lag:] = P.dc_one_ulp_above(2, total - (t - lag))
        onsets.append(t - lag)
    return x, SEAM_LENGTHS, onsets


RETRIGGER_LENGTHS = [341, 4097, 4099, 2049]     # the first run's last trigger (programmes.LAST_TRIGGER = 340) ends call 0
RETRIGGER_K = [0, 3, 5]                         # re-trigger in the attack, in the early release, and one step before idle


def seam_retrigger():
    """programmes.retrigger_sweep for three k: the lone impulse's last trigger is the LAST sample of the ragged first call, the
    release then runs across the three calls behind it, and the 3.0 impulse re-triggers in the second call (k = 0, 3) or in
    the fourth (k = 5).  -> (x [3][2][total], lengths, k)"""
    import programmes as P
    total = sum(RETRIGGER_LENGTHS)
    return np.stack([P.retrigger_sweep(2, total, k=k) for k in RETRIGGER_K]), RETRIGGER_LENGTHS, RETRIGGER_K


def drive(amx, m, oc, x, steps, bd=16, streams=None, eg=EG, og=OG, pad=0, off_floats=0, rng=None, out_stream=None,
          before_call=None, second=None, out_ramp=False, frame_size=1, export=True, sample_rate=48000, threshold_db=-1.0):
    """x [S][m][total].  pad: floats between sample-frames (in_frame_stride = m + pad); off_floats: d_in that many floats
    behind a 256-byte aligned base; rng: (s0, cnt) — every step over that range only; second: (matrix, x2 [S][m2][total]) —
    a second element on the batch; out_ramp: an all-0.5 output ramp on every call; sample_rate, threshold_db: the batch's."""
    import torch
    import iac_amd as A
    import gpu_util as G
    Sx = x.shape[0] if streams is None else streams
    fmt = getattr(A, BD_FMT[bd])
    bps = {16: 2, 24: 3, 32: 4, -32: 4}[bd]
    st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
    s0, cnt = rng or (0, Sx)
    b = A.Batch(Sx, amx, oc, frame_size=frame_size, out_format=fmt, projection=A.PROJ_EXACT, sample_rate=sample_rate,
                threshold_db=threshold_db)
    recs, pos = [], 0
    try:
        b.set_gains(element=[eg[s % len(eg)] for s in range(Sx)], output=[og[s % len(og)] for s in range(Sx)])
        if second:
            b.set_second_element(second[0], [1.0] * Sx)
        sb = b.stream_state_bytes()

        def exported():
            if not export:
                return None
            d_state = torch.zeros((Sx, sb), dtype=torch.uint8, device="cuda")
            tickets = b.export_range(0, Sx, d_state.data_ptr(), sb, st)
            torch.cuda.synchronize()
            return d_state.cpu().numpy(), [(t.bytes, t.cursor[0], t.cursor[1]) for t in tickets]

        def placed(xi, n, mch):
            """[S][mch][n] -> device floats: stream s's sample-frames dense (or padded) from off_floats on, quiet NaNs between"""
            fstride = mch + pad
            ss = ((off_floats + n * fstride + 3) & ~3) + 4
            h = np.full((Sx, ss), np.nan, dtype=np.float32)
            for s in range(Sx):
                h[s, off_floats:off_floats + n * fstride].reshape(n, fstride)[:, :mch] = xi[s].T
            return torch.from_numpy(h).cuda(), ss, fstride

        for k, step in enumerate(steps):
            A.route_reset()
            A.route_family_tally(FAM, reset=True)
            if step[0] == "reset":
                b.reset()
                pos = 0
                recs.append(dict(step=step, ret=0, pcm=[np.zeros(0, np.uint8)] * Sx, state=exported(), fam={}, base={}))
                continue
            n = 240 if step[0] == "flush" else step[1]
            rows, d_pcm, stride = G.pcm_rows(Sx, max(n, 240) * oc * bps, G.PAD16, bps)
            keep = []
            after = None
            if step[0] == "flush":
                after = before_call(k, st) if before_call else None
                ret = b.flush_range(d_pcm, stride, st, s0, cnt)
            else:
                d_x, ss, fstride = placed(x[:, :, pos:pos + n], n, m)
                keep.append(d_x)
                a = A.RenderArgs()
                a.d_in, a.in_stream_stride, a.in_frame_stride = d_x.data_ptr() + 4 * off_floats, ss, fstride
                a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n, d_pcm, stride, st
                if second:
                    m2 = second[1].shape[1]
                    d_x2, ss2, fstride2 = placed(second[1][:, :, pos:pos + n], n, m2)
                    keep.append(d_x2)
                    a.d_in2, a.in2_stream_stride, a.in2_frame_stride = d_x2.data_ptr() + 4 * off_floats, ss2, fstride2
                if out_ramp:
                    d_r = torch.full((Sx, n + 4), 0.5, dtype=torch.float32, device="cuda")
                    keep.append(d_r)
                    a.d_output_ramp, a.ramp_stream_stride = d_r.data_ptr(), n + 4
                after = before_call(k, st) if before_call else None      # (every buffer of the call is in place)
                ret = b.render_interleaved(a, s0, cnt) if step[0] == "il" else b.render_range(a, s0, cnt)
                pos += n
            note = after() if after else None
            torch.cuda.synchronize()
            pcm = G.rows_and_rest(rows, G.PAD16, ret * oc * bps, only=(s0, cnt))
            recs.append(dict(step=step, ret=ret, pcm=pcm, state=exported(), fam=A.route_family_tally(FAM, reset=True),
                             base=A.route_tally(), note=note))
    finally:
        b.close()
    return recs


def stream_pcm(recs, s, oc, bd):
    """everything stream s emitted over the steps, as the oracle's want() shapes it"""
    import iac_amd as A
    import gpu_util as G
    raw = np.concatenate([r["pcm"][s] for r in recs])
    bps = {16: 2, 24: 3, 32: 4, -32: 4}[bd]
    return G._view(raw, raw.size // (oc * bps), oc, getattr(A, BD_FMT[bd]))


def assert_same(got, ref, what=""):
    """step by step: the value returned, every stream's bytes and the exported state (blob and tickets)"""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["ret"] == r["ret"], (what, "step %d returned" % k, g["ret"], r["ret"])
        for s, (a, b) in enumerate(zip(g["pcm"], r["pcm"])):
            assert np.array_equal(a, b), (what, "step %d, stream %d: PCM against the twin" % (k, s),
                                          int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else (a.shape, b.shape))
        if g["state"] is not None:
            assert g["state"][1] == r["state"][1], (what, "step %d: tickets" % k, g["state"][1], r["state"][1])
            assert np.array_equal(g["state"][0], r["state"][0]), (what, "step %d: the exported state against the twin's" % k)


def assert_tallies(recs, m, oc, fused, what=""):
    """fused: per step True (the instance's row once, nothing in the base tally), False (GENERIC once, the family's tally
    empty) — flush steps are GENERIC by themselves, reset steps launch nothing"""
    for k, (r, f) in enumerate(zip(recs, fused)):
        if r["step"][0] == "reset":
            continue
        if r["step"][0] == "il" and f:
            assert r["fam"] == {inst(m, oc): 1} and r["base"] == {}, (what, "step %d" % k, r["fam"], r["base"])
        else:
            assert r["fam"] == {} and r["base"] == {gen(m): 1}, (what, "step %d" % k, r["fam"], r["base"])


def check(m, oc, x, lengths, bd=16, mats=None, fused=None, what="", eg=EG, og=OG, **kw):
    """calls of `lengths` through the new entry and a flush; a twin through iamf_hip_batch_render_range; the oracle.
    fused: per call whether the family's row is expected (default: from the second call on, or from the first if it starts
    at a multiple of 16 — which position 0 is).  -> (records, twin's records)"""
    amx, omx = mats or dense_matrices(m, oc)
    steps = [("il", n) for n in lengths] + [("flush",)]
    got = drive(amx, m, oc, x, steps, bd=bd, eg=eg, og=og, **kw)
    ref = drive(amx, m, oc, x, twin(steps), bd=bd, eg=eg, og=og, **kw)
    if fused is None:
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        fused = [bool(p % 16 == 0 or p >= 240) for p in starts]
    assert_tallies(got, m, oc, list(fused) + [False], what)
    assert_tallies(ref, m, oc, [False] * len(steps), what)
    assert_same(got, ref, what)
    import test_gpu_programmes as TP
    s0, cnt = kw.get("rng") or (0, x.shape[0])
    for s in range(s0, s0 + cnt):
        w, pre = want(omx, oc, x[s][:, :sum(lengths)], list(lengths), bd, eg[s % len(eg)], og[s % len(og)],
                      sample_rate=kw.get("sample_rate", 48000), threshold_db=kw.get("threshold_db", -1.0))
        g = stream_pcm(got, s, oc, bd)
        assert TP.mismatch(g, w) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, w))
    return got, ref
