"""Shared pieces of the tests of iamf_hip_batch_render_ragged (tests/test_gpu_ragged.py, tests/test_ragged_cpu.py): the cases,
the oracle of a run of ragged calls, and the driver that runs a list of steps on one batch.

A step is ("rag", n_frames, n_samples) — the new entry —, ("range", n_frames, n_samples) — iamf_hip_batch_render_range over
the same —, ("flush",), ("reset",) or ("do", name, fn) — fn(batch, stream) between two calls (a restart, new gains, an export
and import).  n_samples == 0: whole frames.  drive() returns one record per step: the value returned, every stream's emitted
bytes (every other byte of the PCM rows asserted 0xA5: gpu_util.rows_and_rest), the exported stream state behind the step
and the tallies of the step.  twin(steps) is the same list with every "rag" turned into "range".

The input of every call is placed by place(): the call's frames under a layout of gpu_util, with EVERY float that is no
sample of the call — the rest of a trimmed frame's rows behind n_samples, the gaps between frames and streams, the slack
around the allocation — set to `fill` (a quiet NaN unless a test says otherwise).  Importing this module needs numpy only."""
import numpy as np

import interleaved_util as IU

FAM = "FAST_RAGGED"
RAGGED_M = (1, 2, 4, 6, 8, 9, 10, 12, 16)       # RaggedM x RaggedOC of render_route.hpp
INSTANCES = [(m, oc) for m in RAGGED_M for oc in (1, 2)]
BD_FMT = IU.BD_FMT
S = 3
EG, OG = IU.EG, IU.OG
RAG = "RAG"       # a step's expected route: the form's own row; else a key of the base tally

# name: (m, oc, frame size, [(n_frames, n_samples)] of the calls) — what tests/test_gpu_ragged.py renders and
# tests/test_ragged_cpu.py proves hot across every call boundary
CASES = {
    "frame_1000": (16, 2, 1000, [(1, 0), (1, 0)]),
    "lengths": (16, 2, 2048, [(1, n) for n in (1000, 1, 3, 63, 65, 1023, 1025, 480)]),
    "frames_100": (9, 2, 100, [(3, 0)] * 4),
    "frames_1000": (6, 2, 1000, [(5, 0), (5, 0)]),
    "mod4": (4, 2, 2048, [(1, 1001), (1, 1002), (1, 1003)]),
    "first_100": (2, 2, 1000, [(1, 100), (1, 0), (1, 0)]),
    "mixed": (16, 2, 1000, [(1, 0), (8, 0), (1, 0), (8, 0), (1, 0)]),
}


def inst(m, oc):
    return (FAM, 0, m, oc, 0)


def gen(m):
    return ("GENERIC", 0, m, 0, 0)


def fast(m, oc):
    return ("FAST", 0, m, oc, 0)


def samples(fs, call):
    return call[1] if call[1] else call[0] * fs


def sizes(fs, calls):
    return [samples(fs, c) for c in calls]


def twin(steps):
    return [("range",) + tuple(s[1:]) if s[0] == "rag" else s for s in steps]


def default_routes(fs, calls):
    """per call: RAG where ragged_shape_ok's length and position rules hold, the fast kernel for whole blocks at such a
    position, else the general kernel (m, oc filled in by check)"""
    out, pos = [], 0
    for c in calls:
        n = samples(fs, c)
        pos_ok = pos % 16 == 0 or pos >= 240
        out.append((RAG if n % 64 else "FAST") if pos_ok else "GENERIC")
        pos += n
    return out


def hot(m, total, streams=S, seed=4100):
    """THE programme of the GPU tests, [streams][m][total]: noise with 1.5 bursts of 240 samples every 700, stream s's first
    burst from sample 30 + 20 s on — inside the first call of every test, the shortest of which has 100 samples; the limiter
    is then never idle again (its release takes 9600).  Stream s is the same whatever `streams` is."""
    import synth
    return np.stack([synth.hot(seed + 11 * s, m, total, sigma=0.2, burst_phase=30 + 20 * s, burst_period=700) for s in range(streams)])


def programme(name):
    """the input of a case of CASES: hot() for its element and its length"""
    m, _, fs, calls = CASES[name]
    return hot(m, sum(sizes(fs, calls)))


def proofs():
    """Every (programme, matrix, gains, calls) a limiter-on GPU test of tests/test_gpu_ragged.py renders, for
    tests/test_ragged_cpu.py to prove hot across every call boundary: (label, m, oc, fs, calls, streams, eg, og); eg / og:
    per stream (cycled), a constant or one value per call.  Input is hot(m, total, streams) and the matrix
    interleaved_util.dense_matrices(m, oc) in every one of them.  Not here: the second-element fall-back (its mix has no
    oracle in these tests) and the limiter-off one."""
    two, three = [(1, 0), (1, 0)], [(1, 0)] * 3
    out = [(name,) + CASES[name] + (S, EG, OG) for name in sorted(CASES)]
    out += [("instance %d -> %d" % (m, oc), m, oc, 1000, two, S, EG, OG) for m, oc in INSTANCES]       # test_every_instance
    out += [("both entries / stalled streams", 16, 2, 1000, three, S, EG, OG),
            ("lifecycle, streams 0 and 1 up to the restart", 9, 2, 1000, three, 2, [[0.8, 1.1, 1.1], 1.0], [[1.0, 0.7, 0.7], 0.9]),
            ("range of streams", 16, 2, 1000, two, 4, EG, OG),
            ("fall-back, M = 14", 14, 2, 1000, two, S, EG, OG),
            ("fall-back, 6 output channels", 16, 6, 1000, two, S, EG, OG),
            ("fall-back, an output ramp of 0.5 (in place of the output gain)", 16, 2, 1000, two, S, EG, [0.5])]
    return out


def want(omx, oc, x, sz, bd=16, eg=1.0, og=1.0, flush=True):
    """the oracle of one stream over calls of sz samples; eg, og: a constant, or one value per call
    -> (PCM as interleaved_util.want, the limiter's input [oc][total])"""
    import oracle_lib as O
    if not isinstance(eg, (list, tuple)) and not isinstance(og, (list, tuple)):
        return IU.want(omx, oc, x, list(sz), bd, eg, og, flush=flush)
    egs = list(eg) if isinstance(eg, (list, tuple)) else [eg] * len(sz)
    ogs = list(og) if isinstance(og, (list, tuple)) else [og] * len(sz)
    y = np.ascontiguousarray(O.render(omx, x, oc), dtype=np.float32)
    parts, pos = [], 0
    for n, e, o in zip(sz, egs, ogs):
        seg = np.ascontiguousarray(y[:, pos:pos + n])
        O.lib().orc_frame_gain_const(O.fp(seg), oc, n, float(e))
        seg = np.ascontiguousarray(np.zeros_like(seg) + seg, dtype=np.float32)
        O.lib().orc_frame_gain_const(O.fp(seg), oc, n, float(o))
        parts.append(seg)
        pos += n
    z = np.ascontiguousarray(np.concatenate(parts, axis=1))
    pre = z.copy()
    with np.errstate(all="ignore"):
        z, _ = O.limiter_run(z, list(sz), flush=flush)
    return (np.ascontiguousarray(z.T) if bd == -32 else O.pack(z, bd)), pre


def place(xc, nf, fs, layout, fill, backend=None):
    """xc [S][m][n], n <= nf * fs: the call's samples as nf frames [m][fs] per stream under `layout` (gpu_util's table); every
    other float of the allocation is `fill`.  -> (keep, d_in, in_stream_stride, in_frame_stride)"""
    import gpu_util as G
    backend = backend or G.TORCH
    Sx, m, n = xc.shape
    off, fst, sst = G.input_geometry(layout, Sx, nf, m, fs)
    e = m * fs
    slack = (e + 63) & ~63
    first = slack + off
    host = np.full(first + (Sx - 1) * sst + (nf - 1) * fst + e + slack, fill, dtype=np.float32)
    fr = np.full((Sx, m, nf * fs), fill, dtype=np.float32)
    fr[:, :, :n] = xc
    fr = fr.reshape(Sx, m, nf, fs)
    for s in range(Sx):
        for f in range(nf):
            a = first + s * sst + f * fst
            host[a:a + e] = fr[s, :, f].reshape(-1)
    t = backend.upload(host)
    return t, backend.ptr(t) + 4 * first, sst, fst


def drive(amx, m, oc, fs, x, steps, bd=16, eg=EG, og=OG, layout=None, fill=np.nan, rng=None, second=None, out_ramp=False,
          limiter=True, export=True, out_stream=None, before_call=None):
    """x [S][m][total].  layout: gpu_util's (PAD16 unless named), for the input and the PCM rows; rng: (s0, cnt) — every
    call over that range only; second: (matrix, x2 [S][m2][total]) — a second element on the batch; out_ramp: an all-0.5
    output ramp on every call; limiter: the batch's; out_stream: the stream of every call (torch's current one unless given);
    before_call(k, stream): called when every buffer of render step k is in place, may return a callable that is called
    directly behind the call (its value is the record's "note")."""
    import torch
    import iac_amd as A
    import gpu_util as G
    layout = layout or G.PAD16
    Sx = x.shape[0]
    fmt = getattr(A, BD_FMT[bd])
    bps = {16: 2, 24: 3, 32: 4, -32: 4}[bd]
    st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
    s0, cnt = rng or (0, Sx)
    b = A.Batch(Sx, amx, oc, frame_size=fs, out_format=fmt, projection=A.PROJ_EXACT, limiter=limiter)
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

        for k, step in enumerate(steps):
            A.route_reset()
            A.route_family_tally(FAM, reset=True)
            if step[0] in ("reset", "do"):
                if step[0] == "reset":
                    b.reset()
                    pos = 0
                else:
                    step[2](b, st)
                torch.cuda.synchronize()
                recs.append(dict(step=step, ret=0, pcm=[np.zeros(0, np.uint8)] * Sx, state=exported(), fam={}, base={}))
                continue
            keep = []
            after = None
            if step[0] == "flush":
                rows, d_pcm, stride = G.pcm_rows(Sx, 240 * oc * bps, layout, bps)
                ret = b.flush_range(d_pcm, stride, st, s0, cnt)
            else:
                nf, n = step[1], samples(fs, step[1:])
                rows, d_pcm, stride = G.pcm_rows(Sx, max(n, 240) * oc * bps, layout, bps)
                t, d_in, sst, fst = place(x[:, :, pos:pos + n], nf, fs, layout, fill)
                keep.append(t)
                a = A.RenderArgs()
                a.d_in, a.in_stream_stride, a.in_frame_stride = d_in, sst, fst
                a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, step[2], d_pcm, stride, st
                if second:
                    t2, a.d_in2, a.in2_stream_stride, a.in2_frame_stride = place(second[1][:, :, pos:pos + n], nf, fs, G.second_layout(layout), fill)
                    keep.append(t2)
                if out_ramp:
                    d_r = torch.full((Sx, nf * fs + 4), 0.5, dtype=torch.float32, device="cuda")
                    keep.append(d_r)
                    a.d_output_ramp, a.ramp_stream_stride = d_r.data_ptr(), nf * fs + 4
                after = before_call(k, st) if before_call else None
                ret = b.render_ragged(a, s0, cnt) if step[0] == "rag" else b.render_range(a, s0, cnt)
                pos += n
            note = after() if after else None
            torch.cuda.synchronize()
            pcm = G.rows_and_rest(rows, layout, ret * oc * bps, only=(s0, cnt))
            recs.append(dict(step=step, ret=ret, pcm=pcm, state=exported(), fam=A.route_family_tally(FAM, reset=True),
                             base=A.route_tally(), note=note))
    finally:
        b.close()
    return recs


stream_pcm = IU.stream_pcm
assert_same = IU.assert_same


def assert_tallies(recs, m, oc, routes, what=""):
    """routes, per step: RAG (the instance's row once, nothing in the base tally), "FAST" / "GENERIC" / a key of the base
    tally (that row once, the family's tally empty), None (a "do" or "reset" step: nothing launched)"""
    for k, (r, f) in enumerate(zip(recs, routes)):
        if f is None or r["step"][0] in ("reset", "do"):
            assert r["fam"] == {} and r["base"] == {}, (what, "step %d" % k, r["fam"], r["base"])
            continue
        if f == RAG:
            assert r["step"][0] == "rag" and r["fam"] == {inst(m, oc): 1} and r["base"] == {}, (what, "step %d" % k, r["fam"], r["base"])
        else:
            key = {"FAST": fast(m, oc), "GENERIC": gen(m)}.get(f, f)
            assert r["fam"] == {} and r["base"] == {key: 1}, (what, "step %d" % k, r["fam"], r["base"], key)


def check(m, oc, fs, x, calls, bd=16, mats=None, routes=None, what="", eg=EG, og=OG, oracle=True, flush=True, entries=None, **kw):
    """`calls` through the new entry (entries: per call "rag" or "range") and a flush; a twin through
    iamf_hip_batch_render_range; the oracle.  routes: per call what the new entry's batch must have run (default_routes);
    the twin must have run the same, with the general kernel in place of RAG.  -> (records, twin's records)"""
    amx, omx = mats or IU.dense_matrices(m, oc)
    entries = entries or ["rag"] * len(calls)
    steps = [(e,) + tuple(c) for e, c in zip(entries, calls)] + ([("flush",)] if flush else [])
    routes = list(routes or default_routes(fs, calls)) + (["GENERIC"] if flush else [])
    got = drive(amx, m, oc, fs, x, steps, bd=bd, eg=eg, og=og, **kw)
    ref = drive(amx, m, oc, fs, x, twin(steps), bd=bd, eg=eg, og=og, **kw)
    assert_tallies(got, m, oc, routes, what)
    assert_tallies(ref, m, oc, ["GENERIC" if r == RAG else r for r in routes], what + " (twin)")
    assert_same(got, ref, what)
    if oracle:
        import test_gpu_programmes as TP
        s0, cnt = kw.get("rng") or (0, x.shape[0])
        sz = sizes(fs, calls)
        for s in range(s0, s0 + cnt):
            w, _ = want(omx, oc, x[s][:, :sum(sz)], sz, bd, eg[s % len(eg)], og[s % len(og)], flush=flush)
            g = stream_pcm(got, s, oc, bd)
            assert TP.mismatch(g, w) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, w))
    return got, ref
