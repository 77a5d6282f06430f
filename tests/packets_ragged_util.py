"""Shared pieces of the tests of iamf_hip_batch_render_packets_ragged (tests/test_gpu_zz_packets_ragged.py,
tests/test_packets_ragged_cpu.py): the forms and instances, the programme on the packets' integer grid, the oracle of a run of
calls, and the driver that runs a list of steps on one batch.

A step is ("prag", n_frames, n_samples[, first_sample]) — the new entry —, ("packets", ...) — iamf_hip_batch_render_packets
over the same —, ("rag" | "range", n_frames, n_samples) — the f32 entries iamf_hip_batch_render_ragged / _range over the same
samples as planar f32 —, ("flush",), ("reset",) or ("do", name, fn) — fn(batch, stream) between two calls.  n_samples == 0:
whole frames.  drive() returns one record per step: the value returned, every stream's emitted bytes (every other byte of the
PCM rows asserted 0xA5: gpu_util.rows_and_rest), the exported stream state behind the step and the tallies of the step.
twin(steps) is the same list with every "prag" turned into "packets".

The packets of every call are built by packets_of(): the call's frames as lpcm_util.rows lays them out, with EVERY byte that
is no sample of the call — the rest of a trimmed frame's runs in front of first_sample and behind n_samples, the gaps between
the runs, the rows' padding — set to `fill`.  Importing this module needs numpy only."""
import numpy as np

import interleaved_util as IU
import ragged_util as RU

FAM = "PACKETS_RAGGED"
FAMILY = 37
# form: (bytes per sample, coupled) — the four single-element packet forms of lpcm_form.hpp
FORMS = {"s16": (2, False), "s16c": (2, True), "s24": (3, False), "s24c": (3, True)}
MONO_M = (1, 4, 9, 16)              # LpcmM of render_route.hpp
COUPLED_M = (2, 6, 8, 10, 12)       # LpcmCoupledM
INSTANCES = [(form, m, oc) for form in ("s16", "s16c", "s24", "s24c") for m in (COUPLED_M if FORMS[form][1] else MONO_M) for oc in (1, 2)]
# the whole-block family of each form and the variant the host's rule picks for a few streams
WHOLE = {"s16": "LPCM", "s16c": "LPCM_COUPLED", "s24": "LPCM24", "s24c": "LPCM24_COUPLED"}
OTHER_FAMILIES = ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED", "LPCM24_COUPLED", "LPCM24_MIX")
PACKET_FED = ("LPCM", "LPCM24", "FANOUT_LPCM", "LPCM_COUPLED", "LPCM_MIX", "LPCM24_COUPLED", "LPCM24_MIX", FAM)
S = 3
EG, OG = RU.EG, RU.OG
PRAG = "PRAG"       # a step's expected route: the family's own row; WHOLE_ROW: the form's whole-block row; else a key of the base tally
WHOLE_ROW = "WHOLE"
BD_FMT = IU.BD_FMT

# name: (form, m, oc, frame size, [(n_frames, n_samples[, first_sample])] of the calls) — what the GPU tests render and
# tests/test_packets_ragged_cpu.py proves hot across every call boundary
CASES = {
    "frame_1000": ("s16", 16, 2, 1000, [(1, 0), (1, 0)]),
    "lengths": ("s24", 16, 2, 2048, [(1, n) for n in (1000, 1, 3, 63, 65, 1023, 1025, 480)]),
    "lengths_coupled": ("s16c", 6, 2, 2048, [(1, n) for n in (1000, 1, 3, 63, 65, 1023, 1025, 480)]),
    "frames_100": ("s24c", 12, 2, 100, [(3, 0)] * 4),
    "frames_100_mono": ("s16", 9, 2, 100, [(3, 0)] * 4),
    "frames_1000": ("s16c", 6, 2, 1000, [(5, 0), (5, 0)]),
    "frames_1000_s24": ("s24", 4, 1, 1000, [(5, 0), (5, 0)]),
    "mod4_s16": ("s16", 4, 2, 2048, [(1, 1001), (1, 1002), (1, 1003)]),
    "mod4_s16c": ("s16c", 8, 2, 2048, [(1, 1001), (1, 1002), (1, 1003)]),
    "mod4_s24": ("s24", 9, 2, 2048, [(1, 1001), (1, 1002), (1, 1003)]),
    "mod4_s24c": ("s24c", 10, 2, 2048, [(1, 1001), (1, 1002), (1, 1003)]),
}


# the shapes of the placement, PCM-format and hand-over tests
PLACED = (("s16", 4), ("s16c", 6), ("s24", 9), ("s24c", 2))
PCM_SHAPES = (("s16c", 6, 2), ("s24", 4, 1))
HANDOVER = (("s16", 4), ("s24c", 6))
# per boundary (frame size): the calls with a whole-block call in the middle, and with three ragged ones
HANDOVER_CALLS = {1000: {"whole": [(1, 0), (8, 0), (1, 0)], "ragged": [(1, 0)] * 3}, 100: {"whole": [(3, 0), (16, 0), (3, 0)], "ragged": [(3, 0)] * 3}}


def inst(form, m, oc):
    return (FAM, 0, m, oc, FORMS[form][0])


def whole(form, m, oc):
    return (WHOLE[form], 1, m, oc, 0)


gen, fast, samples, sizes = RU.gen, RU.fast, RU.samples, RU.sizes


def rag(m, oc):
    return ("FAST_RAGGED", 0, m, oc, 0)


def twin(steps):
    return [("packets",) + tuple(s[1:]) if s[0] == "prag" else s for s in steps]


def default_routes(fs, calls):
    """per call: PRAG where packets_ragged_shape_ok's length and position rules hold (render_route.hpp), the form's whole-block
    family for whole blocks at such a position, else the general kernel behind the unpacker"""
    out, pos = [], 0
    for c in calls:
        n = samples(fs, c)
        pos_ok = pos % 16 == 0 or pos >= 240
        out.append((PRAG if n % 64 else WHOLE_ROW) if pos_ok else "GENERIC")
        pos += n
    return out


def coupled(m):
    """-> (widths, perm) of lpcm_util.rows for a loudspeaker layout of m channels: sub-streams in audio-layer order (the
    coupled pairs, then C and LFE), perm[p] = the decoded channel playback channel p takes (L R C LFE, then the pairs)"""
    if m <= 2:
        return [m], list(range(m))
    return [2] * ((m - 2) // 2) + [1, 1], [0, 1, m - 2, m - 1] + list(range(2, m - 2))


def layout_of(form, m):
    return coupled(m) if FORMS[form][1] else ([1] * m, list(range(m)))


def quantise(x, bps):
    """f32 [..] -> the nearest integers of the packets' grid, clipped to it (int64)"""
    full = float(1 << (8 * bps - 1))
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * full), -full, full - 1).astype(np.int64)


def as_f32(ints, bps):
    """ints / 2^15 or / 2^23: the reference's LPCM decode, exact in f32"""
    return (ints.astype(np.float64) / float(1 << (8 * bps - 1))).astype(np.float32)


def hot_ints(form, m, total, streams=S):
    """THE programme of the GPU tests on the form's grid, [streams][m][total] in playback order: ragged_util.hot() quantised"""
    return quantise(RU.hot(m, total, streams), FORMS[form][0])


def programme(name):
    form, m, _, fs, calls = CASES[name]
    return hot_ints(form, m, sum(sizes(fs, calls)))


def proofs():
    """Every (programme, matrix, gains, calls) a limiter-on GPU test of tests/test_gpu_zz_packets_ragged.py renders with the
    constant-hot programme, for tests/test_packets_ragged_cpu.py to prove hot across every call boundary:
    (label, form, m, oc, fs, calls, streams).  Input is hot_ints(form, m, total, streams), the matrix
    interleaved_util.dense_matrices(m, oc), the gains EG / OG in every one of them."""
    two = [(1, 0), (1, 0)]
    out = [(name,) + CASES[name] + (S,) for name in sorted(CASES)]
    out += [("instance %s %d -> %d" % (f, m, oc), f, m, oc, 1000, two, S) for f, m, oc in INSTANCES]
    for form, m in (("s16", 4), ("s16c", 6), ("s24", 4), ("s24c", 6)):
        out += [("trimmed start %d, %s" % (first, form), form, m, 2, 1000, [(1, 1000 - first, first), (1, 0)], S) for first in (4, 100, 240)]
    for form in ("s16c", "s24c"):
        out += [("stereo from first sample 2, %d samples, %s" % (n, form), form, 2, 2, 1000, [(1, n, 2), (1, 0)], S) for n in (993, 996, 997, 998)]
    mod4 = [(1, 1001), (1, 1002), (1, 1003)]
    out += [("placement / range, %s" % form, form, m, 2, 1000, two, 4) for form, m in PLACED]
    out += [("PCM formats, %s %d -> %d" % (form, m, oc), form, m, oc, 2048, mod4, S) for form, m, oc in PCM_SHAPES]
    out += [("sequence", "s16", 4, 2, 1000, [(1, 0), (8, 0), (1, 0), (1, 0)], S), ("stalled streams", "s16c", 6, 2, 1000, [(1, 0)] * 3, S)]
    for form, m in HANDOVER:
        for fs, calls in HANDOVER_CALLS.items():
            out += [("hand-over at %d, %s, %s" % (fs, form, k), form, m, 2, fs, c, S) for k, c in calls.items()]
    return out


def want(omx, oc, ints, bps, sz, bd=16, eg=1.0, og=1.0, flush=True, rate=48000):
    """the oracle of one stream, ints [m][total] in playback order, over calls of sz samples"""
    x = np.ascontiguousarray(as_f32(ints, bps)[:, :sum(sz)])
    if rate != 48000:
        return IU.want(omx, oc, x, list(sz), bd, eg, og, flush=flush, sample_rate=rate)
    return RU.want(omx, oc, x, sz, bd, eg, og, flush=flush)


def packets_of(form, ints, nf, fs, first=0, fill=0, head=16, pad=0):
    """ints [S][m][n] in playback order, n <= nf * fs - first: the call's packets, nf frames per stream as lpcm_util.rows lays
    them out (sample k of the call at position first + k of the runs), every byte that is no sample of the call = fill
    -> (raw [S][nf][row] uint8, layout, row)"""
    import lpcm_util as LP
    bps, _ = FORMS[form]
    Sx, m, n = ints.shape
    widths, perm = layout_of(form, m)
    assert first + n <= nf * fs
    play = np.zeros((Sx, m, nf * fs), dtype=np.int64)
    mark = np.zeros((Sx, m, nf * fs), dtype=np.int64)
    play[:, :, first:first + n] = ints
    mark[:, :, first:first + n] = -1                       # every byte of a sample of the call: 0xFF
    out = []
    for v in (play, mark):
        dec = np.zeros((Sx, nf, m, fs), dtype=np.int64)
        dec[:, :, perm, :] = v.reshape(Sx, m, nf, fs).transpose(0, 2, 1, 3)     # playback channel p is decoded channel perm[p]
        out.append(LP.rows(dec, bps, True, widths, perm, head=head, pad=pad, frame_size=fs))
    (raw, L, row), (mask, _, _) = out
    return np.where(mask == 0xFF, raw, np.uint8(fill)), L, row


def _reset(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    for f in (FAM,) + OTHER_FAMILIES:
        A.route_family_tally(f, reset=True)


def _tallies(A):
    """-> (the family's tally, table 0, everything else that lists a kernel as one dict), all reset"""
    fam, base = A.route_family_tally(FAM, reset=True), A.route_tally()
    rest = dict(A.route_tally_ext())
    rest.update(A.route_table_tally(2, reset=True))
    for f in OTHER_FAMILIES:
        rest.update(A.route_family_tally(f, reset=True))
    A.route_reset()
    A.route_tally_ext(reset=True)
    return fam, base, rest


def drive(amx, form, oc, fs, ints, steps, bd=16, eg=EG, og=OG, layout=None, fill=0, rng=None, second=None, limiter=True,
          export=True, out_stream=None, before_call=None, packets=None, head=16, pad=0, batch_kw=None, le=True, rate=48000, edit_layout=None):
    """ints [S][m][total] in playback order.  layout: gpu_util's, for the PCM rows (and the f32 steps' input; PAD16 unless
    named); packets: a packet layout of gpu_util (place_packets; None: the rows as they are, dense); fill: the byte of
    packets_of; rng: (s0, cnt) — every call over that range only; second: a matrix — a second element on the batch;
    before_call(k, stream): as ragged_util.drive; le False: the packets big-endian; edit_layout(L): changes the call's layout"""
    import torch
    import iac_amd as A
    import gpu_util as G
    import lpcm_util as LP
    layout = layout or G.PAD16
    bps_in = FORMS[form][0]
    Sx, m, _ = ints.shape
    fmt = getattr(A, BD_FMT[bd])
    bps = {16: 2, 24: 3, 32: 4, -32: 4}[bd]
    sc = (batch_kw or {}).get("pcm_stride_channels", 0) or oc
    st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
    s0, cnt = rng or (0, Sx)
    b = A.Batch(Sx, amx, oc, frame_size=fs, out_format=fmt, projection=A.PROJ_EXACT, limiter=limiter, sample_rate=rate, **(batch_kw or {}))
    recs, pos = [], 0
    try:
        b.set_gains(element=[eg[s % len(eg)] for s in range(Sx)], output=[og[s % len(og)] for s in range(Sx)])
        if second is not None:
            b.set_second_element(second, [1.0] * Sx)
        sb = b.stream_state_bytes()

        def exported():
            if not export:
                return None
            d_state = torch.zeros((Sx, sb), dtype=torch.uint8, device="cuda")
            tickets = b.export_range(0, Sx, d_state.data_ptr(), sb, st)
            torch.cuda.synchronize()
            return d_state.cpu().numpy(), [(t.bytes, t.cursor[0], t.cursor[1]) for t in tickets]

        for k, step in enumerate(steps):
            _reset(A)
            if step[0] in ("reset", "do"):
                if step[0] == "reset":
                    b.reset()
                    pos = 0
                else:
                    step[2](b, st)
                torch.cuda.synchronize()
                recs.append(dict(step=step, ret=0, pcm=[np.zeros(0, np.uint8)] * Sx, state=exported(), fam={}, base={}, rest={}, err=None))
                continue
            keep, after, err = [], None, None
            if step[0] == "flush":
                rows, d_pcm, stride = G.pcm_rows(Sx, 240 * sc * bps, layout, bps)
                ret = b.flush_range(d_pcm, stride, st, s0, cnt)
            else:
                nf, n = step[1], samples(fs, step[1:3])
                first = step[3] if len(step) > 3 else 0
                rows, d_pcm, stride = G.pcm_rows(Sx, max(n, 240) * sc * bps, layout, bps)
                a = A.RenderArgs()
                a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, step[2], d_pcm, stride, st
                if step[0] in ("prag", "packets"):
                    raw, L, row = packets_of(form, ints[:, :, pos:pos + n], nf, fs, first, fill, head, pad)
                    if not le:      # the same samples, big-endian
                        widths, perm = layout_of(form, m)
                        dec = np.zeros((Sx, nf, m, fs), dtype=np.int64)
                        play = np.zeros((Sx, m, nf * fs), dtype=np.int64)
                        play[:, :, first:first + n] = ints[:, :, pos:pos + n]
                        dec[:, :, perm, :] = play.reshape(Sx, m, nf, fs).transpose(0, 2, 1, 3)
                        raw, L, row = LP.rows(dec, bps_in, False, widths, perm, head=head, pad=pad, frame_size=fs)
                    if edit_layout:
                        edit_layout(L)
                    inp = A.LpcmInput()
                    if packets is None:
                        d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
                        keep.append(d_raw)
                        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = d_raw.data_ptr(), nf * row, row
                    else:
                        pl = G.place_packets(raw, L, packets, 0, nf)
                        keep.append(pl.keep)
                        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = pl.d_raw, pl.stream_stride, pl.frame_stride
                    inp.first_sample, inp.layout = first, L
                    after = before_call(k, st) if before_call else None
                    try:
                        ret = b.render_packets_ragged(inp, a, s0, cnt) if step[0] == "prag" else b.render_packets(inp, a, s0, cnt)
                    except A.IamfHipError as e:
                        ret, err = 0, e.code
                else:
                    x = as_f32(ints[:, :, pos:pos + n], bps_in)
                    t, d_in, sst, fst = RU.place(x, nf, fs, layout, np.nan)
                    keep.append(t)
                    a.d_in, a.in_stream_stride, a.in_frame_stride = d_in, sst, fst
                    after = before_call(k, st) if before_call else None
                    ret = b.render_ragged(a, s0, cnt) if step[0] == "rag" else b.render_range(a, s0, cnt)
                if err is None:
                    pos += n
            note = after() if after else None
            torch.cuda.synchronize()
            pcm = G.rows_and_rest(rows, layout, ret * sc * bps, only=(s0, cnt))
            fam, base, rest = _tallies(A)
            recs.append(dict(step=step, ret=ret, pcm=pcm, state=exported(), fam=fam, base=base, rest=rest, note=note, err=err))
    finally:
        b.close()
    return recs


stream_pcm = IU.stream_pcm


def assert_same(got, ref, what=""):
    IU.assert_same(got, ref, what)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["err"] == r["err"], (what, "step %d: the error code" % k, g["err"], r["err"])


def no_packet_rows(*tables):
    return not [k for t in tables for k in t if k[0] in PACKET_FED]


def assert_tallies(recs, form, m, oc, routes, what="", is_twin=False):
    """routes, per step: PRAG (the instance's row once, nothing else anywhere), WHOLE_ROW (the form's whole-block row once,
    nothing else), "GENERIC" / "FAST" / "RAG" / a key of the base tally (that row once, the family's tally empty, no packet row
    anywhere), None (nothing launched).  is_twin: PRAG reads "GENERIC" (the unpacker has no row)."""
    for k, (r, f) in enumerate(zip(recs, routes)):
        ctx = (what, "step %d" % k, r["fam"], r["base"], r["rest"])
        if is_twin and f == PRAG:
            f = "GENERIC"
        if f is None or r["step"][0] in ("reset", "do"):
            assert r["fam"] == {} and r["base"] == {} and r["rest"] == {}, ctx
        elif f == PRAG:
            assert r["step"][0] == "prag" and r["fam"] == {inst(form, m, oc): 1} and r["base"] == {} and r["rest"] == {}, ctx
        elif f == WHOLE_ROW:
            merged = dict(r["base"])
            merged.update(r["rest"])
            assert r["fam"] == {} and merged == {whole(form, m, oc): 1}, ctx
        else:
            key = {"FAST": fast(m, oc), "GENERIC": gen(m), "RAG": rag(m, oc)}.get(f, f)
            merged = dict(r["base"])
            merged.update(r["rest"])
            assert r["fam"] == {} and merged == {key: 1}, ctx + (key,)


def check(form, m, oc, fs, ints, calls, bd=16, routes=None, what="", eg=EG, og=OG, oracle=True, flush=True, entries=None, mats=None, **kw):
    """`calls` through the new entry (entries: per call "prag", "packets", "rag" or "range") and a flush; a twin through
    iamf_hip_batch_render_packets, compared after every call; the oracle.  routes: per call what the new entry's batch must
    have run (default_routes); the twin must have run the same, with the general kernel in place of PRAG.
    -> (records, twin's records)"""
    amx, omx = mats or IU.dense_matrices(m, oc)
    entries = entries or ["prag"] * len(calls)
    steps = [(e,) + tuple(c) for e, c in zip(entries, calls)] + ([("flush",)] if flush else [])
    routes = list(routes or default_routes(fs, calls)) + (["GENERIC"] if flush else [])
    got = drive(amx, form, oc, fs, ints, steps, bd=bd, eg=eg, og=og, **kw)
    ref = drive(amx, form, oc, fs, ints, twin(steps), bd=bd, eg=eg, og=og, **kw)
    assert_tallies(got, form, m, oc, routes, what)
    assert_tallies(ref, form, m, oc, routes, what + " (twin)", is_twin=True)
    assert_same(got, ref, what)
    if oracle:
        import test_gpu_programmes as TP
        s0, cnt = kw.get("rng") or (0, ints.shape[0])
        sz = sizes(fs, [c[:2] for c in calls])
        for s in range(s0, s0 + cnt):
            w, _ = want(omx, oc, ints[s], FORMS[form][0], sz, bd, eg[s % len(eg)], og[s % len(og)], flush=flush, rate=kw.get("rate", 48000))
            g = stream_pcm(got, s, oc, bd)
            assert TP.mismatch(g, w) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, w))
    return got, ref


# ---- the decoder façade and the groups ----

# element kinds whose packets the façade hands to the render kernel as they are (lp_worth_asking, iamf_decoder_facade.c):
# mono-coded scene-based elements of 16 or 24 bits, channel-based ones of 16 bits whose pairs are all coupled
FACADE_KINDS = {"zoa": (16, 24), "foa": (16, 24), "soa": (16, 24), "toa": (16, 24), "stereo": (16,), "l51": (16,), "l512": (16,), "l514": (16,),
                "l71": (16,), "l712": (16,), "l714": (16,)}
FACADE_LAYOUTS = (("ss", 0), ("ss", 12))        # stereo, mono
FACADE_VARIANTS = ("default", "wide")


def facade_ragged_frames(c):
    """the frames of a stored fuzz stream (its e2e_fuzz case) that the façade gives the ragged packet form: one element of
    FACADE_KINDS into stereo or mono, little-endian, limiter on, no resampler, no gain ramps, a frame size that is a multiple
    of 4 — and of those frames the ones whose kept samples start at a multiple of 4 and are no whole number of 64-sample blocks"""
    if len(c["pair"]) != 1 or c["pair"][0] not in FACADE_KINDS or c["sample_size"] not in FACADE_KINDS[c["pair"][0]]:
        return []
    if c["layout"] not in FACADE_LAYOUTS or not c.get("limiter", True) or "rate" in c or c.get("big_endian") or c.get("pair_ramps") or c["fs"] % 4:
        return []
    out = []
    for f in range(c["frames"]):
        s0, te = c.get("trims", {}).get(f, (0, 0))
        keep = c["fs"] - s0 - te
        if keep > 0 and s0 % 4 == 0 and keep % 64:
            out.append(f)
    return out


def facade_streams():
    """[(variant, seed, frames)] of the stored fuzz sets (tests/golden/fuzz.json, fuzz_wide.json), selected by configuration"""
    import e2e_fuzz as F
    out = []
    for v in FACADE_VARIANTS:
        for seed in range(F.VARIANTS[v][1]):
            fr = facade_ragged_frames(F.case(seed, v))
            if fr:
                out.append((v, seed, fr))
    return out
