"""Shared pieces of the tests of iamf_hip_batch_render_packets_nolim (tests/test_gpu_zz_nolim_packets.py,
tests/test_nolim_packets_cpu.py, tests/test_gpu_zz_nolim_packets_facade.py): the family's instances, the oracle of a limiter-less
stream on the packets' integer grid, the driver that runs a list of calls on one batch, and the selection of stored fuzz streams.

A call is (n_frames, n_samples[, first_sample]); n_samples == 0: whole frames.  drive() renders the calls through the new
entry ("nolim") or through iamf_hip_batch_render_packets_ragged ("ragged", the twin) and returns one record per call: the
value returned (or the refusal's code), every stream's emitted bytes (every other byte of the PCM rows asserted 0xA5:
gpu_util.rows_and_rest), the exported stream state behind the call and the tallies of the call.  The programme, the packets
and the placements are packets_ragged_util's.  Importing this module needs numpy only."""
import numpy as np

import interleaved_util as IU
import packets_ragged_util as PU

FAM = "NOLIM_PACKETS"
FAMILY = 43
FORMS = PU.FORMS
# (form, m) in the listing's order: the 16-bit unit first, mono-coded before coupled
INSTANCES = [(form, m) for form in ("s16", "s16c", "s24", "s24c") for m in (PU.COUPLED_M if FORMS[form][1] else PU.MONO_M)]
S = 3
# per stream: unity, a plain gain, and the two branches a non-positive gain skips (element gain 0, output gain -1)
EG, OG, LG = [1.0, 0.8, 0.0], [1.0, 0.8, -1.0], [1.0, 0.7, 1.3]
OTHER_FAMILIES = PU.OTHER_FAMILIES + (PU.FAM, "PACKETS_MIX_RAGGED")
BD_FMT = IU.BD_FMT
BPS = {16: 2, 24: 3, 32: 4, -32: 4}


def inst(form, m):
    return (FAM, 0, m, 0, FORMS[form][0])


def nolim_f32(m):
    return ("NOLIM", 0, m, 0, 0)


def want(omx, oc, ints, bps_in, bd=-32, eg=1.0, og=1.0, lg=None):
    """the oracle of one limiter-less stream, ints [m][total] in playback order: O.stream_run(.., limiter_on=0) for the integer
    formats; for f32 PCM, which orc_stream does not pack, its stages one by one (render, element gain, 0 + y, output gain,
    loudness gain) -> PCM [total][oc] (s24: [total][oc][3])"""
    import oracle_lib as O
    x = np.ascontiguousarray(PU.as_f32(ints, bps_in))
    if bd != -32:
        return O.stream_run(omx, oc, x, 1024, flush=False, element_gain=float(eg), output_gain=float(og), loudness_on=0 if lg is None else 1,
                            loudness_gain=1.0 if lg is None else float(lg), limiter_on=0, bit_depth=bd)
    y = np.ascontiguousarray(O.render(omx, x, oc), dtype=np.float32)
    n = y.shape[1]
    O.lib().orc_frame_gain_const(O.fp(y), oc, n, float(eg))      # (skips 1.0 and non-positive gains, as the reference)
    z = np.ascontiguousarray(np.zeros_like(y) + y, dtype=np.float32)
    O.lib().orc_frame_gain_const(O.fp(z), oc, n, float(og))
    if lg is not None and np.float32(lg) != np.float32(1.0):
        z = (z * np.float32(lg)).astype(np.float32)
    return np.ascontiguousarray(z.T)


def _reset(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    for f in (FAM,) + OTHER_FAMILIES:
        A.route_family_tally(f, reset=True)


def _tallies(A):
    """-> (the family's tally, table 0, every other table and family as one dict), all reset"""
    fam, base = A.route_family_tally(FAM, reset=True), A.route_tally()
    rest = dict(A.route_tally_ext())
    rest.update(A.route_table_tally(2, reset=True))
    for f in OTHER_FAMILIES:
        rest.update(A.route_family_tally(f, reset=True))
    A.route_reset()
    A.route_tally_ext(reset=True)
    return fam, base, rest


def drive(entry, amx, form, oc, fs, ints, calls, bd=-32, eg=EG, og=OG, lg=None, limiter=False, fill=0, rng=None, second=None, packets=None,
          le=True, edit_layout=None, out_stream=None, before_call=None, export=True, raw_call=None):
    """ints [S][m][total] in playback order; entry: "nolim" or "ragged".  lg: per-stream loudness gains (None: loudness off);
    packets: a packet layout of gpu_util (place_packets; None: the rows as they are, dense); rng: (s0, cnt) — every call over that
    range only; second: a matrix — a second element on the batch; le False: the packets big-endian; edit_layout(L): changes the
    call's layout; raw_call(call): changes the PacketCall and goes through the C entry itself (the refusals)"""
    import ctypes as C
    import torch
    import iac_amd as A
    import gpu_util as G
    import lpcm_util as LP
    layout = G.PAD16
    bps_in, bps = FORMS[form][0], BPS[bd]
    Sx, m, _ = ints.shape
    st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
    s0, cnt = rng or (0, Sx)
    b = A.Batch(Sx, amx, oc, frame_size=fs, out_format=getattr(A, BD_FMT[bd]), projection=A.PROJ_EXACT, limiter=limiter, loudness=lg is not None)
    recs, pos = [], 0
    try:
        b.set_gains(element=[eg[s % len(eg)] for s in range(Sx)], output=[og[s % len(og)] for s in range(Sx)],
                    loudness=None if lg is None else [lg[s % len(lg)] for s in range(Sx)])
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

        for k, c in enumerate(calls):
            _reset(A)
            nf, n = c[0], PU.samples(fs, c[:2])
            first = c[2] if len(c) > 2 else 0
            rows, d_pcm, stride = G.pcm_rows(Sx, max(n, 240) * oc * bps, layout, bps)
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, c[1], d_pcm, stride, st
            raw, L, row = PU.packets_of(form, ints[:, :, pos:pos + n], nf, fs, first, fill)
            if not le:      # the same samples, big-endian
                widths, perm = PU.layout_of(form, m)
                dec = np.zeros((Sx, nf, m, fs), dtype=np.int64)
                play = np.zeros((Sx, m, nf * fs), dtype=np.int64)
                play[:, :, first:first + n] = ints[:, :, pos:pos + n]
                dec[:, :, perm, :] = play.reshape(Sx, m, nf, fs).transpose(0, 2, 1, 3)
                raw, L, row = LP.rows(dec, bps_in, False, widths, perm, head=16, pad=0, frame_size=fs)
            if edit_layout:
                edit_layout(L)
            inp = A.LpcmInput()
            if packets is None:
                d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
                keep = d_raw
                inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = d_raw.data_ptr(), nf * row, row
            else:
                pl = G.place_packets(raw, L, packets, 0, nf)
                keep = pl.keep
                inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = pl.d_raw, pl.stream_stride, pl.frame_stride
            inp.first_sample, inp.layout = first, L
            after = before_call(k, st) if before_call else None
            err = None
            if raw_call is not None:
                call = A.PacketCall()
                call.in_, call.args = inp, a
                fn = A.lib().iamf_hip_batch_render_packets_nolim if entry == "nolim" else A.lib().iamf_hip_batch_render_packets_ragged
                arg = raw_call(call)       # (None: a NULL call)
                ret = fn(b.h, None if arg is None else C.byref(arg), s0, cnt)
                if ret < 0:
                    ret, err = 0, ret
            else:
                try:
                    ret = (b.render_packets_nolim if entry == "nolim" else b.render_packets_ragged)(inp, a, s0, cnt)
                except A.IamfHipError as e:
                    ret, err = 0, e.code
            if err is None:
                pos += n
            note = after() if after else None
            torch.cuda.synchronize()
            del keep
            pcm = G.rows_and_rest(rows, layout, ret * oc * bps, only=(s0, cnt))
            fam, base, rest = _tallies(A)
            recs.append(dict(call=c, ret=ret, pcm=pcm, state=exported(), fam=fam, base=base, rest=rest, note=note, err=err))
    finally:
        b.close()
    return recs


def assert_same(got, ref, what=""):
    """call by call: the value returned, the refusal's code, every stream's bytes and the exported state (blob and tickets)"""
    IU.assert_same(got, ref, what)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["err"] == r["err"], (what, "call %d: the error code" % k, g["err"], r["err"])


def stream_pcm(recs, s, oc, bd):
    return IU.stream_pcm(recs, s, oc, bd)


def check(form, m, oc, fs, ints, calls, bd=-32, fused=True, what="", eg=EG, og=OG, lg=None, oracle=True, mats=None, **kw):
    """`calls` through the new entry and through iamf_hip_batch_render_packets_ragged on a twin, compared call by call.
    fused: every call ran the family's instance once and nothing else, anywhere; the twin never ran the family.  Not fused: the
    family's tally empty and the same rows in every other table as the twin.  Then every stream against the oracle.
    -> (records, twin's records)"""
    amx, omx = mats or IU.dense_matrices(m, oc)
    got = drive("nolim", amx, form, oc, fs, ints, calls, bd=bd, eg=eg, og=og, lg=lg, **kw)
    ref = drive("ragged", amx, form, oc, fs, ints, calls, bd=bd, eg=eg, og=og, lg=lg, **kw)
    for k, (g, r) in enumerate(zip(got, ref)):
        ctx = (what, "call %d" % k, g["fam"], g["base"], g["rest"], r["base"], r["rest"])
        assert r["fam"] == {}, ctx
        if fused:
            assert g["fam"] == {inst(form, m): 1} and g["base"] == {} and g["rest"] == {}, ctx
        else:
            assert g["fam"] == {} and g["base"] == r["base"] and g["rest"] == r["rest"], ctx
    assert_same(got, ref, what)
    if oracle and kw.get("limiter", False) is False and kw.get("second") is None:
        import test_gpu_programmes as TP
        s0, cnt = kw.get("rng") or (0, ints.shape[0])
        total = sum(PU.samples(fs, c[:2]) for c in calls)
        for s in range(s0, s0 + cnt):
            w = want(omx, oc, ints[s][:, :total], FORMS[form][0], bd, eg[s % len(eg)], og[s % len(og)], None if lg is None else lg[s % len(lg)])
            g = stream_pcm(got, s, oc, bd)
            assert TP.mismatch(g, w) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, w))
    return got, ref


# ---- the decoder façade and the groups ----

FACADE_KINDS = PU.FACADE_KINDS
FACADE_VARIANTS = PU.FACADE_VARIANTS


def facade_case_selected(c):
    """a stored fuzz stream (its e2e_fuzz case) whose first stage the façade may give the packet-fed limiter-less renderer: one
    element of FACADE_KINDS' kinds, 16 or 24 bit, little-endian, no gain ramps, a frame size that is a multiple of 4 — and either
    a resampler behind it (rate != output rate) or the limiter off"""
    if len(c["pair"]) != 1 or c["pair"][0] not in FACADE_KINDS or c["sample_size"] not in (16, 24):
        return False
    if c.get("big_endian") or c.get("pair_ramps") or c["fs"] % 4:
        return False
    return c.get("rate", 48000) != (c.get("out_rate") or 48000) or not c.get("limiter", True)


def facade_first_stage_fits(c):
    """whether the first stage's batch of a selected stream is one the kernel takes at all, by the entry's own rule on the PCM
    sample-frame — whole dwords that fit the tile: out_channels * bytes a multiple of 4 and at most 60, f32 into the resampler,
    else the handle's bit depth.  (Sound system E has 11 channels: 22 bytes of s16; H has 24; stereo s24 is 6 bytes.)  A stream
    it rejects stays selected — its PCM hash and the f32 path's bytes are checked — with an empty tally"""
    import e2e_model as M
    oc = M.SS_CH[c["layout"][1]] if c["layout"][0] == "ss" else 2      # (binaural: two channels through a matrix)
    resamples = c.get("rate", 48000) != (c.get("out_rate") or 48000)
    width = oc * (4 if resamples else c["bit_depth"] // 8)
    return width % 4 == 0 and width <= 60


def facade_fused_frames(c):
    """of a selected stream's frames those the first stage renders in one pass of the new kernel: kept samples that start at a
    multiple of 4 and number a positive multiple of 4 (none where facade_first_stage_fits says no)"""
    out = []
    if not facade_first_stage_fits(c):
        return out
    for f in range(c["frames"]):
        s0, te = c.get("trims", {}).get(f, (0, 0))
        keep = c["fs"] - s0 - te
        if keep > 0 and s0 % 4 == 0 and keep % 4 == 0:
            out.append(f)
    return out


def facade_streams(limiter_off=None):
    """[(variant, seed, fused frames)] of the stored fuzz sets (tests/golden/fuzz.json, fuzz_wide.json), selected by
    configuration.  limiter_off: None — all of them; True / False — those with the limiter off / the resampling ones with it on"""
    import e2e_fuzz as F
    out = []
    for v in FACADE_VARIANTS:
        for seed in range(F.VARIANTS[v][1]):
            c = F.case(seed, v)
            if facade_case_selected(c) and (limiter_off is None or limiter_off == (not c.get("limiter", True))):
                out.append((v, seed, facade_fused_frames(c)))
    return out
