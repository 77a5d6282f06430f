"""Shared pieces of the tests of iamf_hip_batch_render_packets_mix_nolim (tests/test_gpu_zz_nolim_packets_mix.py,
tests/test_nolim_packets_mix_cpu.py, tests/test_gpu_zz_nolim_packets_mix_facade.py): the family's instances, the driver that runs a
two-element presentation's calls through the new entry ("nolim") or through iamf_hip_batch_render_packets_mix_ragged ("ragged", the
twin) on one batch, the oracle of a limiter-less two-element stream, and the selection of stored fuzz streams.

The programme, the packet rows of both elements, pre_limiter() and ramp_rows() are packets_mix_ragged_util.Mix's; the tally
helpers and the placements are nolim_packets_util's and gpu_util's.  A call is (n_frames, n_samples[, first_sample]),
n_samples == 0: whole frames.  drive() returns one record per call: the value returned (or the refusal's code), every stream's
emitted bytes (every other byte of the PCM rows asserted 0xA5: gpu_util.rows_and_rest), the exported stream state behind the
call and the tallies of the call.  Importing this module needs numpy only."""
import numpy as np

import interleaved_util as IU
import nolim_packets_util as NU
import packets_mix_ragged_util as PMU
import route_cases_lpcm_mix as RM

FAM = "NOLIM_PACKETS_MIX"
FAMILY = 47
# (bytes per sample, m, LP2) as the launchers walk them: the 16-bit unit first, the mono-coded beds in front of the coupled
INSTANCES = [(bps, m, k) for bps in (2, 3) for m in RM.LPCM_M + RM.COUPLED_M for k in RM.MIX_K]
S = NU.S
EG, OG, LG = NU.EG, NU.OG, NU.LG          # per stream, as the single-element tests have them
EG2 = [1.0, 0.8, 0.0]                      # element 1: unity, a plain gain, and the branch a non-positive gain skips
OTHER_FAMILIES = NU.OTHER_FAMILIES + (NU.FAM,)
BD_FMT, BPS = NU.BD_FMT, NU.BPS


def inst(bps, m, k):
    return (FAM, bps, m, 0, k)


class Mix(PMU.Mix):
    """packets_mix_ragged_util.Mix with this file's gains; bps1: element 1's sample bytes where they differ from element 0's"""

    def __init__(self, bps, m, oc, k, calls, fs, S=S, bps1=None, **kw):
        kw.setdefault("eg", EG)
        kw.setdefault("og", OG)
        kw.setdefault("eg2", EG2)
        if bps1 is None or bps1 == bps:
            PMU.Mix.__init__(self, bps, m, oc, k, calls, fs, S=S, **kw)
        else:
            d2, form2 = PMU.second(m, k)
            self.calls3 = [PMU.norm(c) for c in calls]
            self.bps, self.k_inst = bps, k
            RM.Mix.__init__(self, m, oc, d2, form2, S=S, calls=[c[0] for c in self.calls3], fs=fs, bps0=bps, bps1=bps1, **kw)
        self.nl_inst = inst(bps, m, k)


def want(mix, s, bd=-32, lg=None):
    """the oracle of stream s over the calls: Mix.pre_limiter (render, the element gains or ramps, 0 + y, + y2, the output gain or
    ramp), the loudness gain, the format's conversion — the reference's stages with the limiter off -> PCM [n][oc] (s24: [n][oc][3])"""
    import oracle_lib as O
    z = mix.pre_limiter(s)[0]
    if lg is not None and np.float32(lg) != np.float32(1.0):
        z = (z * np.float32(lg)).astype(np.float32)
    z = np.ascontiguousarray(z, dtype=np.float32)
    return np.ascontiguousarray(z.T) if bd == -32 else O.pack(z, bd)


def _reset(A):
    NU._reset(A)
    A.route_family_tally(FAM, reset=True)
    A.route_family_tally(NU.FAM, reset=True)


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


def drive(entry, mix, bd=-32, lg=None, limiter=False, rng=None, packets=(None, None), ramp_shift=None, ramp_stride_extra=0,
          out_stream=None, before_call=None, export=True, raw_call=None, second=True):
    """entry: "nolim" or "ragged".  lg: per-stream loudness gains (None: loudness off); rng: (s0, cnt) — every call over that range
    only; packets: a packet layout of gpu_util per element (place_packets; None: the rows as they are, dense); ramp_shift:
    {which: floats}; second False: the batch has no second element; raw_call(call): changes the PacketMixCall and goes through the
    C entry itself (the refusals)"""
    import ctypes as C
    import torch
    import iac_amd as A
    import gpu_util as G
    Sx, fs, oc = mix.S, mix.fs, mix.oc
    bps = BPS[bd]
    st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
    s0, cnt = rng or (0, Sx)
    b = A.Batch(Sx, mix.mx, oc, frame_size=fs, out_format=getattr(A, BD_FMT[bd]), projection=A.PROJ_EXACT, limiter=limiter, loudness=lg is not None)
    recs = []
    try:
        b.set_gains(element=mix.eg, output=mix.og, loudness=None if lg is None else [lg[s % len(lg)] for s in range(Sx)])
        if second:
            b.set_second_element(mix.mx2, mix.eg2)
        sb = b.stream_state_bytes()

        def exported():
            if not export:
                return None
            d_state = torch.zeros((Sx, sb), dtype=torch.uint8, device="cuda")
            tickets = b.export_range(0, Sx, d_state.data_ptr(), sb, st)
            torch.cuda.synchronize()
            return d_state.cpu().numpy(), [(t.bytes, t.cursor[0], t.cursor[1]) for t in tickets]

        f0 = 0
        for k, ((nf, n, first), idx) in enumerate(zip(mix.calls3, mix.kept())):
            _reset(A)
            total = len(idx)
            rows, d_pcm, stride = G.pcm_rows(Sx, max(total, 240) * oc * bps, G.PAD16, bps)
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n, d_pcm, stride, st
            keep = []
            for which, field in (("e0", "d_element_ramp"), ("e1", "d_element2_ramp"), ("out", "d_output_ramp")):
                if which in mix.ramps:
                    host, off, rstride = PMU.ramp_rows(mix, which, idx, (ramp_shift or {}).get(which, 0), ramp_stride_extra, nf * fs)
                    t = torch.from_numpy(host).cuda()
                    keep.append(t)
                    setattr(a, field, t.data_ptr() + 4 * off)
                    a.ramp_stream_stride = rstride
            ins = []
            for raw, row, L, pk in ((mix.raw0, mix.row0, mix.L0, packets[0]), (mix.raw1, mix.row1, mix.L1, packets[1])):
                inp = A.LpcmInput()
                part = np.ascontiguousarray(raw[:, f0:f0 + nf, :])
                if pk is None:
                    d_raw = torch.from_numpy(part).cuda()
                    keep.append(d_raw)
                    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = d_raw.data_ptr(), nf * row, row
                else:
                    pl = G.place_packets(part, L, pk, 0, nf)
                    keep.append(pl.keep)
                    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = pl.d_raw, pl.stream_stride, pl.frame_stride
                inp.first_sample, inp.layout = first, L
                ins.append(inp)
            after = before_call(k, st) if before_call else None
            err = None
            if raw_call is not None:
                call = A.PacketMixCall()
                call.in_[0], call.in_[1], call.args = ins[0], ins[1], a
                fn = A.lib().iamf_hip_batch_render_packets_mix_nolim if entry == "nolim" else A.lib().iamf_hip_batch_render_packets_mix_ragged
                arg = raw_call(call)       # (None: a NULL call)
                ret = fn(b.h, None if arg is None else C.byref(arg), s0, cnt)
                if ret < 0:
                    ret, err = 0, ret
            else:
                try:
                    ret = (b.render_packets_mix_nolim if entry == "nolim" else b.render_packets_mix_ragged)(ins[0], ins[1], a, s0, cnt)
                except A.IamfHipError as e:
                    ret, err = 0, e.code
            note = after() if after else None
            torch.cuda.synchronize()
            del keep
            pcm = G.rows_and_rest(rows, G.PAD16, ret * oc * bps, only=(s0, cnt))
            fam, base, rest = _tallies(A)
            recs.append(dict(call=(nf, n, first), ret=ret, pcm=pcm, state=exported(), fam=fam, base=base, rest=rest, note=note, err=err))
            f0 += nf
    finally:
        b.close()
    return recs


def assert_same(got, ref, what=""):
    """call by call: the value returned, the refusal's code, every stream's bytes and the exported state (blob and tickets)"""
    NU.assert_same(got, ref, what)


def stream_pcm(recs, s, oc, bd):
    return IU.stream_pcm(recs, s, oc, bd)


def check(mix, bd=-32, fused=True, what="", lg=None, oracle=True, **kw):
    """mix.calls3 through the new entry and through iamf_hip_batch_render_packets_mix_ragged on a twin, compared call by call.
    fused: every call ran the family's instance once and nothing else, anywhere (a list: per call); the twin never ran the family.
    Not fused: the family's tally empty and the same rows in every other table as the twin.  Then every stream of the range against
    the oracle (a limiter-off batch with a second element whose calls all ran).  -> (records, twin's records)"""
    got = drive("nolim", mix, bd=bd, lg=lg, **kw)
    ref = drive("ragged", mix, bd=bd, lg=lg, **kw)
    flags = fused if isinstance(fused, (list, tuple)) else [fused] * len(got)
    for k, (g, r, f) in enumerate(zip(got, ref, flags)):
        ctx = (what, "call %d" % k, g["fam"], g["base"], g["rest"], r["base"], r["rest"])
        assert r["fam"] == {}, ctx
        if f:
            assert g["fam"] == {mix.nl_inst: 1} and g["base"] == {} and g["rest"] == {}, ctx
        else:
            assert g["fam"] == {} and g["base"] == r["base"] and g["rest"] == r["rest"], ctx
    assert_same(got, ref, what)
    if oracle and not kw.get("limiter", False) and kw.get("second", True) and all(r["err"] is None for r in got):
        import test_gpu_programmes as TP
        s0, cnt = kw.get("rng") or (0, mix.S)
        for s in range(s0, s0 + cnt):
            w = want(mix, s, bd, None if lg is None else lg[s % len(lg)])
            g = stream_pcm(got, s, mix.oc, bd)
            assert TP.mismatch(g, w) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, w))
    return got, ref


# ---- the decoder façade and the groups ----

FACADE_BEDS = PMU.FACADE_BEDS
FACADE_SECONDS = PMU.FACADE_SECONDS
FACADE_SCENE = PMU.FACADE_SCENE
FACADE_VARIANTS = ("default", "params", "wide")          # (the sets the single-element façade test decodes, and params)
FACADE_GOLD = {"default": "fuzz.json", "params": "fuzz_params.json", "wide": "fuzz_wide.json"}
IL = "FAST_INTERLEAVED"


def facade_case_selected(c, variant="default"):
    """a stored fuzz stream (its e2e_fuzz case) whose first stage the façade may give the two-element form of the limiter-less
    renderer: two elements of FACADE_BEDS x FACADE_SECONDS, 16 or 24 bit, little-endian, a frame size that is a multiple of 4 —
    and either a resampler behind it (rate != output rate) or the limiter off.  With the LFE variant a scene-based second element
    gets a batch of its own and is not selected"""
    if len(c["pair"]) != 2 or c["pair"][0] not in FACADE_BEDS or c["pair"][1] not in FACADE_SECONDS or c["sample_size"] not in (16, 24):
        return False
    if c.get("big_endian") or c["fs"] % 4:
        return False
    if variant == "lfe" and c["pair"][1] in FACADE_SCENE:
        return False
    return c.get("rate", 48000) != (c.get("out_rate") or 48000) or not c.get("limiter", True)


def facade_case(seed, variant):
    """the description stream `seed` of a set is BUILT from (e2e_fuzz.build): the params set's is case_params(seed) — the default
    set's stream of that number with mix-gain parameter timelines on the element and output gains — not case(seed, "params")"""
    import e2e_fuzz as F
    return F.case_params(seed) if variant == "params" else F.case(seed, variant)


def facade_instance(c):
    return inst(c["sample_size"] // 8, FACADE_BEDS[c["pair"][0]], FACADE_SECONDS[c["pair"][1]][1])


def facade_fused_frames(c):
    """of a selected stream's frames those the first stage renders in one pass of the new kernel: kept samples that start at a
    multiple of 4 and number a positive multiple of 4, where the first stage's PCM sample-frame is whole dwords of at most 60 bytes
    (nolim_packets_util.facade_first_stage_fits); none otherwise"""
    return NU.facade_fused_frames(c)


def facade_resamples_into_one_or_two(c):
    """the last stage is one iamf_hip_batch_render_interleaved runs its fast form for: behind a resampler, one or two channels,
    limiter on"""
    return c.get("rate", 48000) != (c.get("out_rate") or 48000) and c["layout"] in (("ss", 0), ("ss", 12), ("binaural",)) and c.get("limiter", True)


def facade_streams():
    """[(variant, seed, fused frames)] of the stored fuzz sets, selected by configuration, each with a PCM hash of the real
    reference in its golden file"""
    import json
    import os
    import e2e_fuzz as F
    out = []
    here = os.path.dirname(os.path.abspath(__file__))
    for v in FACADE_VARIANTS:
        with open(os.path.join(here, "golden", FACADE_GOLD[v])) as f:
            gold = json.load(f)
        for seed in range(F.VARIANTS[v][1]):
            c = facade_case(seed, v)
            if facade_case_selected(c, v) and "sha256" in gold.get(str(seed), {}):
                out.append((v, seed, facade_fused_frames(c)))
    return out
