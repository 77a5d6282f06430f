"""Shared pieces of the tests of iamf_hip_batch_render_packets_mix_ragged (tests/test_gpu_zz_packets_mix_ragged.py,
tests/test_packets_mix_ragged_cpu.py): the instances, a two-element presentation whose calls may have any length, the oracle
of a run of such calls and the driver that runs them on one batch.

The programme, the packet rows of both elements and the matrices are route_cases_lpcm_mix.Mix's (one frame of the programme per
frame of a call; a call trimmed to n_samples from first_sample on takes those samples of its frame and leaves the rest of the
frame's runs in the packets, behind and in front of what the call reads).  A call is (n_frames, n_samples[, first_sample]),
n_samples == 0: whole frames.  An entry is "new" (iamf_hip_batch_render_packets_mix_ragged), "twin"
(iamf_hip_batch_render_packets_mix on the same packets), "f32" (iamf_hip_batch_render_range with d_in and d_in2 over the same
whole frames as planar f32) or "flush".  Importing this module needs numpy only."""
import numpy as np

import route_cases as R
import route_cases_lpcm_mix as RM

FAM = "PACKETS_MIX_RAGGED"
FAMILY = 39
WHOLE = {2: "LPCM_MIX", 3: "LPCM24_MIX"}          # the whole-block family of each sample size
OTHER_FAMILIES = ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED", "LPCM24_COUPLED", "LPCM24_MIX", "PACKETS_RAGGED")
PACKET_FED = ("LPCM", "LPCM24", "FANOUT_LPCM") + OTHER_FAMILIES + (FAM,)
# (bytes per sample, m, oc, LP2) as the launchers walk them: the 16-bit units first, the mono-coded beds in front of the coupled
INSTANCES = [(bps, m, oc, k) for bps in (2, 3) for m in RM.LPCM_M + RM.COUPLED_M for oc in RM.MIX_OC for k in RM.MIX_K]
RAG, WHOLE_ROW, GENERIC = "RAG", "WHOLE", "GENERIC"      # what a call must have run
# the two shapes of the length, trim, ramp and switch tests: 3rd order + coupled stereo in 16 bit, 5.1 coupled + mono in 24
SHAPES = {"toa_stereo_16": (2, 16, 2, 2), "l51_mono_24": (3, 6, 2, 1)}


def inst(bps, m, oc, k):
    return (FAM, bps, m, oc, k)


def whole(bps, m, oc, k):
    return (WHOLE[bps], 0, m, oc, k)


def second(m, k):
    """the second element of instance (m, .., k): a coupled stereo pair for k == 2, else mono for odd m, first order for even"""
    return (2, "pair") if k == 2 else ((1 if m & 1 else 4), "mono")


def norm(call):
    return (call[0], call[1], call[2] if len(call) > 2 else 0)


def samples(fs, call):
    nf, n, _ = norm(call)
    return n if n else nf * fs


class Mix(RM.Mix):
    """route_cases_lpcm_mix.Mix over calls of any length.  calls: [(n_frames, n_samples[, first_sample])]; bps: both elements'
    sample bytes; m2 / form2 default to second(m, k)"""

    def __init__(self, bps, m, oc, k, calls, fs, S=3, m2=None, **kw):
        d2, form2 = second(m, k)
        self.calls3 = [norm(c) for c in calls]
        self.bps, self.k_inst = bps, k
        RM.Mix.__init__(self, m, oc, m2 or d2, form2, S=S, calls=[c[0] for c in self.calls3], fs=fs, bps0=bps, bps1=bps, **kw)
        self.rag_inst = inst(bps, m, oc, k)
        self.whole_inst = whole(bps, m, oc, k)

    def kept(self):
        """per call the indices of its samples in the programme (frame f of the programme starts at f * fs)"""
        out, f0 = [], 0
        for nf, n, first in self.calls3:
            out.append(f0 * self.fs + first + np.arange(n if n else nf * self.fs))
            f0 += nf
        return out

    def sizes(self):
        return [len(k) for k in self.kept()]

    def pre_limiter(self, s):
        """-> (the mix of stream s in front of the limiter over the calls' samples [oc][n], element 0's and element 1's share)"""
        import oracle_lib as O
        idx = np.concatenate(self.kept())
        x0, x1 = np.ascontiguousarray(self.x0[s][:, idx]), np.ascontiguousarray(self.x1[s][:, idx])
        n, oc = idx.size, self.oc
        y0, y1 = O.render(self.omx, x0, oc), O.render(self.omx2, x1, oc)

        def gain(y, const, which):
            r = self.ramps.get(which)
            if r is not None:
                O.lib().orc_frame_gain_ramp(O.fp(y), oc, n, O.fp(np.ascontiguousarray(r[s][idx])))
            else:
                O.lib().orc_frame_gain_const(O.fp(y), oc, n, const)     # (skips 1.0 and non-positive gains, as the reference)
        gain(y0, self.eg[s], "e0")
        gain(y1, self.eg2[s], "e1")
        z = np.ascontiguousarray((np.zeros_like(y0) + y0) + y1, dtype=np.float32)
        gain(z, self.og[s], "out")
        return z, y0, y1

    def want_any(self, s, bd=16, flush=True):
        """the oracle's PCM of stream s over the calls (and the flush)"""
        import oracle_lib as O
        z, _, _ = self.pre_limiter(s)
        y, _ = O.limiter_run(z, self.sizes(), flush=flush, rate=self.sample_rate, thr_db=self.threshold_db)
        return np.ascontiguousarray(y.T) if bd == -32 else O.pack(y, bd)

    def const_ramp(self, which, values):
        """a ramp row that holds one value per stream: what the decoder façade sends for element 1's gain"""
        n = self.F * self.fs
        self.ramps[which] = np.ascontiguousarray(np.stack([np.full(n, values[s % len(values)], dtype=np.float32) for s in range(self.S)]))
        return self


def default_routes(mix):
    """per call what the new entry must have run: RAG where packets_mix_ragged_shape_ok's length, position and trim rules hold
    (render_route.hpp), the whole-block mix family for whole blocks at such a position, else the general kernel behind the two
    unpackers"""
    out, pos = [], 0
    for nf, n, first in mix.calls3:
        tot = n if n else nf * mix.fs
        pos_ok = pos % 16 == 0 or pos >= 240
        trim_ok = tot >= mix.fs or (first % 4 == 0 and first + ((tot + 3) & ~3) <= mix.fs)
        if not pos_ok or first % 4:
            out.append(GENERIC)
        elif tot % 64 == 0:
            out.append(WHOLE_ROW)
        else:
            out.append(RAG if trim_ok else GENERIC)
        pos += tot
    return out


def reset_tallies(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    for f in OTHER_FAMILIES + (FAM,):
        A.route_family_tally(f, reset=True)


def tallies(A):
    """-> (the family's tally, the base tally, every other row that was launched), all reset"""
    fam, base = A.route_family_tally(FAM, reset=True), A.route_tally()
    other = dict(A.route_tally_ext())
    other.update(A.route_table_tally(2, reset=True))
    for f in OTHER_FAMILIES:
        other.update(A.route_family_tally(f, reset=True))
    A.route_reset()
    A.route_tally_ext(reset=True)
    return fam, base, other


def ramp_rows(mix, which, idx, shift=0, stride_extra=0, min_stride=0):
    """the call's samples `idx` of ramp `which` as the call hands them over -> (host float32 array, float index of row 0,
    stream stride in floats).  Every stream's row holds len(idx) floats; the rows lie stride floats apart with NaN between
    them, and the allocation ENDS with the last stream's last float: a read at or behind index total of the last row leaves the
    buffer, one behind any other row multiplies NaN in.  shift: floats the rows start behind the allocation's (aligned) start;
    stride_extra: floats added to a stride that is otherwise a multiple of 4; min_stride: n_frames * frame_size, below which
    the entries refuse a stride (a multiple of 4)"""
    total, S = len(idx), mix.S
    stride = max(((total + 3) & ~3) + 4, min_stride) + stride_extra
    host = np.full(shift + (S - 1) * stride + total, np.nan, dtype=np.float32)
    for s in range(S):
        host[shift + s * stride:shift + s * stride + total] = mix.ramps[which][s][idx]
    return host, shift, stride


def render(mix, entries=None, fmt=None, limiter=True, flush=True, ramp_shift=None, ramp_stride_extra=0, between=None):
    """Runs mix.calls3 on one batch.  entries: per call "new" (default), "twin" or "f32".  ramp_shift: {which: floats};
    between: {k: fn(batch, stream)} run in front of call k.
    -> [one record per call, and the flush's]: dict(ret, pcm=[per stream uint8], state=[S][bytes] exported behind the step,
    fam, base, other — the step's tallies)"""
    import torch
    import iac_amd as A
    import gpu_util as G
    S, fs, oc, F = mix.S, mix.fs, mix.oc, mix.F
    fmt = A.FMT_S16 if fmt is None else fmt
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    st = torch.cuda.current_stream().cuda_stream
    entries = list(entries or ["new"] * len(mix.calls3))
    d0, d1 = torch.from_numpy(mix.raw0).cuda(), torch.from_numpy(mix.raw1).cuda()
    places = [(d0.data_ptr(), mix.row0), (d1.data_ptr(), mix.row1)]
    d_x0 = d_x1 = None
    if "f32" in entries:     # [S][F][ch][fs] planar f32 copies of both elements

        def frames(x, ch):
            return torch.from_numpy(np.ascontiguousarray(x.reshape(S, ch, F, fs).transpose(0, 2, 1, 3))).cuda()
        d_x0, d_x1 = frames(mix.x0, mix.m), frames(mix.x1, mix.m2)
    b = A.Batch(S, mix.mx, oc, frame_size=fs, out_format=fmt, limiter=limiter, projection=A.PROJ_EXACT,
                sample_rate=mix.sample_rate, threshold_db=mix.threshold_db)
    recs = []
    try:
        b.set_gains(element=mix.eg, output=mix.og)
        b.set_second_element(mix.mx2, mix.eg2)
        sb = b.stream_state_bytes()

        def export():
            d_state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
            b.export_range(0, S, d_state.data_ptr(), sb, st)
            torch.cuda.synchronize()
            return d_state.cpu().numpy()

        def record(rows, ret):
            torch.cuda.synchronize()
            pcm = G.rows_and_rest(rows, G.PAD16, ret * oc * bps)     # (every byte outside the emitted runs: 0xA5)
            fam, base, other = tallies(A)
            recs.append(dict(ret=ret, pcm=pcm, state=export(), fam=fam, base=base, other=other))

        f0 = 0
        for k, ((nf, n, first), idx, entry) in enumerate(zip(mix.calls3, mix.kept(), entries)):
            if between and k in between:
                between[k](b, st)
                torch.cuda.synchronize()
            reset_tallies(A)
            total = len(idx)
            rows, d_pcm, stride = G.pcm_rows(S, max(total, 240) * oc * bps, G.PAD16, bps)
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n, d_pcm, stride, st
            keep = []
            for which, field in (("e0", "d_element_ramp"), ("e1", "d_element2_ramp"), ("out", "d_output_ramp")):
                if which in mix.ramps:
                    host, off, rstride = ramp_rows(mix, which, idx, (ramp_shift or {}).get(which, 0), ramp_stride_extra, nf * fs)
                    t = torch.from_numpy(host).cuda()
                    keep.append(t)
                    setattr(a, field, t.data_ptr() + 4 * off)
                    a.ramp_stream_stride = rstride
            if entry == "f32":
                assert n == 0 and first == 0
                a.d_in, a.in_stream_stride, a.in_frame_stride = d_x0.data_ptr() + 4 * f0 * mix.m * fs, F * mix.m * fs, mix.m * fs
                a.d_in2, a.in2_stream_stride, a.in2_frame_stride = d_x1.data_ptr() + 4 * f0 * mix.m2 * fs, F * mix.m2 * fs, mix.m2 * fs
                ret = b.render_range(a, 0, S)
            else:
                ins = []
                for (ptr, row), L in zip(places, (mix.L0, mix.L1)):
                    inp = A.LpcmInput()
                    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = ptr + f0 * row, F * row, row
                    inp.first_sample, inp.layout = first, L
                    ins.append(inp)
                ret = (b.render_packets_mix_ragged if entry == "new" else b.render_packets_mix)(ins[0], ins[1], a, 0, S)
            record(rows, ret)
            del keep
            f0 += nf
        if flush and limiter:
            reset_tallies(A)
            rows, d_pcm, stride = G.pcm_rows(S, 240 * oc * bps, G.PAD16, bps)
            record(rows, b.flush_range(d_pcm, stride, st, 0, S))
    finally:
        b.close()
    return recs


def stream_pcm(recs, s):
    parts = [r["pcm"][s] for r in recs]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def assert_tallies(mix, recs, routes, what="", is_twin=False, entries=None):
    """per call: RAG — the instance's row once in the family's tally and nothing else anywhere (the twin: the general kernel's
    row in its place); WHOLE_ROW — the whole-block mix family's row once, nothing else; GENERIC — the general kernel's row
    once, no packet-fed row anywhere; a dict — that base tally.  The flush, if any: the general kernel"""
    entries = entries or ["new"] * len(mix.calls3)
    routes = list(routes) + [GENERIC] * (len(recs) - len(routes))
    for k, (r, f) in enumerate(zip(recs, routes)):
        ctx = (what, "step %d" % k, f, r["fam"], r["base"], r["other"])
        if is_twin and f == RAG:
            f = GENERIC
        if f == RAG:
            assert r["fam"] == {mix.rag_inst: 1} and r["base"] == {} and r["other"] == {}, ctx
        elif f == WHOLE_ROW:
            assert r["fam"] == {} and r["base"] == {} and r["other"] == {mix.whole_inst: 1}, ctx
        elif f == GENERIC:
            assert r["fam"] == {} and r["base"] == {R.gen(mix.m): 1} and r["other"] == {}, ctx
        else:
            assert r["fam"] == {} and r["base"] == f and r["other"] == {}, ctx


def assert_same(got, ref, what=""):
    """return values, PCM bytes and the exported stream state, step by step"""
    assert len(got) == len(ref), what
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["ret"] == r["ret"], (what, "step %d: the value returned" % k, g["ret"], r["ret"])
        for s, (a, b) in enumerate(zip(g["pcm"], r["pcm"])):
            assert np.array_equal(a, b), (what, "step %d, stream %d: PCM" % k, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))
        assert np.array_equal(g["state"], r["state"]), (what, "step %d: the exported stream state" % k)


def check(mix, routes=None, what="", bd=16, oracle=True, entries=None, twin_entries=None, **kw):
    """mix.calls3 through the new entry and a flush; a twin batch through iamf_hip_batch_render_packets_mix, compared after
    every call (return value, PCM, exported state); the tallies of both; the oracle, stream by stream.
    -> (records, twin's records)"""
    import iac_amd as A
    import test_gpu_programmes as TP
    fmt = getattr(A, RM.BD_FMT[bd])
    entries = list(entries or ["new"] * len(mix.calls3))
    twin_entries = twin_entries or ["twin" if e == "new" else e for e in entries]
    routes = routes or default_routes(mix)
    got = render(mix, entries, fmt=fmt, **kw)
    ref = render(mix, twin_entries, fmt=fmt, **kw)
    assert_tallies(mix, got, routes, what)
    assert_tallies(mix, ref, routes, what + " (twin)", is_twin=True)
    assert_same(got, ref, what)
    if oracle:
        for s in range(mix.S):
            w = mix.want_any(s, bd)
            g = RM.view(stream_pcm(got, s), mix.oc, fmt)
            assert TP.mismatch(g, w) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, w))
    return got, ref


def lim_states(state):
    """[S][4]: LimState {g, gs, ge, n} of every exported stream (the blob's first row), n as an integer"""
    f = np.ascontiguousarray(state[:, :16]).view(np.float32).reshape(-1, 4)
    n = np.ascontiguousarray(state[:, 12:16]).view(np.int32).reshape(-1)
    return f, n


# ---- the limiter cases: integer-grid input through selection matrices of weight 2, one peak that engages the limiter ----

LIM_FS = 1000
LIM_LEVEL = 0.6          # x weight 2 = 1.2: above the threshold (-1 dB = 0.891)
# name: (calls, the peak's sample index in the programme).  All on one batch: the ragged calls, then a whole-block mix call, an
# f32 call with d_in2 and the flush (test_gpu_zz_packets_mix_ragged.py adds the entries)
LIM_CASES = {
    # 1000 = 15 * 64 + 40: the last partial block holds samples 960 .. 999 of a call.  A peak on input p triggers at step p + 1
    "trigger_in_the_last_partial_block": ([(1, 0), (1, 0), (1, 0)], 1000 + 975),
    "peak_on_the_last_real_sample": ([(1, 0), (1, 0), (1, 0)], 1000 + 999),
    "release_across_the_next_call": ([(1, 0), (1, 0), (1, 0)], 1000 + 500),
}
LIM_TAIL = [(1, 0), (1, 64 * 15), (1, 0)]      # a ragged call, a whole-block mix call (960 samples), a call for the f32 entry


def lim_mix(name, bps=2, m=4, oc=2, k=2, S=3):
    """the presentation of a limiter case: quiet noise on the integer grid, one peak of LIM_LEVEL on every channel of element 0
    (stream s: one sample earlier per stream, so that the streams differ), selection matrices of weight 2"""
    import lpcm_util as LP
    import test_gpu_programmes as TP
    calls, peak = LIM_CASES[name]
    calls = list(calls) + LIM_TAIL
    F = sum(c[0] for c in calls)
    m2, _ = second(m, k)
    rng = np.random.default_rng(4242)
    i0 = LP.ints(rng, S, F, m, LIM_FS, bps, level=0.02)
    i1 = LP.ints(rng, S, F, m2, LIM_FS, bps, level=0.02)
    full = 1 << (8 * bps - 1)
    for s in range(S):
        p = peak - s
        i0[s, p // LIM_FS, :, p % LIM_FS] = int(LIM_LEVEL * full)
    mats = (TP.selection(m, oc, weight=2.0), TP.selection(m2, oc, weight=2.0))
    mix = Mix(bps, m, oc, k, calls, LIM_FS, S=S, ints=(i0, i1), mats=mats, eg=[1.0] * S, eg2=[1.0] * S, og=[1.0] * S)
    mix.peak = peak
    return mix


# ---- the decoder façade and the groups ----

# element kinds whose packets the façade hands to the two-element forms as they are (lp_worth_asking, iamf_decoder_facade.c).
# The bed: a mono-coded scene-based element, or a channel-based one of a single layer that couples every pair of its layout
# and has no demixing information (M of the render kernel); the second element: mono, a mono-coded scene-based element of 1 or
# 4 channels, or one coupled stereo sub-stream -> (channels, LP2)
FACADE_BEDS = {"zoa": 1, "foa": 4, "soa": 9, "toa": 16, "mono": 1, "stereo": 2, "l51": 6, "l512": 8, "l71": 8, "l514": 10, "l712": 10, "l714": 12}
FACADE_SECONDS = {"mono": (1, 1), "zoa": (1, 1), "foa": (4, 1), "stereo": (2, 2)}
FACADE_SCENE = ("zoa", "foa", "soa", "toa")
FACADE_LAYOUTS = {("ss", 0): 2, ("ss", 12): 1}        # stereo, mono: layouts without an LFE slot (no LFE generator in the batch)
FACADE_VARIANTS = ("default", "lfe")                  # (the lfe set is decoded with its own switch: the HOA LFE generator compiled in)
MIX_FAMILIES = (FAM, "LPCM_MIX", "LPCM24_MIX")


def facade_mix_frames(c, variant="default"):
    """the frames of a stored fuzz stream (its e2e_fuzz case) that the façade gives the two-element packet forms, by kind:
    -> None, or dict(inst=(bps, m, oc, k), ragged=[frames], whole=[frames], f32=[frames]).  Two elements of the kinds above in
    16 or 24 bit into stereo or mono, little-endian, limiter on, no resampler, a frame size that is a multiple of 4; with the
    LFE generator compiled in, a scene-based second element gets a batch of its own (order_elements) and the stream is none of
    these.  A frame whose kept samples start off a multiple of 4 takes the f32 path; of the others, whole 64-sample blocks take
    the whole-block mix family and every other length the ragged one, where the stream stands at a multiple of 16 or past 240"""
    if len(c["pair"]) != 2 or c["pair"][0] not in FACADE_BEDS or c["pair"][1] not in FACADE_SECONDS or c["sample_size"] not in (16, 24):
        return None
    if c["layout"] not in FACADE_LAYOUTS or not c.get("limiter", True) or "rate" in c or "out_rate" in c or c.get("big_endian") or c["fs"] % 4:
        return None
    if variant == "lfe" and c["pair"][1] in FACADE_SCENE:
        return None
    m2, k = FACADE_SECONDS[c["pair"][1]]
    out = dict(inst=(c["sample_size"] // 8, FACADE_BEDS[c["pair"][0]], FACADE_LAYOUTS[c["layout"]], k), ragged=[], whole=[], f32=[])
    pos = 0
    for f in range(c["frames"]):
        s0, te = c.get("trims", {}).get(f, (0, 0))
        keep = c["fs"] - s0 - te
        if keep <= 0:
            continue
        pos_ok = pos % 16 == 0 or pos >= 240
        out["f32" if (s0 % 4 or not pos_ok) else ("ragged" if keep % 64 else "whole")].append(f)
        pos += keep
    return out


def facade_mix_streams():
    """[(variant, seed, frames dict)] of the stored fuzz sets, selected by configuration: every stream with at least one frame
    for a two-element packet form"""
    import e2e_fuzz as F
    out = []
    for v in FACADE_VARIANTS:
        for seed in range(F.VARIANTS[v][1]):
            fr = facade_mix_frames(F.case(seed, v), v)
            if fr and (fr["ragged"] or fr["whole"]):
                out.append((v, seed, fr))
    return out
