"""The two-element packet form (iamf_hip_batch_render_lpcm_mix, render_fast_kernel<.., LP2>): one case per kernel instance
of the LPCM_MIX family (iamf_hip_route_family_instances), and the pieces tests/test_gpu_lpcm_mix.py builds its cases from —
the programme, the packet rows of both elements, the loop that renders them through the entry and the oracle.
tests/test_lpcm_mix_cpu.py holds the cases against the library's listing (no GPU).  Importing this module needs neither a
GPU nor the library.

The oracle is composed as route_cases.run_matrix composes it for a second element: oracle_lib.render of each element from
ints / 2^15 (the reference's LPCM decode, pcm/IAMF_pcm_decoder.c:64-83, exact in f32), orc_frame_gain_const or
orc_frame_gain_ramp on each, (0 + y0) + y1, the output gain, oracle_lib.limiter_run, oracle_lib.pack.  Tolerance 0."""
import numpy as np

import route_cases as R
from route_cases import Case

FAM = "LPCM_MIX"
# the lists of render_route.hpp, restated: tests/test_lpcm_mix_cpu.py fails when they drift
LPCM_M = [1, 4, 9, 16]
COUPLED_M = [2, 6, 8, 10, 12]
MIX_OC = [1, 2]
MIX_K = [1, 2]          # the second element's form: 1 mono-coded runs (1 or 4 channels), 2 one coupled stereo pair
PACKET_FED = ("LPCM", "LPCM24", "LPCM_COUPLED", "FANOUT_LPCM", FAM)
BD_FMT = {16: "FMT_S16", 24: "FMT_S24", 32: "FMT_S32", -32: "FMT_F32"}


def inst(m, oc, k):
    return (FAM, 0, m, oc, k)


def elem0_substreams(m, rng):
    """-> (widths, perm) of lpcm_util.rows: a loudspeaker layout's canonical coupling (the pairs, then C and LFE; playback
    order L R C LFE, then the pairs) for the channel counts of COUPLED_M, mono sub-streams in a seeded order otherwise"""
    if m == 2:
        return [2], [0, 1]
    if m in COUPLED_M:
        return [2] * ((m - 2) // 2) + [1, 1], [0, 1, m - 2, m - 1] + list(range(2, m - 2))
    return [1] * m, [int(v) for v in rng.permutation(m)]


def elem1_substreams(m2, form):
    """form: "mono" (one mono sub-stream per channel) or "pair" (one coupled stereo sub-stream)"""
    assert form in ("mono", "pair") and (form == "mono" or m2 == 2)
    return ([2], [0, 1]) if form == "pair" else ([1] * m2, list(range(m2)))


def planar(ints, perm, bps=2):
    S, F, m, fs = ints.shape
    x = (ints[:, :, perm, :].astype(np.float64) / float(1 << (8 * bps - 1))).astype(np.float32)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)


def programme(S, F, fs, m, m2, seed, bps0=2, bps1=2):
    """-> (ints0 [S][F][m][fs], ints1 [S][F][m2][fs]): quiet noise and, on every channel of an element at once, bursts —
    element 0 at 0.946 of full scale every 97 samples from sample 11 of a frame on, element 1 at 0.6 every 131 from 53 on,
    signs alternating.  Through matrices whose columns add up to 1.4 (route_cases.matrices, table=False) element 0 alone
    passes the limiter's threshold; element 1's bursts fall between element 0's."""
    import lpcm_util as LP
    rng = np.random.default_rng(seed)
    i0 = LP.ints(rng, S, F, m, fs, bps0, level=0.05)
    i1 = LP.ints(rng, S, F, m2, fs, bps1, level=0.05)
    for v, lo, step, level, bps in ((i0, 11, 97, 0.946, bps0), (i1, 53, 131, 0.6, bps1)):
        n = v[0, 0, 0, lo::step].size
        v[:, :, :, lo::step] = (int(level * (1 << (8 * bps - 1))) * (-1) ** np.arange(n))[None, None, None, :]
    return i0, i1


class Mix:
    """one two-element presentation: matrices, gains, the programme as ints, packet rows and planar f32"""

    def __init__(self, m, oc, m2, form2="mono", S=3, calls=(1, 3, 2), fs=1024, seed=0, bps0=2, le0=True, bps1=2, le1=True,
                 eg=None, eg2=None, og=None, head=(16, 16), pad=(0, 0), fill=False, two_mono=False, sample_rate=48000,
                 threshold_db=-1.0, ints=None, mats=None):
        """sample_rate, threshold_db: the batch's and the oracle limiter's; ints: (ints0 [S][F][m][fs], ints1 [S][F][m2][fs]) in
        place of programme()'s — such a mix need not drive the limiter through both elements (hot = False); mats: ((product,
        oracle) of element 0, the same of element 1) in place of the seeded dense matrices"""
        import lpcm_util as LP
        import gpu_util as G
        self.m, self.oc, self.m2, self.S, self.fs, self.calls = m, oc, m2, S, fs, list(calls)
        self.sample_rate, self.threshold_db, self.hot = sample_rate, threshold_db, ints is None
        F = self.F = sum(calls)
        (self.mx, self.omx), (self.mx2, self.omx2) = mats or (R.matrices(m, oc, table=False), R.matrices(m2, oc, table=False, salt=1))
        self.eg = list(eg) if eg is not None else [R.EG[s % 3] for s in range(S)]
        self.og = list(og) if og is not None else [R.OG[s % 3] for s in range(S)]
        self.eg2 = list(eg2) if eg2 is not None else [[0.6, 1.0, 0.9][s % 3] for s in range(S)]
        rng = np.random.default_rng(7000 + 64 * m + 8 * m2 + oc + seed)
        i0, i1 = ints or programme(S, F, fs, m, m2, 7100 + 64 * m + 8 * m2 + seed, bps0, bps1)
        w0, p0 = elem0_substreams(m, rng)
        w1, p1 = ([1, 1], [0, 1]) if two_mono else elem1_substreams(m2, form2)
        self.x0, self.x1 = planar(i0, p0, bps0), planar(i1, p1, bps1)
        self.raw0, self.L0, self.row0 = LP.rows(i0, bps0, le0, w0, p0, head=head[0], pad=pad[0], frame_size=fs)
        self.raw1, self.L1, self.row1 = LP.rows(i1, bps1, le1, w1, p1, head=head[1], pad=pad[1], frame_size=fs)
        if fill:   # every byte that belongs to no run: 0x7F / 0x80 alternating (a load that strays reads a large sample)
            for name, L in (("raw0", self.L0), ("raw1", self.L1)):
                raw = getattr(self, name)
                used = G.packet_run_mask(L, raw.shape[-1])
                f = np.where(np.arange(raw.shape[-1]) % 2 == 0, 0x7F, 0x80).astype(np.uint8)
                setattr(self, name, np.where(used[None, None, :], raw, f[None, None, :]))
        self.k = 2 if (form2 == "pair" and not two_mono) else 1
        self.inst = inst(m, oc, self.k)
        self.ramps = {}           # "e0" / "e1" / "out" -> [S][F * fs] f32

    def ramp(self, which, seed):
        """a per-sample gain between 0.9 and 1.2, its own curve per stream"""
        n = self.F * self.fs
        t = np.arange(n, dtype=np.float64)
        r = [1.05 + 0.15 * np.sin(t / (300.0 + 70 * seed + 40 * s) + seed + s) for s in range(self.S)]
        self.ramps[which] = np.ascontiguousarray(np.stack(r), dtype=np.float32)
        return self

    # ---- the oracle ----
    def want(self, s, bd=16, sizes=None, cut=None, limiter=True):
        """-> (PCM of stream s as the oracle packs it, the mix in front of the limiter, element 0's and element 1's share
        of it).  cut: (lo, hi) — the samples of the programme the calls took (a trimmed start); sizes: the calls' lengths"""
        import oracle_lib as O
        lo, hi = cut or (0, self.F * self.fs)
        x0, x1 = np.ascontiguousarray(self.x0[s][:, lo:hi]), np.ascontiguousarray(self.x1[s][:, lo:hi])
        n, oc = hi - lo, self.oc
        y0, y1 = O.render(self.omx, x0, oc), O.render(self.omx2, x1, oc)

        def gain(y, const, which):
            r = self.ramps.get(which)
            if r is not None:
                O.lib().orc_frame_gain_ramp(O.fp(y), oc, n, O.fp(np.ascontiguousarray(r[s][lo:hi])))
            else:
                O.lib().orc_frame_gain_const(O.fp(y), oc, n, const)     # (skips 1.0 and non-positive gains, as the reference)
        gain(y0, self.eg[s], "e0")
        gain(y1, self.eg2[s], "e1")
        z = np.ascontiguousarray((np.zeros_like(y0) + y0) + y1, dtype=np.float32)
        gain(z, self.og[s], "out")
        pre = z.copy()
        if limiter:
            z, _ = O.limiter_run(z, sizes or [self.fs * nf for nf in self.calls], rate=self.sample_rate, thr_db=self.threshold_db)
        pcm = np.ascontiguousarray(z.T) if bd == -32 else O.pack(z, bd)
        return pcm, pre, y0, y1

    def assert_drives_the_limiter(self, s, pre, y0, y1, what=""):
        """from the oracle alone: the mix passes the threshold (-1 dB = 0.891), both elements burst, at different phases"""
        p0, p1 = np.abs(y0).max(axis=0), np.abs(y1).max(axis=0)
        assert float(np.abs(pre).max()) > 0.95, (what, s, "the mix stays under the threshold", float(np.abs(pre).max()))
        assert float(p0.max()) > 0.5 and float(p1.max()) > 0.25, (what, s, "an element has no bursts", float(p0.max()), float(p1.max()))
        assert int(p0.argmax()) % self.fs != int(p1.argmax()) % self.fs, (what, s, "the elements burst in phase")

    # ---- the device side ----
    def render(self, fmt=None, placement="own", first=0, n_samples=0, rng_streams=None, limiter=True, out_stream=None,
               steps=None, before_call=None, prefill_state=False):
        """Renders the calls through iamf_hip_batch_render_lpcm_mix and flushes.  placement: "own" — each element in a buffer
        of its own; "shared" — element 1's runs in the same packet rows as element 0's, behind them.  steps: per call "mix"
        (default) or "f32" (iamf_hip_batch_render_range on f32 copies of the same frames).  rng_streams: (s0, cnt) — every
        call and the flush over that range only.  before_call(k, stream handle) runs in front of call k and may return a
        function to run right behind it.
        -> dict(pcm=[per stream uint8], emitted=[..], state=[S][bytes] exported in front of the flush, notes=[...])"""
        import torch
        import iac_amd as A
        import gpu_util as G
        S, fs, oc, F = self.S, self.fs, self.oc, self.F
        fmt = A.FMT_S16 if fmt is None else fmt
        bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
        st = out_stream if out_stream is not None else torch.cuda.current_stream().cuda_stream
        s0, cnt = rng_streams or (0, S)
        if placement == "shared":
            both = np.concatenate([self.raw0, self.raw1], axis=2)
            d_both = torch.from_numpy(both).cuda()
            row = self.row0 + self.row1
            places = [(d_both.data_ptr(), row), (d_both.data_ptr() + self.row0, row)]
        else:
            d0, d1 = torch.from_numpy(self.raw0).cuda(), torch.from_numpy(self.raw1).cuda()
            places = [(d0.data_ptr(), self.row0), (d1.data_ptr(), self.row1)]
        d_x0 = d_x1 = None
        if steps and "f32" in steps:     # [S][F][ch][fs] planar f32 copies of both elements
            def frames(x, ch):
                return torch.from_numpy(np.ascontiguousarray(x.reshape(S, ch, F, fs).transpose(0, 2, 1, 3))).cuda()
            d_x0, d_x1 = frames(self.x0, self.m), frames(self.x1, self.m2)
        d_ramps = {k: torch.from_numpy(v).cuda() for k, v in self.ramps.items()}
        b = A.Batch(S, self.mx, oc, frame_size=fs, out_format=fmt, limiter=limiter, projection=A.PROJ_EXACT,
                    sample_rate=self.sample_rate, threshold_db=self.threshold_db)
        outs, emitted, notes = [[] for _ in range(S)], [], []
        try:
            b.set_gains(element=self.eg, output=self.og)
            b.set_second_element(self.mx2, self.eg2)
            sb = b.stream_state_bytes()

            def export():
                d_state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
                b.export_range(0, S, d_state.data_ptr(), sb, st)
                torch.cuda.synchronize()
                return d_state.cpu().numpy()

            def take(rows, n):
                torch.cuda.synchronize()
                h = G.rows_and_rest(rows, G.DENSE, n * oc * bps, only=(s0, cnt))   # (every byte outside the emitted runs: 0xA5)
                for s in range(s0, s0 + cnt):
                    outs[s].append(h[s])
                emitted.append(n)

            state0 = export() if prefill_state else None
            f0 = 0
            for k, nf in enumerate(self.calls):
                total = n_samples if n_samples else nf * fs
                rows, d_pcm, stride = G.pcm_rows(S, max(total, 240) * oc * bps, G.DENSE, bps)
                a = A.RenderArgs()
                a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n_samples, d_pcm, stride, st
                for which, field in (("e0", "d_element_ramp"), ("e1", "d_element2_ramp"), ("out", "d_output_ramp")):
                    if which in d_ramps:   # the call's samples of every stream's ramp: stream stride = the whole programme
                        setattr(a, field, d_ramps[which].data_ptr() + 4 * (f0 * fs + first))
                        a.ramp_stream_stride = F * fs
                after = before_call(k, st) if before_call else None
                if steps and steps[k] == "f32":
                    a.d_in, a.in_stream_stride, a.in_frame_stride = d_x0.data_ptr() + 4 * f0 * self.m * fs, F * self.m * fs, self.m * fs
                    a.d_in2, a.in2_stream_stride, a.in2_frame_stride = d_x1.data_ptr() + 4 * f0 * self.m2 * fs, F * self.m2 * fs, self.m2 * fs
                    n = b.render_range(a, s0, cnt)
                else:
                    ins = []
                    for (ptr, row), L in zip(places, (self.L0, self.L1)):
                        inp = A.LpcmInput()
                        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = ptr + f0 * row, F * row, row
                        inp.first_sample, inp.layout = first, L
                        ins.append(inp)
                    n = b.render_lpcm_mix(ins[0], ins[1], a, s0, cnt)
                if after:
                    notes.append(after())
                take(rows, n)
                f0 += nf
            state = export()
            if limiter:
                rows, d_pcm, stride = G.pcm_rows(S, 240 * oc * bps, G.DENSE, bps)
                take(rows, b.flush_range(d_pcm, stride, st, s0, cnt))
        finally:
            b.close()
        pcm = [np.concatenate(o) if o else np.zeros(0, dtype=np.uint8) for o in outs]
        return dict(pcm=pcm, emitted=emitted, state=state, state0=state0, notes=notes, fmt=fmt)


def reset_tallies(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    A.route_family_tally("LPCM_COUPLED", reset=True)
    A.route_family_tally(FAM, reset=True)


def tallies(A):
    """-> (the family's tally, the base tally, every other packet-fed row that was launched), all reset"""
    fam, base = A.route_family_tally(FAM, reset=True), A.route_tally()
    other = dict(A.route_tally_ext())
    other.update(A.route_table_tally(2, reset=True))
    other.update(A.route_family_tally("LPCM_COUPLED", reset=True))
    A.route_reset()
    A.route_tally_ext(reset=True)
    return fam, base, other


def view(raw, oc, fmt):
    import iac_amd as A
    import gpu_util as G
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    return G._view(raw, raw.size // (oc * bps), oc, fmt)


def check(mix, fused, bd=16, what="", unfused_base=None, **kw):
    """Renders `mix` through the entry, and a twin batch through the same entry under IAMF_HIP_LPCM_UNFUSED=1.  fused: the
    family tally names mix.inst once per call and the base tally holds the flush's GENERIC row alone; else the family tally
    is empty and the base tally is unfused_base (default: the f32 mixing variant per call + the flush).  Either way: PCM
    bit for bit the oracle's, and PCM, n_emitted and the exported stream state equal to the twin's."""
    import iac_amd as A
    import test_gpu_programmes as TP
    fmt = getattr(A, BD_FMT[bd])
    n_calls = len(mix.calls)
    reset_tallies(A)
    got = mix.render(fmt=fmt, **kw)
    fam, base, other = tallies(A)
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        twin = mix.render(fmt=fmt, **kw)
        fam_twin, base_twin, other_twin = tallies(A)
    f32 = unfused_base if unfused_base is not None else {("FAST", 1, mix.m, mix.oc, 0): n_calls, R.gen(mix.m): 1}
    if fused:
        assert fam == {mix.inst: n_calls}, (what, "the family's tally", fam)
        assert base == {R.gen(mix.m): 1}, (what, "the base tally: the flush's GENERIC row alone", base)
    else:
        assert fam == {} and base == f32, (what, fam, base)
    assert other == {} and not [k for k in base if k[0] in PACKET_FED or k[0] == "NONE"], (what, other, base)
    assert fam_twin == {} and other_twin == {} and base_twin == f32, (what, fam_twin, other_twin, base_twin)
    assert got["emitted"] == twin["emitted"], (what, got["emitted"], twin["emitted"])
    assert np.array_equal(got["state"], twin["state"]), (what, "the exported stream state against the unfused twin's")
    first, n_samples = kw.get("first", 0), kw.get("n_samples", 0)
    cut, sizes = ((first, first + n_samples), [n_samples]) if n_samples else (None, None)
    s0, cnt = kw.get("rng_streams") or (0, mix.S)
    for s in range(s0, s0 + cnt):
        want, pre, y0, y1 = mix.want(s, bd, sizes=sizes, cut=cut, limiter=kw.get("limiter", True))
        if mix.hot:
            mix.assert_drives_the_limiter(s, pre, y0, y1, what)
        g, t = view(got["pcm"][s], mix.oc, fmt), view(twin["pcm"][s], mix.oc, fmt)
        assert TP.mismatch(g, want) is None, (what, "stream %d against the oracle" % s, TP.mismatch(g, want))
        assert TP.mismatch(g, t) is None, (what, "stream %d against the unfused twin" % s, TP.mismatch(g, t))
    return got, twin


def run_mix(c):
    """one instance: element 0 of m channels (mono-coded or coupled by its channel count) and a second element of form k
    (1: mono for odd m, first-order ambisonics else; 2: a coupled stereo pair) into oc channels, calls of [1, 3, 2] frames"""
    m, oc, k = c.kw["m"], c.kw["oc"], c.kw["k"]
    m2 = 2 if k == 2 else (1 if m & 1 else 4)
    check(Mix(m, oc, m2, "pair" if k == 2 else "mono"), True, what=c.id)


CASES = [Case("lpcm_mix_m%d_oc%d_k%d" % (m, oc, k), inst(m, oc, k), run_mix, dict(m=m, oc=oc, k=k))
         for m in LPCM_M + COUPLED_M for oc in MIX_OC for k in MIX_K]
