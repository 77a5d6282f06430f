"""One case per kernel instance of the build (iamf_hip_route_instances) and one builder per kernel family.

A builder makes the smallest call pick_route() (iac_amd/csrc/render_route.hpp) or the resampler's launcher sends to the
case's instance, runs it on the GPU — three streams with their own seeds and gains, three calls whose state carries
over, then the flush — and checks two things: the launch tally (iamf_hip_route_tally) names exactly the instances the
calls were expected to take, and every stream equals the oracle.  Exact kernels bit for bit; the MFMA projections
within 1 LSB; the HRTF stages against the float64 convolution with the tolerance of tests/test_gpu_fir.py.

tests/test_route_coverage_cpu.py holds the cases against the library's listing (no GPU);
tests/test_gpu_route_coverage.py runs them, tests/test_gpu_layouts.py runs some of them again with their buffers under
the layouts of tests/gpu_util.py (kw["layout"], default: dense).  Importing this module needs neither a GPU nor the library.

Matrices: the reference's own table where it has one for the (inputs, outputs) pair, else a seeded dense matrix whose
columns sum to 1.4, so that the bursts of the hot programme (1.5 on every channel) drive the limiter.
"""
import contextlib
import ctypes as C
import os
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id inst build kw")
Unreachable = namedtuple("Unreachable", "id inst rule build kw")

S = 3                                   # streams of a case
EG, OG = [0.8, 1.0, 1.2], [1.0, 0.9, 1.0]   # element / output gain per stream

# the lists of render_route.hpp and resample_route.hpp, restated: tests/test_route_coverage_cpu.py fails when they drift
GENERIC_M = [1, 2, 4, 6, 8, 9, 10, 11, 12, 14, 16, 24]
FAST_M = [1, 2, 4, 6, 8, 9, 10, 12, 14, 16, 24]
WIDE4_M = [4, 6, 8, 9, 10, 12, 16]
WIDE4_C = [6, 8, 10, 12, 14, 24]
WIDE4_MIX_C = [6, 8, 10, 12]
WIDE4_DEMIX_M = [6, 8, 10, 12]
WIDE4_DEMIX_C = [6, 8, 10, 12, 24]
WIDE4_LFE_M = [4, 9, 16]
LPCM_M = [1, 4, 9, 16]
FAN_M = [4, 6, 8, 9, 12, 16]
FIR_M = [1, 4, 9, 16, 2, 6, 8, 10, 12]
RS_BLOCK_C = [1, 2, 6, 8, 10, 12, 14, 24]
RS_DIRECT_C = [1, 2, 6, 8, 10, 12]
# (in rate, out rate, taps N, planes NUMP) of the direct-mode instances
RS_DIRECT_RATES = [(16000, 48000, 64, 1), (48000, 32000, 96, 1), (96000, 48000, 128, 2), (48000, 16000, 192, 3)]

# channel count -> a layout of the tables with that many channels (outputs: sound systems; inputs: element layouts)
_OUT_SS = {1: "MONO", 2: "A", 6: "B", 8: "C", 10: "D", 11: "E", 12: "J", 14: "G", 24: "H"}
_IN_SS = {1: "MONO", 2: "STEREO", 6: "L51", 8: "L71", 10: "L514", 12: "L714"}
_ORDER = {1: 0, 4: 1, 9: 2, 16: 3}
# IAChannelLayoutType with M channels, for the parametric down-mixer and the demixer's layer stacks
_DOWN_PAIR = {(8, 2): (5, 1), (8, 1): (5, 0), (6, 2): (2, 1), (6, 1): (2, 0), (2, 1): (1, 0),
              (12, 10): (7, 6), (12, 8): (7, 3), (12, 6): (7, 8), (10, 8): (6, 3), (10, 6): (6, 8), (8, 6): (3, 8)}
_DEMIX_LAYERS = {6: [1, 2], 8: [0, 1, 2, 5], 10: [2, 4], 12: [1, 3, 7]}
_LAYOUT_SS = {2: "L51", 3: "L512", 4: "L514", 5: "L71", 6: "L712", 7: "L714", 8: "L312"}


def gen(m):
    return ("GENERIC", 0, m, 0, 0)


# ------------------------------------------------------------------------------------------
# shared pieces of the builders (GPU side: imported lazily)
# ------------------------------------------------------------------------------------------

@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _custom(A, O, kind, m, n, w, channels, lfe1=-1):
    """the same weights as a product and an oracle matrix (as gpu_util.identity_matrix builds its matrix)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = []
    for cls in (A.Matrix, O.Matrix):
        mx = cls()
        mx.kind, mx.in_id, mx.out_id, mx.channels, mx.lfe1, mx.lfe2, mx.m, mx.n = kind, 0, 0, channels, lfe1, -1, m, n
        mx.mat = w.ctypes.data_as(C.POINTER(C.c_float))
        mx._keep = w
        out.append(mx)
    return out


def matrices(m, c, table=True, salt=0):
    """(product matrix, oracle matrix) for m inputs and c output channels; salt: another seeded matrix for the same pair"""
    import iac_amd as A
    import oracle_lib as O
    if table and c in _OUT_SS:
        try:
            if m in _ORDER and m != 1:
                return A.get_h2m_matrix(_ORDER[m], A.SS[_OUT_SS[c]]), O.get_h2m(_ORDER[m], O.SS[_OUT_SS[c]])
            if m in _IN_SS:
                return A.get_m2m_matrix(A.SS[_IN_SS[m]], A.SS[_OUT_SS[c]]), O.get_m2m(O.SS[_IN_SS[m]], O.SS[_OUT_SS[c]])
        except (KeyError, AssertionError):
            pass
    rng = np.random.default_rng(1000 * m + c + 100000 * salt)
    w = rng.uniform(0.2, 1.0, size=(m, c)) * rng.choice([1.0, 1.0, 1.0, -1.0], size=(m, c))
    w[0] = np.abs(w[0])
    w = w * (1.4 / np.abs(w.sum(axis=0)))[None, :]
    return _custom(A, O, A.KIND_M2M, m, c, w, c)


def hot(m, frames, fs, seed=900):
    import synth
    return np.stack([synth.hot(seed + 7 * s, m, frames * fs, sigma=0.22, burst_phase=150 + 400 * s, burst_period=2300)
                     for s in range(S)])


def drive_limiter(O, omx, ch, x, eg=EG, og=OG):
    """x scaled, stream by stream, so that the rendered peak is at least 1.3 (threshold: -1 dB = 0.89): the limiter's
    recurrence must run in every stream.  The scale comes from the oracle's rendering, never from the code under test."""
    x = x.copy()
    for s in range(x.shape[0]):
        peak = float(np.abs(O.render(omx, x[s], ch)).max()) * eg[s % len(eg)] * og[s % len(og)]
        assert peak > 0.0
        if peak < 1.3:
            x[s] *= np.float32(1.3 / peak)
    return x


def compare(got, want, lsb, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if lsb == 0:
        assert np.array_equal(got, want), what
    else:
        d = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
        assert d <= lsb, (what, d)


def check_tally(tally, expected):
    """expected: {instance: launches} or [(instance, launches)], where an instance may appear more than once"""
    exp = {}
    for k, v in (expected.items() if isinstance(expected, dict) else expected):
        exp[k] = exp.get(k, 0) + v
    assert tally == exp, "launched %s, expected %s" % (sorted(tally.items()), sorted(exp.items()))


# ------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------

def run_matrix(c):
    """one matrix-rendered element: Generic, Nolim, Fast, Wide, Wide4, Wide4Lfe, and with a 1-channel second element the
    mixing variants of Fast and Wide4.  kw: m, oc, fs, calls (frames per call), fmt (16 / 24 / 32), limiter, mfma, second,
    lfe, env, streams (+ check: the streams compared), expect: [(instance, calls that take it)], layout (gpu_util.Layout)"""
    import torch
    import gpu_util as G
    import iac_amd as A
    import lfe_cases as LC
    import oracle_lib as O
    import synth
    k = c.kw
    m, oc, fs, calls = k["m"], k["oc"], k["fs"], k["calls"]
    bd = k.get("fmt", 16)
    fmt = {16: A.FMT_S16, 24: A.FMT_S24, 32: A.FMT_S32}[bd]
    limiter, mfma, second, lfe = k.get("limiter", True), k.get("mfma", False), k.get("second", False), k.get("lfe", False)
    ns = k.get("streams", S)
    check = k.get("check", list(range(ns)))
    layout = k.get("layout", G.DENSE)
    F = sum(calls)
    mx, omx = matrices(m, oc)
    if lfe:
        assert mx.kind == A.KIND_H2M and mx.lfe1 >= 0
        x = np.stack([LC.programme(500 + 7 * s + m, m, fs * F) * np.float32(2.5) for s in range(ns)])
    else:
        x = hot(m, F, fs)
    eg, og = (EG, OG) if ns == S else ([EG[s % 3] for s in range(ns)], [OG[s % 3] for s in range(ns)])
    proj = A.PROJ_MFMA if mfma else A.PROJ_EXACT
    if limiter:
        x = drive_limiter(O, omx, oc, x, eg, og)
    with environment(k.get("env", {})):
        A.route_reset()
        if second:
            mx2, omx2 = matrices(1, oc, table=False)
            x2 = np.stack([synth.hot(271 + s, 1, F * fs, sigma=0.3, burst_phase=900, burst_period=1700) for s in range(ns)])
            eg2 = [0.6, 1.0, 0.9]
            b = A.Batch(ns, mx, oc, frame_size=fs, out_format=fmt, projection=proj)
            b.set_gains(element=eg, output=og)
            b.set_second_element(mx2, eg2)
            got = G.run_ex(A, G, torch, b, ns, m, x, fs, oc, fmt, x2=x2, m2=1, calls=calls, layout=layout)
            b.close()
        else:
            got = G.hip_render(mx, oc, x, frame_size=fs, fmt=fmt, limiter=limiter, flush=True, frames_per_call=calls,
                               gains=dict(element=eg, output=og), projection=proj, lfe_hoa=lfe, layout=layout)
        tally = A.route_tally()
    for s in check:
        if second:
            y0, y1 = O.render(omx, x[s], oc), O.render(omx2, x2[s], oc)
            for y, g in ((y0, eg[s]), (y1, eg2[s])):
                if g != 1.0:
                    O.lib().orc_frame_gain_const(O.fp(y), oc, F * fs, g)
            z = ((np.zeros_like(y0) + y0) + y1).astype(np.float32)
            if og[s] != 1.0:
                O.lib().orc_frame_gain_const(O.fp(z), oc, F * fs, og[s])
            z, _ = O.limiter_run(z, [fs] * F)
            want = O.pack(z, bd)
        else:
            want = O.stream_run(omx, oc, x[s], fs, element_gain=eg[s], output_gain=og[s], limiter_on=int(limiter), bit_depth=bd,
                                lfe_rate=48000 if lfe else 0)
        compare(got[s], want, 1 if mfma else 0, (c.id, s))
    expect = dict(k["expect"]) if "expect" in k else {c.inst: len(calls)}
    if limiter:
        expect[gen(m)] = expect.get(gen(m), 0) + 1          # the flush: 240 zero samples on the generic kernel
    check_tally(tally, expect)


def run_lpcm(c):
    """a mono-coded ambisonics element as 16-bit LPCM packets (render_fast_kernel<M, OC, .., LP>); kw: m, oc, env, streams,
    check, calls, layout (the PCM side)"""
    import iac_amd as A
    import lpcm_util as LP
    import oracle_lib as O
    k = c.kw
    m, oc, fs = k["m"], k["oc"], 1024
    calls = k.get("calls", [1, 3, 2])
    ns = k.get("streams", S)
    check = k.get("check", list(range(ns)))
    F = sum(calls)
    rng = np.random.default_rng(100 + 16 * m + oc)
    ints = LP.ints(rng, ns, F, m, fs, 2)
    ints[:, :, :, ::97] = (31000 * (-1) ** np.arange(ints[0, 0, 0, ::97].size))[None, None, None, :]   # bursts on every channel at once
    perm = list(rng.permutation(m))
    x = (ints[:, :, perm, :].astype(np.float64) / 32768.0).astype(np.float32)       # [S][F][m][fs], exact
    planar = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(ns, m, F * fs)
    mx, omx = matrices(m, oc)
    if min(float(np.abs(O.render(omx, planar[s], oc)).max()) for s in check) <= 0.95:
        mx, omx = matrices(m, oc, table=False)   # full-scale samples stay under the threshold through the table's weights
    raw, L, row = LP.rows(ints, 2, True, [1] * m, perm, head=16, pad=0, frame_size=fs)
    with environment(k.get("env", {})):
        A.route_reset()
        got = LP.render_lpcm(mx, oc, raw, L, row, fs, calls, layout=k.get("layout", LP.G.DENSE))
        tally = A.route_tally()
    for s in check:
        want = O.stream_run(omx, oc, planar[s], fs)
        assert float(np.abs(O.render(omx, planar[s], oc)).max()) > 0.95, "the programme does not drive the limiter"
        compare(got[s].view(np.int16).reshape(-1, oc), want, 0, (c.id, s))
    check_tally(tally, [(c.inst, len(calls)), (gen(m), 1)])


def run_fanout(c):
    """one element into K one- and two-channel batches in one launch (render_fanout_kernel<M, K>); kw: m, k, calls, layout,
    fused: the members a call renders in the shared launch (K, or 0 where every member is rendered singly: c.inst then
    names the kernel each of them takes)"""
    import torch
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    m, K = c.kw["m"], c.kw["k"]
    fs, calls = 1024, c.kw.get("calls", [1, 3, 2])
    layout, n_fused = c.kw.get("layout", G.DENSE), c.kw.get("fused", K)
    F = sum(calls)
    ocs = [2, 1, 2, 1][:K]
    mxs = [matrices(m, oc, table=(j < 2), salt=j) for j, oc in enumerate(ocs)]   # members 2, 3: the same layouts, other weights
    gains = [(EG, OG), (OG, EG), ([1.1, 0.7, 1.0], OG), (EG, [0.9, 1.0, 1.1])][:K]
    x = hot(m, F, fs)
    for j in range(K):   # every member's limiter must work
        x = drive_limiter(O, mxs[j][1], ocs[j], x, gains[j][0], gains[j][1])
    xf = G.to_frames(x, fs)
    st = torch.cuda.current_stream().cuda_stream
    batches = []
    for j in range(K):
        b = A.Batch(S, mxs[j][0], ocs[j], frame_size=fs, projection=A.PROJ_EXACT)
        b.set_gains(element=gains[j][0], output=gains[j][1])
        batches.append(b)
    outs = [[[] for _ in range(S)] for _ in range(K)]

    def take(j, rows, n):
        torch.cuda.synchronize()
        h = G.rows_and_rest(rows, layout, n * ocs[j] * 2)
        for s in range(S):
            outs[j][s].append(h[s].view(np.int16).reshape(n, ocs[j]).copy())

    A.route_reset()
    f0 = 0
    keep = pcms = rows = None
    try:
        for nf in calls:
            caps = [(nf * fs * oc * 2 + 15) & ~15 for oc in ocs]
            pcms = [G.pcm_rows(S, cap, layout) for cap in caps]
            pl = G.place_input(xf, layout, f0, nf, keep=keep)
            keep = pl.keep
            n_emitted, fused = A.render_fanout(batches, pl.d_in, pl.stream_stride, pl.frame_stride, nf,
                                               [p[1] for p in pcms], [p[2] for p in pcms], st)
            assert fused == n_fused, (fused, n_fused)
            for j in range(K):
                take(j, pcms[j][0], n_emitted[j])
            pcms = None
            f0 += nf
        for j, b in enumerate(batches):
            cap = 240 * ocs[j] * 2
            rows, d_pcm, stride = G.pcm_rows(S, cap, layout)
            take(j, rows, b.flush(d_pcm, stride, st))
            rows = None
    finally:
        keep = pcms = rows = pl = None
        for b in batches:
            b.close()
    tally = A.route_tally()
    for j in range(K):
        for s in range(S):
            want = O.stream_run(mxs[j][1], ocs[j], x[s], fs, element_gain=gains[j][0][s], output_gain=gains[j][1][s])
            compare(np.concatenate(outs[j][s]), want, 0, (c.id, j, s))
    check_tally(tally, [(c.inst, len(calls) * (1 if n_fused else K)), (gen(m), K)])


def _ex_loop(A, b, x, per_call_extra, calls, oc, layout=None):
    """x [S][F][m][fs]; render_ex per entry of calls (frames), then the flush; per_call_extra(a, f0, nf) fills the stage's
    fields of the call's RenderArgs and returns what must stay alive.  Returns per stream [n][oc] int16."""
    import torch
    import gpu_util as G
    layout = layout or G.DENSE
    ns, F, m, fs = x.shape
    st = torch.cuda.current_stream().cuda_stream
    outs = [[] for _ in range(ns)]
    f0 = 0
    placed = rows = pl = keep = None
    try:
        for nf in calls + [0]:
            cap = max(nf * fs, 240) * oc * 2
            rows, d_pcm, stride = G.pcm_rows(ns, cap, layout)
            if nf:
                a = A.RenderArgs()
                pl = G.place_input(x, layout, f0, nf, keep=placed)
                placed = pl.keep
                a.d_in, a.in_stream_stride, a.in_frame_stride = pl.d_in, pl.stream_stride, pl.frame_stride
                a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, d_pcm, stride, st
                keep = per_call_extra(a, f0, nf)
                n = b.render_ex(a)
            else:
                keep = None
                n = b.flush(d_pcm, stride, st)
            torch.cuda.synchronize()
            del keep
            h = G.rows_and_rest(rows, layout, n * oc * 2)
            rows = None
            for s in range(ns):
                outs[s].append(h[s].view(np.int16).reshape(n, oc).copy())
            f0 += nf
    finally:
        placed = rows = pl = None
    return [np.concatenate(o, axis=0) for o in outs]


def run_down(c):
    """the parametric down-mixer: render_fast_kernel<.., DOWN> (mono / stereo) and render_wide4_kernel<.., DOWN>; kw: m, oc, calls, layout"""
    import torch
    import iac_amd as A
    import oracle_lib as O
    import synth
    L = A.lib()
    m, oc = c.kw["m"], c.kw["oc"]
    il, ol = _DOWN_PAIR[(m, oc)]
    assert L.iamf_hip_dmx_valid(il, ol) == 1 and O.LAYOUT_CH[il] == m and O.LAYOUT_CH[ol] == oc
    fs, calls = 1024, c.kw.get("calls", [1, 3, 2])
    F = sum(calls)
    sched = [((-1, 1, 2, 4, 5, 6, 0, 2)[f % 8], (0, 0, 37, 128, 0, fs - 3, 4, 0)[f % 8]) for f in range(F)]
    x = np.stack([np.stack([synth.hot(500 + 31 * s + f, m, fs, sigma=0.3, burst_phase=100 + 50 * f, burst_period=700)
                            for f in range(F)]) for s in range(S)])               # [S][F][m][fs]
    frames = (A.DmxFrame * (S * F))()
    stt = A.DmxState()
    for s in range(S):
        L.iamf_hip_dmx_state_init(C.byref(stt))
        L.iamf_hip_dmx_set_mode_weight(C.byref(stt), 1, 3)
        for f, (mode, off) in enumerate(sched):
            fr = frames[s * F + f]
            fr.offset = off
            L.iamf_hip_dmx_coefficients(C.byref(stt), fr.prev)
            if mode > -1:
                L.iamf_hip_dmx_set_mode_weight(C.byref(stt), mode, -1)
            L.iamf_hip_dmx_coefficients(C.byref(stt), fr.cur)
    rec = np.frombuffer(bytes(frames), dtype=np.uint8).reshape(S, F, -1)

    def extra(a, f0, nf):
        d = torch.from_numpy(rec[:, f0:f0 + nf].copy()).cuda()    # the records of this call's frames, [S][nf]
        a.d_dmx_frames = d.data_ptr()
        return d

    A.route_reset()
    b = A.Batch(S, A.dmx_matrix(il, ol), oc, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    got = _ex_loop(A, b, x, extra, calls, oc, c.kw.get("layout"))
    b.close()
    tally = A.route_tally()
    for s in range(S):
        y = O.downmix_run(il, ol, x[s], sched, 1, 3)                     # [F][oc][fs]
        yd = np.ascontiguousarray(y.transpose(1, 0, 2).reshape(oc, F * fs))
        assert float(np.abs(yd).max()) > 1.2, "the programme does not drive the limiter"
        z, _ = O.limiter_run(yd, [fs] * F)
        compare(got[s], O.pack(z, 16), 0, (c.id, s))
    check_tally(tally, [(c.inst, len(calls)), (gen(m), 1)])


def demix_frames(A, c, ns):
    """the per-frame records of iamf_hip_batch_set_demixer's stage for a case of demix_cases.py, [ns * frames]"""
    F = len(c["schedule"])
    frames = (A.DemixFrame * (ns * F))()
    st = A.DemixState()
    rec = (C.c_int32 * 12)(*c["recon"])
    for s in range(ns):
        A.lib().iamf_hip_demix_state_init(C.byref(st))
        A.lib().iamf_hip_demix_set_info(C.byref(st), c["default"][0], c["default"][1])
        cur = [1.0] * len(c["recon"])
        for f, (mode, rg) in enumerate(c["schedule"]):
            if rg is not None:
                cur = rg
            if mode > -1:
                A.lib().iamf_hip_demix_set_info(C.byref(st), mode, -1)
            A.lib().iamf_hip_demix_frame_fill(C.byref(st), len(cur), rec, (C.c_float * 12)(*cur),
                                              C.byref(frames[s * F + f]))
    return frames


def demix_render(A, c, mx, out_ch, x, calls):
    """x [S][F][ch][fs] decoded channels -> demixer -> mx -> limiter -> s16; one render_ex per entry of `calls`, then
    the flush.  Returns [S][n][out_ch].  An entry of `calls` is
      nf               that many whole frames;
      (s0, n)          ONE frame whose first s0 samples were trimmed away before the call and of which n are rendered, given
                       the way the decoder facade's render_tu gives it (include/iamf_hip.h, iamf_hip_render_args): every
                       channel row starts at the first KEPT sample (rows stay frame_size apart; what lies behind the n
                       samples is NaN here, nothing may read it), the record is the frame's own, n_frames = 1,
                       demix_sample0 = s0, n_samples = n (0 for a whole frame);
      ("refuse", s0, n)  the same call on the next frame, which must be refused with IAMF_HIP_ERR_BAD_ARG: it consumes no
                       frame and emits nothing."""
    import torch
    S, F, ch, fs = x.shape
    b = A.Batch(S, mx, out_ch, frame_size=fs, out_format=A.FMT_S16, limiter=True)
    b.set_demixer(c["layout"], c["order"], c["gains"], c["offset"])
    frames = demix_frames(A, c, S)
    xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    outs = [[] for _ in range(S)]
    f0 = 0
    for call in list(calls) + [0]:
        refuse = isinstance(call, tuple) and call[0] == "refuse"
        s0, n = (call[-2], call[-1]) if isinstance(call, tuple) else (0, 0)
        nf = 1 if isinstance(call, tuple) else call
        cap = max(nf * fs, 240) * out_ch * 2
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        if nf:
            # the records of this call's frames, [S][nf]
            raw = np.frombuffer(bytes(frames), dtype=np.uint8).reshape(S, F, -1)[:, f0:f0 + nf].copy()
            d_fr = torch.from_numpy(raw).cuda()
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = xin.data_ptr() + 4 * f0 * ch * fs, F * ch * fs, ch * fs
            if isinstance(call, tuple):
                cut = np.full((S, ch, fs), np.nan, dtype=np.float32)
                keep = x[:, f0, :, max(s0, 0):max(s0, 0) + n]
                cut[:, :, :keep.shape[2]] = keep
                d_cut = torch.from_numpy(cut).cuda()
                a.d_in, a.in_stream_stride = d_cut.data_ptr(), ch * fs
                a.demix_sample0, a.n_samples = s0, (n if n < fs else 0)
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr(), cap, st
            a.d_demix_frames = d_fr.data_ptr()
            if refuse:
                try:
                    b.render_ex(a)
                except A.IamfHipError as e:
                    assert e.code == -1, e   # IAMF_HIP_ERR_BAD_ARG
                else:
                    raise AssertionError("demix_sample0 %d with %d samples of %d was not refused" % (s0, n, fs))
                torch.cuda.synchronize()
                assert not pcm.cpu().numpy().any()
                continue
            n = b.render_ex(a)
        else:
            n = b.flush(pcm.data_ptr(), cap, st)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(h[s][:n * out_ch * 2].view(np.int16).reshape(n, out_ch).copy())
        f0 += nf
    b.close()
    return [np.concatenate(o, axis=0) for o in outs]


def run_demix(c):
    """scalable channel audio: the demixer in front of the projection (render_wide4_kernel<.., DMX>); kw: m, oc, calls, layout"""
    import torch
    import demix_cases as D
    import iac_amd as A
    import oracle_lib as O
    import synth
    m, oc = c.kw["m"], c.kw["oc"]
    fs, calls = 1024, c.kw.get("calls", [1, 2, 1])
    F = sum(calls)
    dc = D.make_case(_DEMIX_LAYERS[m], default=(1, 3), offset=8, fs=fs, seed=770 + m)
    dc["schedule"] = dc["schedule"][:F]
    assert len(dc["order"]) == m
    src = _LAYOUT_SS[dc["layout"]]
    try:
        mx, omx = A.get_m2m_matrix(A.SS[src], A.SS[_OUT_SS[oc]]), O.get_m2m(O.SS[src], O.SS[_OUT_SS[oc]])
    except (KeyError, AssertionError):
        mx, omx = matrices(m, oc, table=False)
    x = np.stack([np.stack([synth.uniform(dc["seed"] + 100 * s + f, m, fs, 1.5) for f in range(F)]) for s in range(S)])
    rec = np.frombuffer(bytes(demix_frames(A, dc, S)), dtype=np.uint8).reshape(S, F, -1)

    def extra(a, f0, nf):
        d = torch.from_numpy(rec[:, f0:f0 + nf].copy()).cuda()
        a.d_demix_frames = d.data_ptr()
        return d

    A.route_reset()
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True, projection=A.PROJ_EXACT)
    b.set_demixer(dc["layout"], dc["order"], dc["gains"], dc["offset"])
    got = _ex_loop(A, b, x, extra, calls, oc, c.kw.get("layout"))
    b.close()
    tally = A.route_tally()
    for s in range(S):
        dem = D.drive_demixer(O.lib(), "orc_demixer_", dc, x[s])   # [F][m][fs]
        xd = np.ascontiguousarray(dem.transpose(1, 0, 2).reshape(m, F * fs))
        assert float(np.abs(O.render(omx, xd, oc)).max()) > 1.2, "the programme does not drive the limiter"
        compare(got[s], O.stream_run(omx, oc, xd, fs), 0, (c.id, s))
    check_tally(tally, [(c.inst, len(calls)), (gen(m), 1)])


def run_fir(c):
    """the HRTF stage against the float64 convolution, tolerance and set-up of tests/test_gpu_fir.py; kw: m, env, calls, layout,
    refused: (layout, error code, frames) of a first call that must be refused and change nothing (gpu_util.hip_render)"""
    import gpu_util as G
    import iac_amd as A
    import synth
    from test_gpu_fir import F32_TOL, fir64, hrir_set
    m = c.kw["m"]
    fs, calls, taps = 1024, c.kw.get("calls", [1, 3, 2]), 256
    F = sum(calls)
    x = np.stack([synth.gaussian(800 + s, m, F * fs, 0.1) for s in range(S)])
    h = hrir_set(5 + m, m, taps)
    with environment(c.kw.get("env", {})):
        A.route_reset()
        got = G.hip_render(A.fir_matrix(h), 2, x, frame_size=fs, fmt=A.FMT_F32, limiter=True, flush=True,
                           frames_per_call=calls, fir_taps=taps, layout=c.kw.get("layout", G.DENSE),
                           refused=c.kw.get("refused"))
        tally = A.route_tally()
    for s in range(S):
        y = fir64(h, x[s])
        assert np.abs(y).max() < 0.85   # the limiter stays at unity gain: output = the stage's output, delayed
        assert got[s].shape == (F * fs, 2)
        assert np.abs(got[s].T - y).max() <= F32_TOL, (c.id, s, float(np.abs(got[s].T - y).max()))
    expect = {c.inst: len(calls), gen(m): 1}
    if c.inst[0] == "FIR_SPLIT":
        expect[("FAST", 0, 2, 2, 0)] = len(calls)   # gains, limiter and pack behind the stage
    check_tally(tally, expect)


def run_resample(c):
    """kw: rates, ch, streams, env, layout (input rows as one frame of one channel each, output rows as PCM rows of
    floats).  Three calls of unequal length and the drain, streams 0, the middle and the last one
    bit for bit against the oracle."""
    import torch
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    k = c.kw
    layout = k.get("layout", G.DENSE)
    (r_in, r_out), ch, ns = k["rates"], k["ch"], k["streams"]
    sizes = [700, 1300, 333]
    rng = np.random.default_rng(ch * 1000 + ns)
    x = (rng.standard_normal((ns, sum(sizes), ch)) * 0.3).astype(np.float32)
    x[:, 100:140] *= 4.0   # beyond +-1: the clamp
    st = torch.cuda.current_stream().cuda_stream
    with environment(k.get("env", {})):
        A.route_reset()
        r = A.Resampler(ns, ch, r_in, r_out)
        outs, pos = [], 0
        for n_in in sizes:
            inter = G.place_input(x[:, pos:pos + n_in].reshape(ns, 1, 1, n_in * ch), layout)
            pos += n_in
            cap = max(r.out_capacity(n_in), 1)
            rows, d_out, stride = G.pcm_rows(ns, cap * ch * 4, layout, bps=4)
            n = r.process(inter.d_in, inter.stream_stride, n_in, d_out, stride // 4, st)
            torch.cuda.synchronize()
            assert n >= 0, n
            # (rows_and_rest: nothing is written past the call's outputs)
            outs.append(np.stack(G.rows_and_rest(rows, layout, n * ch * 4)).view(np.float32).reshape(ns, n, ch))
        cap = max(r.flush_capacity(), 1)
        rows, d_out, stride = G.pcm_rows(ns, cap * ch * 4, layout, bps=4)
        n = r.flush(d_out, stride // 4, st)
        torch.cuda.synchronize()
        outs.append(np.stack(G.rows_and_rest(rows, layout, n * ch * 4)).view(np.float32).reshape(ns, n, ch))
        del rows, inter
        r.close()
        tally = A.route_tally()
    got = np.concatenate(outs, axis=1)
    for s_ in sorted({0, ns // 2, ns - 1}):
        want, _ = O.resample_run(np.ascontiguousarray(x[s_].T), r_in, r_out, sizes)
        g = np.ascontiguousarray(got[s_].T)
        assert g.shape == want.shape, (c.id, s_, g.shape, want.shape)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (c.id, s_)
    check_tally(tally, {k.get("routed", c.inst): len(sizes) + 1})


def resampler_filter(in_rate, out_rate):
    """(num, den, taps, direct mode) of a quality-4 resampler, as iamf_hip_resampler_create derives them (resample.c:527-611)"""
    from math import gcd
    g = gcd(in_rate, out_rate)
    num, den = in_rate // g, out_rate // g
    n, oversample = 64, 8
    if num > den:
        n = ((n * num // den - 1) & ~7) + 8
        for k in (2, 4, 8, 16):
            if k * den < num:
                oversample >>= 1
        oversample = max(oversample, 1)
    return num, den, n, n * den <= n * oversample + 8


def resampler_instance(in_rate, out_rate, ch, streams):
    """the instance rs_run (iamf_resample.hip) launches without switches, restated from its rules; the tally on the GPU is
    what pins it"""
    num, den, n, direct = resampler_filter(in_rate, out_rate)
    if direct:
        nump = num if den == 1 else 1
        if den <= 16 and ch in RS_DIRECT_C and (n, nump) in [(r[2], r[3]) for r in RS_DIRECT_RATES] and (n != 192 or ch == 6 or ch >= 10):
            return ("RS_DIRECT", nump, n, ch, 4 if ch <= 2 else (2 if ch <= 8 else 1))
        return ("RS_TILE", 1, 0, 0, 0)
    if den <= 512 and ch in RS_BLOCK_C:
        r = 4 if streams >= 256 else (2 if streams >= 64 else 1)
        return ("RS_BLOCK", 0, 0, ch, min(r, 4 if ch <= 2 else (2 if ch <= 8 else 1)))
    return ("RS_TILE", 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------

def _cases():
    out = []

    def add(cid, inst, build, **kw):
        out.append(Case(cid, inst, build, kw))

    # Generic: a ragged call (1000-sample frames: no multiple of 64) that every other kernel refuses
    for m in GENERIC_M:
        add("generic_m%d" % m, gen(m), run_matrix, m=m, oc=2, fs=1000, calls=[1, 2, 1])
    # Nolim: limiter off
    for m in GENERIC_M:
        add("nolim_m%d" % m, ("NOLIM", 0, m, 0, 0), run_matrix, m=m, oc=2, fs=1024, calls=[1, 3, 2], limiter=False)
    # Fast<M, OC>, plain and with a 1-channel second element
    for mixing in (0, 1):
        for m in FAST_M:
            for oc in (1, 2):
                add("fast_m%d_oc%d%s" % (m, oc, "_mix" if mixing else ""), ("FAST", mixing, m, oc, 0), run_matrix, m=m, oc=oc,
                    fs=1024, calls=[1, 3, 2], second=bool(mixing))
    for (m, oc) in [(8, 2), (8, 1), (6, 2), (6, 1), (2, 1)]:
        add("fast_down_%d_%d" % (m, oc), ("FAST_DOWN", 0, m, oc, 0), run_down, m=m, oc=oc)
    # Wide<M, MFMA>: 11 channels (Sound System E: odd, no wide4 layout), 256-sample chunks
    for mfma in (0, 1):
        for m in FAST_M:
            add("wide_m%d_c11%s" % (m, "_mfma" if mfma else ""), ("WIDE", mfma, m, 0, 0), run_matrix, m=m, oc=11, fs=256,
                calls=[1, 2, 3], mfma=bool(mfma))
        for m in (1, 14, 24):   # 24 channels is a wide4 layout, but these inputs are not wide4's
            add("wide_m%d_c24%s" % (m, "_mfma" if mfma else ""), ("WIDE", mfma, m, 0, 0), run_matrix, m=m, oc=24, fs=256,
                calls=[1, 2, 3], mfma=bool(mfma))
    for bd in (24, 32):         # wide4 packs 16 bit only: other formats of its layouts take this kernel
        add("wide_m12_c11_s%d" % bd, ("WIDE", 0, 12, 0, 0), run_matrix, m=12, oc=11, fs=256, calls=[1, 2, 3], fmt=bd)
        add("wide_m12_c12_s%d" % bd, ("WIDE", 0, 12, 0, 0), run_matrix, m=12, oc=12, fs=256, calls=[1, 2, 3], fmt=bd)
    for mfma in (0, 1):
        for m in WIDE4_M:
            for ch in WIDE4_C:
                add("wide4_m%d_c%d%s" % (m, ch, "_mfma" if mfma else ""), ("WIDE4", mfma, m, ch, 0), run_matrix, m=m, oc=ch,
                    fs=1024, calls=[1, 3, 2], mfma=bool(mfma))
    for m in WIDE4_DEMIX_M:
        for ch in WIDE4_DEMIX_C:
            add("wide4_demix_m%d_c%d" % (m, ch), ("WIDE4_DEMIX", 0, m, ch, 0), run_demix, m=m, oc=ch)
    for (m, oc) in [(12, 10), (12, 8), (12, 6), (10, 8), (10, 6), (8, 6)]:
        add("wide4_down_%d_%d" % (m, oc), ("WIDE4_DOWN", 0, m, oc, 0), run_down, m=m, oc=oc)
    for mfma in (0, 1):
        for m in WIDE4_M:
            for ch in WIDE4_MIX_C:
                add("wide4_mix_m%d_c%d%s" % (m, ch, "_mfma" if mfma else ""), ("WIDE4_MIX", mfma, m, ch, 0), run_matrix, m=m,
                    oc=ch, fs=1024, calls=[1, 3, 2], mfma=bool(mfma), second=True)
    for mfma in (0, 1):
        for m in WIDE4_LFE_M:
            for ch in WIDE4_C:
                add("wide4_lfe_m%d_c%d%s" % (m, ch, "_mfma" if mfma else ""), ("WIDE4_LFE", mfma, m, ch, 0), run_matrix, m=m,
                    oc=ch, fs=1024, calls=[1, 3, 2], mfma=bool(mfma), lfe=True)
    # the remap of workgroups to streams at n_launch % 512 == 0 (render_wide4.hpp), and one stream short of it
    for ns in (512, 511):
        add("wide4_lfe_m4_c6_%d_streams" % ns, ("WIDE4_LFE", 0, 4, 6, 0), run_matrix, m=4, oc=6, fs=1024, calls=[1, 1], lfe=True,
            streams=ns, check=[s for s in (0, 1, 7, 8, 63, 64, 448, 511) if s < ns])
    for early in (1, 0):
        for m in LPCM_M:
            for oc in (1, 2):
                add("lpcm_m%d_oc%d_%s" % (m, oc, "early" if early else "late"), ("LPCM", early, m, oc, 0), run_lpcm, m=m, oc=oc,
                    env={} if early else {"IAMF_HIP_LP_LATE": "1"})
    # late for real: more than 1024 streams in the launch
    add("lpcm_m1_oc2_1025_streams", ("LPCM", 0, 1, 2, 0), run_lpcm, m=1, oc=2, streams=1025, calls=[1], check=[0, 1023, 1024])
    for m in FAN_M:
        for k in (2, 3, 4):
            add("fanout_m%d_k%d" % (m, k), ("FANOUT", 0, m, 0, k), run_fanout, m=m, k=k)
    for m in FIR_M:
        add("fir_split_m%d" % m, ("FIR_SPLIT", 0, m, 0, 0), run_fir, m=m)
        for stage, sw in ((3, "IAMF_HIP_FIR_FUSED"), (2, "IAMF_HIP_FIR_F16"), (1, "IAMF_HIP_FIR_F32")):
            add("fir_fused%d_m%d" % (stage, m), ("FIR_FUSED", stage, m, 0, 0), run_fir, m=m, env={sw: "1"})
    # ---- resampler ----
    add("rs_plain", ("RS_PLAIN", 0, 0, 0, 0), run_resample, rates=(44100, 48000), ch=2, streams=3, env={"IAMF_HIP_RESAMPLE_PLAIN": "1"})
    add("rs_tile_interpolated", ("RS_TILE", 0, 0, 0, 0), run_resample, rates=(44100, 48000), ch=2, streams=3,
        env={"IAMF_HIP_RESAMPLE_TILE": "1"})
    add("rs_tile_direct", ("RS_TILE", 1, 0, 0, 0), run_resample, rates=(96000, 48000), ch=2, streams=3,
        env={"IAMF_HIP_RESAMPLE_TILE": "1"})
    # block<C, R>: R = 4 from 256 streams, 2 from 64, else 1, and at most what the channel count allows
    for ch in RS_BLOCK_C:
        rmax = 4 if ch <= 2 else (2 if ch <= 8 else 1)
        for r, ns in ((1, 63), (2, 64), (4, 256)):
            if r <= rmax:
                add("rs_block_c%d_r%d" % (ch, r), ("RS_BLOCK", 0, 0, ch, r), run_resample, rates=(44100, 48000), ch=ch, streams=ns)
    add("rs_block_c2_r2_255_streams", ("RS_BLOCK", 0, 0, 2, 2), run_resample, rates=(44100, 48000), ch=2, streams=255)
    add("rs_block_c6_r2_256_streams", ("RS_BLOCK", 0, 0, 6, 2), run_resample, rates=(44100, 48000), ch=6, streams=256)
    add("rs_block_c12_r1_64_streams", ("RS_BLOCK", 0, 0, 12, 1), run_resample, rates=(44100, 48000), ch=12, streams=64)
    for ch in RS_DIRECT_C:
        r = 4 if ch <= 2 else (2 if ch <= 8 else 1)
        for (r_in, r_out, n, nump) in RS_DIRECT_RATES:
            if n == 192 and ch in (1, 2, 8):
                continue   # UNREACHABLE below
            add("rs_direct_c%d_n%d" % (ch, n), ("RS_DIRECT", nump, n, ch, r), run_resample, rates=(r_in, r_out), ch=ch, streams=3)
    # the stream counts at which the launcher changes its tile (G), both sides of 64 and 256
    for (r_in, r_out, n, nump) in RS_DIRECT_RATES[:3]:
        for ns in (63, 64, 255, 256):
            add("rs_direct_c2_n%d_%d_streams" % (n, ns), ("RS_DIRECT", nump, n, 2, 4), run_resample, rates=(r_in, r_out), ch=2,
                streams=ns)
    for ns in (64, 256):
        add("rs_direct_c6_n192_%d_streams" % ns, ("RS_DIRECT", 3, 192, 6, 2), run_resample, rates=(48000, 16000), ch=6, streams=ns)
    return out


CASES = _cases()

# Instances the build holds that no call through the public ABI reaches: the rule that shuts each out, and the nearest
# call, which the GPU test runs and asserts is routed elsewhere.
UNREACHABLE = [
    Unreachable("rs_direct_c%d_n192" % ch, ("RS_DIRECT", 3, 192, ch, r),
                "rs_direct_takes() (resample_route.hpp): 3:1 down-sampling with 1, 2 or 8 channels is left to the tiled kernel, "
                "which measured faster; rs_direct_launch instantiates every (N, NUMP) for every channel count of its list",
                run_resample, dict(rates=(48000, 16000), ch=ch, streams=3, routed=("RS_TILE", 1, 0, 0, 0)))
    for ch, r in ((1, 4), (2, 4), (8, 2))
]
