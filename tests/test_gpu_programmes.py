"""-m gpu: the render kernels on the structured programmes of tests/programmes.py — silence, full releases, plateaus and
ties, trigger runs across chunks and calls, peaks on every boundary, re-triggers on the limiter's phase boundaries,
rounding ties and clamps of the pack code, denormal, off-scale and non-finite input, and the demixer's slow quotients.

The branches these programmes are for are taken on the VALUES of the signal; the noise of the other GPU tests does not
reach them.  One programme per stream of one batch, so a family costs one short sequence of launches.  Every test
asserts with the launch tally (iamf_hip_route_tally) that the instance it names ran (the flush of a limiter-on batch is
one launch of the generic kernel, as in route_cases.run_matrix), and compares every stream with the oracle: bit for bit,
f32 output by bits with NaN positions equal, the MFMA projections within 1 LSB.  The matrices are selection matrices
(weights 0 and 1, each output copies one input), so the rendered signal is the programme and what
tests/test_programmes_cpu.py proves about it holds here; one further pass per family uses the reference's table matrix.
The FIR stages are not part of this (their parity is unpinned by design) and neither is the resampler (no branch of it
depends on the values)."""
import ctypes as C

import numpy as np
import pytest

import programmes as P
import route_cases as R

pytestmark = pytest.mark.gpu

FS, CALLS = 1024, [1, 3, 2, 5, 1]          # 12 frames: chunk, call and release boundaries fall in different places
N = FS * sum(CALLS)
CALLS_BY_FRAMES = {12: CALLS, 11: [1, 3, 2, 4, 1], 5: [1, 3, 1], 21: [1, 3, 2, 5, 1, 9]}
SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_PROJECTION", "IAMF_HIP_LP_LATE", "IAMF_HIP_LPCM_UNFUSED")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _mods():
    import gpu_util as G
    import iac_amd as A
    import oracle_lib as O
    return A, G, O


def selection(m, oc, kind=None, channels=None, lfe1=-1, weight=1.0):
    """(product matrix, oracle matrix): output o copies input o % m (weight: times that, programmes.PACKET_WEIGHT for the
    packet-fed kernels)"""
    A, G, O = _mods()
    if kind == A.KIND_H2M:                  # rows = the feeds (the LFE slot is no feed)
        n = channels - 1
        w = np.zeros((n, m), dtype=np.float32)
        w[np.arange(n), np.arange(n) % m] = 1.0
        return R._custom(A, O, A.KIND_H2M, m, n, w, channels, lfe1)
    w = np.zeros((m, oc), dtype=np.float32)
    w[np.arange(oc) % m, np.arange(oc)] = weight
    return R._custom(A, O, A.KIND_M2M, m, oc, w, oc)


def limiter_set(m, n=N, rate=48000, nonfinite=True, sweep=True):
    """[(name, x [m][n])]: every limiter programme, the re-trigger sweep one position per stream"""
    out = [(f.__name__, f(m, n, rate)) for f in P.LIMITER_FINITE]
    if nonfinite:
        out.append(("nonfinite", P.nonfinite(m, n, rate)))
    if sweep:
        out += [("retrigger_sweep_k%d" % k, P.retrigger_sweep(m, n, rate, k=k)) for k in range(P.SWEEP)]
    return out


def some(m, names, n=N, rate=48000):
    return [(nm, getattr(P, nm)(m, n, rate)) for nm in names]


def mismatch(got, want, lsb=0):
    """None, or what differs"""
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32)))
    elif lsb:
        bad = np.abs(got.astype(np.int64) - want.astype(np.int64)) > lsb
    else:
        bad = got != want
    if not bad.any():
        return None
    i = tuple(int(v) for v in np.argwhere(bad)[0])
    return "%d values differ, first at %s: %s, expected %s" % (int(bad.sum()), i, got[i], want[i])


def oracle_stream(O, omx, oc, x, fs, bd, limiter=True, thr=-1.0, rate=48000, lfe=False):
    """[n_out][oc]: integer PCM through the oracle's stream, f32 (bd = -32) as render (+ limiter)"""
    with np.errstate(all="ignore"):
        if bd > 0:
            return O.stream_run(omx, oc, x, fs, limiter_on=int(limiter), thr_db=thr, rate=rate, bit_depth=bd,
                                lfe_rate=rate if lfe else 0)
        z = O.render(omx, x, oc)
        if limiter:
            z, _ = O.limiter_run(z, [fs] * (x.shape[1] // fs), thr_db=thr, rate=rate)
        return np.ascontiguousarray(z.T)


def expected_tally(inst, m, n_calls, flushes=1):
    e = {inst: n_calls}
    if flushes:
        e[R.gen(m)] = e.get(R.gen(m), 0) + flushes
    return e


def run_family(inst, m, oc, progs, fs=FS, calls=CALLS, bd=16, limiter=True, thr=-1.0, rate=48000, mfma=False, table=False,
               lfe=False, env=None):
    """progs [(name, x [m][n])], one per stream, through one matrix-rendered batch"""
    A, G, O = _mods()
    fmt = {16: A.FMT_S16, 24: A.FMT_S24, 32: A.FMT_S32, -32: A.FMT_F32}[bd]
    if table:
        mx, omx = R.matrices(m, oc)
        assert mx.kind != A.KIND_M2M or mx.in_id != 0, "no table matrix for this pair"
    elif lfe:
        mx, omx = selection(m, oc, A.KIND_H2M, oc, lfe1=3)
    else:
        mx, omx = selection(m, oc)
    x = np.stack([p[1] for p in progs])
    assert x.shape[1] == m and x.shape[2] == fs * sum(calls)
    with R.environment(env or {}):
        A.route_reset()
        got = G.hip_render(mx, oc, x, frame_size=fs, fmt=fmt, limiter=limiter, flush=True, frames_per_call=calls,
                           threshold_db=thr, sample_rate=rate, projection=A.PROJ_MFMA if mfma else A.PROJ_EXACT, lfe_hoa=lfe)
        tally = A.route_tally()
    R.check_tally(tally, expected_tally(inst, m, len(calls), 1 if limiter else 0))
    bad = []
    for s, (name, xs) in enumerate(progs):
        d = mismatch(got[s], oracle_stream(O, omx, oc, xs, fs, bd, limiter, thr, rate, lfe), 1 if mfma else 0)
        if d:
            bad.append("%s: %s" % (name, d))
    assert not bad, "\n".join(["%s, %d bit:" % (inst, bd)] + bad)


# ------------------------------------------------------------------------------------------
# FAST
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oc", [2, 1])
def test_fast_limiter_programmes(oc):
    run_family(("FAST", 0, 2, oc, 0), 2, oc, limiter_set(2))


@pytest.mark.parametrize("rate", [44100, 16000, 96000])
def test_fast_release_to_idle_at_other_rates(rate):
    frames = P.RELEASE_FRAMES[rate]
    run_family(("FAST", 0, 2, 2, 0), 2, 2, some(2, ["release_to_idle", "silence", "onset_after_silence"], FS * frames, rate),
               calls=CALLS_BY_FRAMES[frames], rate=rate)


@pytest.mark.parametrize("bd", [16, 24, 32, -32])
def test_fast_pack_edges(bd):
    run_family(("FAST", 0, 2, 2, 0), 2, 2, some(2, ["pack_edges", "denormal", "loud"]), bd=bd, thr=60.0)


def test_fast_table_matrix():
    run_family(("FAST", 0, 2, 2, 0), 2, 2, some(2, ["silence", "release_to_idle", "loud"]), table=True)


def second_pairs(m, n=N, rate=48000):
    """a one-channel second element mixed in: silent beside a release, a release beside silence, a release beside an onset"""
    return [("release_to_idle + silence", P.release_to_idle(m, n, rate), P.silence(1, n, rate)),
            ("silence + release_to_idle", P.silence(m, n, rate), P.release_to_idle(1, n, rate)),
            ("onset_after_silence + release_to_idle", P.onset_after_silence(m, n, rate), P.release_to_idle(1, n, rate))]


def run_second(inst, m, oc, pairs=None, calls=CALLS, rate=48000):
    """pairs [(name, x [m][n], x2 [1][n])]: the second element mixed in, one pair per stream (default: second_pairs)"""
    import torch
    A, G, O = _mods()
    pairs = pairs or second_pairs(m)
    N = pairs[0][1].shape[1]
    assert N == FS * sum(calls)
    (mx, omx), (mx2, omx2) = selection(m, oc), selection(1, oc)
    x, x2 = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
    A.route_reset()
    b = A.Batch(len(pairs), mx, oc, frame_size=FS, out_format=A.FMT_S16, projection=A.PROJ_EXACT, sample_rate=rate)
    b.set_second_element(mx2, [1.0] * len(pairs))
    got = G.run_ex(A, G, torch, b, len(pairs), m, x, FS, oc, A.FMT_S16, x2=x2, m2=1, calls=list(calls))
    b.close()
    R.check_tally(A.route_tally(), expected_tally(inst, m, len(calls)))
    bad = []
    for s, (name, xs, xs2) in enumerate(pairs):
        y0, y1 = O.render(omx, xs, oc), O.render(omx2, xs2, oc)
        z = ((np.zeros_like(y0) + y0) + y1).astype(np.float32)
        z, _ = O.limiter_run(z, [FS] * (N // FS), rate=rate)
        d = mismatch(got[s], O.pack(z, 16))
        if d:
            bad.append("%s: %s" % (name, d))
    assert not bad, "\n".join([str(inst)] + bad)


def test_fast_second_element():
    run_second(("FAST", 1, 2, 2, 0), 2, 2)


def run_down(inst, m, oc, names, N=N, calls=CALLS, rate=48000):
    """the parametric down-mixer in front of the limiter (route_cases.run_down's schedule of modes and offsets); names: the
    programmes (or (name, x [m][N]) pairs), one per stream"""
    import torch
    A, G, O = _mods()
    progs = [(nm, getattr(P, nm)(m, N, rate)) if isinstance(nm, str) else nm for nm in names]
    names = [p[0] for p in progs]
    assert N == FS * sum(calls)
    L = A.lib()
    il, ol = R._DOWN_PAIR[(m, oc)]
    assert L.iamf_hip_dmx_valid(il, ol) == 1
    F, S = N // FS, len(names)
    sched = [((-1, 1, 2, 4, 5, 6, 0, 2)[f % 8], (0, 0, 37, 128, 0, FS - 3, 4, 0)[f % 8]) for f in range(F)]
    x = np.stack([np.ascontiguousarray(xs.reshape(m, F, FS).transpose(1, 0, 2)) for _, xs in progs])
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
        d = torch.from_numpy(rec[:, f0:f0 + nf].copy()).cuda()
        a.d_dmx_frames = d.data_ptr()
        return d

    A.route_reset()
    b = A.Batch(S, A.dmx_matrix(il, ol), oc, frame_size=FS, out_format=A.FMT_S16, limiter=True, sample_rate=rate)
    got = R._ex_loop(A, b, x, extra, list(calls), oc)
    b.close()
    R.check_tally(A.route_tally(), expected_tally(inst, m, len(calls)))
    bad = []
    for s, nm in enumerate(names):
        with np.errstate(all="ignore"):
            y = O.downmix_run(il, ol, x[s], sched, 1, 3)
            z, _ = O.limiter_run(np.ascontiguousarray(y.transpose(1, 0, 2).reshape(oc, N)), [FS] * F, rate=rate)
        d = mismatch(got[s], O.pack(z, 16))
        if d:
            bad.append("%s: %s" % (nm, d))
    assert not bad, "\n".join([str(inst)] + bad)


def test_fast_down():
    run_down(("FAST_DOWN", 0, 6, 2, 0), 6, 2, ["silence", "release_to_idle", "loud_then_silence"])


# ------------------------------------------------------------------------------------------
# LPCM packets
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("early", [1, 0])
def test_lpcm_packets(early):
    """all-zero packets; alternating +32767 / -32768; a full-scale burst, then zeros"""
    import lpcm_util as LP
    A, G, O = _mods()
    m, oc, F = 4, 2, N // FS
    ints = np.zeros((3, F, m, FS), dtype=np.int64)
    ints[1] = np.where(np.arange(FS) % 2 == 0, 32767, -32768)[None, None, :]
    ints[2, 0, :, 100:340] = np.where(np.arange(240) % 2 == 0, 32767, -32768)[None, :]
    perm = [2, 0, 3, 1]
    x = (ints[:, :, perm, :].astype(np.float64) / 32768.0).astype(np.float32)
    planar = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(3, m, N)
    mx, omx = selection(m, oc)
    raw, L, row = LP.rows(ints, 2, True, [1] * m, perm, head=16, pad=0, frame_size=FS)
    with R.environment({} if early else {"IAMF_HIP_LP_LATE": "1"}):
        A.route_reset()
        got = LP.render_lpcm(mx, oc, raw, L, row, FS, list(CALLS))
        tally = A.route_tally()
    R.check_tally(tally, expected_tally(("LPCM", early, m, oc, 0), m, len(CALLS)))
    bad = []
    for s, nm in enumerate(["zero packets", "alternating full scale", "burst then zeros"]):
        d = mismatch(got[s].view(np.int16).reshape(-1, oc), O.stream_run(omx, oc, planar[s], FS))
        if d:
            bad.append("%s: %s" % (nm, d))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------
# FANOUT
# ------------------------------------------------------------------------------------------

def test_fanout_limiter_programmes():
    """one element into a stereo and a mono batch in one launch; each member against its own oracle run"""
    run_fanout(4, [2, 1], limiter_set(4))


def run_fanout(m, ocs, progs, calls=CALLS, rate=48000, thr=-1.0, fused=True):
    """progs [(name, x [m][n])], one per stream, into len(ocs) members of ocs[j] channels in one launch per call; fused: whether
    the members' calls are expected in the shared kernel (else each is rendered singly, by the general kernel)"""
    import torch
    A, G, O = _mods()
    K = len(ocs)
    N = progs[0][1].shape[1]
    assert N == FS * sum(calls)
    S, F = len(progs), N // FS
    mxs = [selection(m, oc) for oc in ocs]
    x = np.stack([p[1] for p in progs])
    xin = torch.from_numpy(G.to_frames(x, FS)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    batches = [A.Batch(S, mxs[j][0], ocs[j], frame_size=FS, projection=A.PROJ_EXACT, sample_rate=rate, threshold_db=thr)
               for j in range(K)]
    outs = [[[] for _ in range(S)] for _ in range(K)]

    def take(j, pcm, n):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[j][s].append(h[s][:n * ocs[j] * 2].view(np.int16).reshape(n, ocs[j]).copy())

    A.route_reset()
    f0 = 0
    for nf in calls:
        caps = [(nf * FS * oc * 2 + 15) & ~15 for oc in ocs]
        pcms = [torch.zeros((S, cap), dtype=torch.uint8, device="cuda") for cap in caps]
        n_emitted, n_fused = A.render_fanout(batches, xin.data_ptr() + 4 * f0 * m * FS, F * m * FS, m * FS, nf,
                                             [p.data_ptr() for p in pcms], caps, st)
        assert n_fused == (K if fused else 0), n_fused
        for j in range(K):
            take(j, pcms[j], n_emitted[j])
        f0 += nf
    for j, b in enumerate(batches):
        cap = 240 * ocs[j] * 2
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        take(j, pcm, b.flush(pcm.data_ptr(), cap, st))
        b.close()
    if fused:
        R.check_tally(A.route_tally(), expected_tally(("FANOUT", 0, m, 0, K), m, len(calls), flushes=K))
    else:
        R.check_tally(A.route_tally(), {R.gen(m): K * (len(calls) + 1)})
    bad = []
    for j in range(K):
        for s, (name, xs) in enumerate(progs):
            d = mismatch(np.concatenate(outs[j][s]), oracle_stream(O, mxs[j][1], ocs[j], xs, FS, 16, thr=thr, rate=rate))
            if d:
                bad.append("member %d (%d ch), %s: %s" % (j, ocs[j], name, d))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------
# WIDE4 and its variants
# ------------------------------------------------------------------------------------------

def test_wide4_limiter_programmes():
    run_family(("WIDE4", 0, 6, 6, 0), 6, 6, limiter_set(6))


def test_wide4_pack_edges():
    run_family(("WIDE4", 0, 6, 6, 0), 6, 6, some(6, ["pack_edges", "denormal", "loud"]), thr=60.0)


def test_wide4_table_matrix():
    run_family(("WIDE4", 0, 6, 6, 0), 6, 6, some(6, ["silence", "release_to_idle", "loud"]), table=True)


def test_wide4_second_element():
    run_second(("WIDE4_MIX", 0, 6, 6, 0), 6, 6)


def test_wide4_down():
    run_down(("WIDE4_DOWN", 0, 12, 10, 0), 12, 10, ["silence", "onset_after_silence", "release_to_idle"])


def test_wide4_lfe():
    run_family(("WIDE4_LFE", 0, 4, 6, 0), 4, 6, some(4, ["silence", "onset_after_silence", "release_to_idle"]), lfe=True)


@pytest.mark.parametrize("fs", [1024, 256])
def test_wide4_demixer_programmes(fs):
    """the eight demixer programmes as the decoded layers of stereo -> 5.1.2 -> 7.1.4 on render_wide4_kernel<.., DMX>, and the
    same calls on the generic kernel.  Waves with a numerator of 0, below 2^-100 or from 2^126 take the quotients' IEEE
    branch; what this pins is that branch's RESULT — on the normal numerators that share such a wave (dm_gap, dm_mixed)
    and on the huge ones (dm_huge) — not which branch ran: behind the limiter and the 16-bit pack a signed zero or one ulp
    of 1e-33 is the same sample either way."""
    import torch
    import demix_cases as D
    A, G, O = _mods()
    dc = P.demix_case(fs)
    m = oc = len(dc["order"])
    F, S = len(dc["schedule"]), len(P.DEMIXER)
    calls = [1, 2, 1] if fs == 1024 else [4, 4]
    mx, omx = selection(m, oc)
    x = np.stack([P.demix_input(f, dc) for f in P.DEMIXER])                  # [S][F][m][fs]
    rec = np.frombuffer(bytes(R.demix_frames(A, dc, S)), dtype=np.uint8).reshape(S, F, -1)

    def extra(a, f0, nf):
        d = torch.from_numpy(rec[:, f0:f0 + nf].copy()).cuda()
        a.d_demix_frames = d.data_ptr()
        return d

    want = []
    with np.errstate(all="ignore"):
        for s in range(S):
            dem = D.drive_demixer(O.lib(), "orc_demixer_", dc, x[s])
            want.append(O.stream_run(omx, oc, np.ascontiguousarray(dem.transpose(1, 0, 2).reshape(m, F * fs)), fs))
    bad = []
    for env, inst in (({}, ("WIDE4_DEMIX", 0, m, oc, 0)), ({"IAMF_HIP_NO_WIDE4": "1"}, R.gen(m))):
        with R.environment(env):
            A.route_reset()
            b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16, limiter=True, projection=A.PROJ_EXACT)
            b.set_demixer(dc["layout"], dc["order"], dc["gains"], dc["offset"])
            got = R._ex_loop(A, b, x, extra, list(calls), oc)
            b.close()
            tally = A.route_tally()
        R.check_tally(tally, expected_tally(inst, m, len(calls)))
        for s, f in enumerate(P.DEMIXER):
            d = mismatch(got[s], want[s])
            if d:
                bad.append("%s, %s: %s" % (inst[0], f.__name__, d))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------
# WIDE, GENERIC, NOLIM
# ------------------------------------------------------------------------------------------

WIDE_CALLS = [1, 2, 3, 40, 2]     # 48 frames of 256


def test_wide_limiter_programmes():
    run_family(("WIDE", 0, 12, 0, 0), 12, 11, limiter_set(12), fs=256, calls=WIDE_CALLS)


@pytest.mark.parametrize("bd", [16, 24, 32])
def test_wide_pack_edges(bd):
    run_family(("WIDE", 0, 12, 0, 0), 12, 11, some(12, ["pack_edges", "denormal", "loud"]), fs=256, calls=WIDE_CALLS, bd=bd, thr=60.0)


def test_wide_table_matrix():
    run_family(("WIDE", 0, 12, 0, 0), 12, 11, some(12, ["silence", "release_to_idle", "loud"]), fs=256, calls=WIDE_CALLS, table=True)


def test_generic_limiter_programmes():
    """1000-sample frames: every call is ragged, and every other kernel refuses it"""
    calls = [1, 3, 2, 5, 2]
    run_family(R.gen(2), 2, 2, limiter_set(2, 13000), fs=1000, calls=calls)


def test_generic_table_matrix():
    run_family(R.gen(2), 2, 2, some(2, ["silence", "release_to_idle", "loud"], 13000), fs=1000, calls=[1, 3, 2, 5, 2], table=True)


@pytest.mark.parametrize("bd", [16, 24, 32, -32])
@pytest.mark.parametrize("m,oc", [(2, 4), (12, 12)])
def test_nolim_pack_edges_and_off_scale(m, oc, bd):
    run_family(("NOLIM", 0, m, 0, 0), m, oc, some(m, ["pack_edges", "denormal", "loud", "nonfinite"]), bd=bd, limiter=False)


# ------------------------------------------------------------------------------------------
# MFMA projections: 1 LSB by design, so no tie, denormal or non-finite programme
# ------------------------------------------------------------------------------------------

MFMA_SET = ["silence", "release_to_idle", "square_full_scale"]


def test_wide4_mfma():
    run_family(("WIDE4", 1, 6, 6, 0), 6, 6, some(6, MFMA_SET), mfma=True)


def test_wide_mfma():
    run_family(("WIDE", 1, 12, 0, 0), 12, 11, some(12, MFMA_SET), fs=256, calls=WIDE_CALLS, mfma=True)
