"""Long-lived streams: the shifts, the programmes and the oracle side of tests/test_gpu_long_positions.py, shared with
tests/test_long_positions_cpu.py.  Nothing here needs a GPU.

A stream exported at position P and imported with cursor[0] = P + D must continue bit for bit as it would have at P: the
limiter, the mixers and the pack code do not depend on time, and the saved rings are the last kSave samples relative to
the position.  Every family renders HEAD samples on a source batch, moves to a fresh batch at Q = P + D and renders
calls of one, two and one frames (of 1024; four times as many of 256) and the flush there.

The shifts.  EDGE is the stream sample (counted from the stream's first kept sample, as the oracle counts) that lands
on the boundary B = D + EDGE; it lies 1536 samples behind the export of an untrimmed stream, inside the two-frame call
and off that call's 1024-sample chunks:

  name         D                       D % 512, D % 1280    boundary
  across_2^31  2^31 - 3584             0, 1024              2^31 at sample 3584
  across_2^32  2^32 - 3584 - 48        464, 464             2^32 at sample 3632
  at_2^40      2^40 + 1024             0, 0                 none: only high bits set
  odd          2^31 - 3584 + 1         the general kernel only: the stream leaves the 16-sample grid with the import

The programme: synth.hot with a burst of 240 samples at 1.5 every 1536 samples, the three streams 30 samples apart, so
that a burst lies across sample 2048 (the export) and one across 3584 and 3632 (the boundaries) in every stream.  The
matrices are selection matrices (each output copies one input), so the rendered signal is the programme."""
import ctypes as C

import numpy as np

import route_cases as R
import synth

S = 3
HEAD = 2048
EDGE = 3584
B31, B32, B40 = 1 << 31, 1 << 32, 1 << 40
# (name, D, the stream sample on the boundary or None)
SHIFTS = [("across_2^31", B31 - EDGE, EDGE), ("across_2^32", B32 - EDGE - 48, EDGE + 48), ("at_2^40", B40 + 1024, None)]
ODD = ("odd", B31 - EDGE + 1, EDGE - 1)
assert all(d % 16 == 0 for _, d, _ in SHIFTS)
assert SHIFTS[1][1] % 512 and SHIFTS[1][1] % 1280 and SHIFTS[2][1] % 512 == 0 and SHIFTS[2][1] % 1280 == 0
assert SHIFTS[0][1] + EDGE == B31 and SHIFTS[1][1] + EDGE + 48 == B32 and ODD[1] + EDGE - 1 == B31

BURST_PERIOD, BURST_PHASE = 1536, EDGE - 120 - 2 * 1536


def programme(seed, m, n, sigma=0.22):
    """[S][m][n]: bursts across the samples 2048, 3584 and 3632 of every stream"""
    return np.stack([synth.hot(seed + 7 * s, m, n, sigma=sigma, burst_phase=BURST_PHASE - 30 + 30 * s, burst_period=BURST_PERIOD)
                     for s in range(S)])


def selection(m, oc, lfe=False):
    """(product matrix, oracle matrix): output o copies input o % m (lfe: an ambisonics matrix whose slot 3 is the LFE)"""
    import iac_amd as A
    import oracle_lib as O
    if lfe:
        n = oc - 1
        w = np.zeros((n, m), dtype=np.float32)
        w[np.arange(n), np.arange(n) % m] = 1.0
        return R._custom(A, O, A.KIND_H2M, m, n, w, oc, 3)
    w = np.zeros((m, oc), dtype=np.float32)
    w[np.arange(oc) % m, np.arange(oc)] = 1.0
    return R._custom(A, O, A.KIND_M2M, m, oc, w, oc)


class Family:
    """one case of the table in tests/test_gpu_long_positions.py.  kind: "plain" (one matrix-rendered element), "mix" (a
    one-channel second element, ramp: an output ramp as well), "down" (the parametric down-mixer), "demix", "lpcm" (packets
    of `bytes` bytes per sample), "fan" / "fan_lpcm" (K = 2: stereo and mono).  x is [S][m][n] in stream samples; a trimmed
    family feeds `trim` more samples in front of them."""

    def __init__(self, fid, inst, kind, m, oc, fs=1024, bd=16, limiter=True, mfma=False, lfe=False, ramp=False, trim=0,
                 bytes=0, env=None, odd=False, table=0):
        self.id, self.inst, self.kind, self.m, self.oc, self.fs, self.bd = fid, inst, kind, m, oc, fs, bd
        self.limiter, self.mfma, self.lfe, self.ramp, self.trim, self.bytes = limiter, mfma, lfe, ramp, trim, bytes
        self.env, self.table = env or {}, table
        self.shifts = SHIFTS + ([ODD] if odd else [])
        scale = 1024 // fs if fs == 256 else 1
        self.head_frames, self.calls = 2 * scale, [scale, 2 * scale, scale]
        self.frames = self.head_frames + sum(self.calls)
        self.n = self.frames * fs - trim                  # stream samples
        self.pos = self.head_frames * fs - trim           # P: where the source stands when it is exported
        self.ocs = [2, 1] if kind in ("fan", "fan_lpcm") else [oc]
        self._made = False

    # ---- the programme and the matrices ----
    def make(self):
        if self._made:
            return self
        import iac_amd as A
        import oracle_lib as O
        self._made = True
        m, fs, n, seed = self.m, self.fs, self.n, 4000 + 13 * sum(map(ord, self.id))
        self.lead = synth.gaussian(seed + 1, m, self.trim, 0.3) if self.trim else np.zeros((m, 0), dtype=np.float32)
        x = programme(seed, m, n)
        if self.bytes:      # packets: the programme as integers, full-scale bursts; what the decoder hands on is exact
            full = float(1 << (8 * self.bytes - 1))
            self.ints = np.clip(np.rint(x.astype(np.float64) * 0.65 * full), -full, full - 1).astype(np.int64)
            x = (self.ints.astype(np.float64) / full).astype(np.float32)
            self.perm = [2, 0, 3, 1]
        self.x = x
        self.mxs = [selection(m, oc, self.lfe) for oc in self.ocs]
        if self.kind == "mix":
            self.mx2 = selection(1, self.oc)
            self.x2 = np.stack([synth.hot(seed + 50 + s, 1, n, sigma=0.3, burst_phase=900, burst_period=1700) for s in range(S)])
            rng = np.random.default_rng(seed + 3)
            self.out_ramp = (0.7 + 0.4 * rng.random((S, n))).astype(np.float32) if self.ramp else None
        if self.kind == "down":
            self.il, self.ol = R._DOWN_PAIR[(m, self.oc)]
            F = self.frames
            self.sched = [((-1, 1, 2, 4, 5, 6, 0, 2)[f % 8], (0, 0, 37, 128, 0, fs - 3, 4, 0)[f % 8]) for f in range(F)]
            L = A.lib()
            assert L.iamf_hip_dmx_valid(self.il, self.ol) == 1
            frames = (A.DmxFrame * (S * F))()
            stt = A.DmxState()
            for s in range(S):
                L.iamf_hip_dmx_state_init(C.byref(stt))
                L.iamf_hip_dmx_set_mode_weight(C.byref(stt), 1, 3)
                for f, (mode, off) in enumerate(self.sched):
                    fr = frames[s * F + f]
                    fr.offset = off
                    L.iamf_hip_dmx_coefficients(C.byref(stt), fr.prev)
                    if mode > -1:
                        L.iamf_hip_dmx_set_mode_weight(C.byref(stt), mode, -1)
                    L.iamf_hip_dmx_coefficients(C.byref(stt), fr.cur)
            self.records = np.frombuffer(bytes(frames), dtype=np.uint8).reshape(S, F, -1).copy()
        if self.kind == "demix":
            import demix_cases as D
            import programmes as P
            dc = dict(P.demix_case(fs))
            dc["schedule"] = D._sched(len(dc["recon"]), dc["seed"])[:self.frames]     # the same schedule, two frames longer
            assert len(dc["order"]) == m and dc["schedule"][:4] == P.demix_case(fs)["schedule"]
            self.dc = dc
            self.records = np.frombuffer(bytes(R.demix_frames(A, dc, S)), dtype=np.uint8).reshape(S, self.frames, -1).copy()
        return self

    def frames_of(self, x, lead=None):
        """[S][m][n] stream samples (+ the trimmed lead) -> [S][F][m][fs]"""
        lead = self.lead if lead is None else lead
        full = np.concatenate([np.broadcast_to(lead[None], (S,) + lead.shape), x], axis=2)
        return np.ascontiguousarray(full.reshape(S, x.shape[1], self.frames, self.fs).transpose(0, 2, 1, 3))

    # ---- the oracle ----
    def limiter_input(self, s, j=0):
        """[oc][n]: what the limiter of member j is fed, by the oracle's stages"""
        import oracle_lib as O
        self.make()
        omx, oc, x = self.mxs[j][1], self.ocs[j], self.x[s]
        if self.kind == "down":
            xf = self.frames_of(self.x)[s]
            y = O.downmix_run(self.il, self.ol, xf, self.sched, 1, 3)
            return np.ascontiguousarray(y.transpose(1, 0, 2).reshape(oc, self.n))
        if self.kind == "demix":
            import demix_cases as D
            dem = D.drive_demixer(O.lib(), "orc_demixer_", self.dc, self.frames_of(self.x)[s])
            x = np.ascontiguousarray(dem.transpose(1, 0, 2).reshape(self.m, self.n))
            self._demixed = getattr(self, "_demixed", {})
            self._demixed[s] = x
        if self.lfe:
            return O.render_h2m_lfe(omx, x, oc, 48000, [self.n])
        y = O.render(omx, x, oc)
        if self.kind == "mix":
            y1 = O.render(self.mx2[1], self.x2[s], oc)
            y = ((np.zeros_like(y) + y) + y1).astype(np.float32)
            if self.out_ramp is not None:
                y = (y * self.out_ramp[s][None, :]).astype(np.float32)
        return np.ascontiguousarray(y)

    def want(self, s, j=0):
        """the oracle's PCM of stream s (member j) for the whole programme: [n_out][oc] (s24: [n_out][oc][3])"""
        import oracle_lib as O
        self.make()
        omx, oc, fs = self.mxs[j][1], self.ocs[j], self.fs
        if self.kind in ("mix", "down"):
            z, _ = O.limiter_run(self.limiter_input(s, j), [fs] * self.frames)
            return O.pack(z, self.bd)
        x = self.x[s]
        if self.kind == "demix":
            self.limiter_input(s)
            x = self._demixed[s]
        if self.bd == -32:
            assert not self.limiter
            return np.ascontiguousarray(O.render(omx, x, oc).T)
        return O.stream_run(omx, oc, x, fs, flush=self.limiter, limiter_on=int(self.limiter), bit_depth=self.bd,
                            lfe_rate=48000 if self.lfe else 0)


def _families():
    F = Family
    late, early = {"IAMF_HIP_LP_LATE": "1"}, {"IAMF_HIP_LP_EARLY": "1"}
    return [
        F("fast_m2_oc2", ("FAST", 0, 2, 2, 0), "plain", 2, 2),
        F("fast_m2_oc1", ("FAST", 0, 2, 1, 0), "plain", 2, 1),
        F("fast_mix_ramp", ("FAST", 1, 2, 2, 0), "mix", 2, 2, ramp=True),
        F("fast_down_6_2", ("FAST_DOWN", 0, 6, 2, 0), "down", 6, 2),
        F("lpcm_early", ("LPCM", 1, 4, 2, 0), "lpcm", 4, 2, bytes=2),
        F("lpcm_late", ("LPCM", 0, 4, 2, 0), "lpcm", 4, 2, bytes=2, env=late),
        F("lpcm24_early", ("LPCM24", 1, 4, 2, 0), "lpcm", 4, 2, bytes=3, env=early, table=2),
        F("lpcm24_late", ("LPCM24", 0, 4, 2, 0), "lpcm", 4, 2, bytes=3, env=late, table=2),
        F("fanout_k2", ("FANOUT", 0, 4, 0, 2), "fan", 4, 2),
        F("fanout_lpcm_k2", ("FANOUT_LPCM", 0, 4, 0, 2), "fan_lpcm", 4, 2, bytes=2, table=1),
        F("wide4_6_6", ("WIDE4", 0, 6, 6, 0), "plain", 6, 6),
        F("wide4_mix", ("WIDE4_MIX", 0, 6, 6, 0), "mix", 6, 6),
        F("wide4_down_12_10", ("WIDE4_DOWN", 0, 12, 10, 0), "down", 12, 10),
        F("wide4_demix", ("WIDE4_DEMIX", 0, 12, 12, 0), "demix", 12, 12),
        F("wide4_lfe_4_6", ("WIDE4_LFE", 0, 4, 6, 0), "plain", 4, 6, lfe=True),
        F("wide_12_11", ("WIDE", 0, 12, 0, 0), "plain", 12, 11, fs=256),
        F("wide_12_11_s24", ("WIDE", 0, 12, 0, 0), "plain", 12, 11, fs=256, bd=24),
        F("generic_fs1000", R.gen(2), "plain", 2, 2, fs=1000, odd=True),
        F("nolim_2_4_s16", ("NOLIM", 0, 2, 0, 0), "plain", 2, 4, limiter=False),
        F("nolim_2_4_f32", ("NOLIM", 0, 2, 0, 0), "plain", 2, 4, limiter=False, bd=-32),
        F("wide4_mfma", ("WIDE4", 1, 6, 6, 0), "plain", 6, 6, mfma=True),
        F("wide_mfma", ("WIDE", 1, 12, 0, 0), "plain", 12, 11, fs=256, mfma=True),
        F("fast_off_grid", ("FAST", 0, 2, 2, 0), "plain", 2, 2, trim=237),
        F("wide4_off_grid", ("WIDE4", 0, 6, 6, 0), "plain", 6, 6, trim=237),
    ]


FAMILIES = _families()
BY_ID = {f.id: f for f in FAMILIES}
