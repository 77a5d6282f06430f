"""Shared by tests/test_gpu_fanout_lpcm.py, tests/route_cases_ext.py and tools/fanout_lpcm_rate.py: the members, the packet
programme and the driver of iamf_hip_batch_render_fanout_lpcm and its twins.  Nothing here needs a GPU until a Drive is made."""
import numpy as np

import iac_amd as A
import lpcm_util as LP

BPS = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}
FILL = 0xA5

ORDER = {"foa": 1, "soa": 2, "toa": 3}
CHANNELS = {"foa": 4, "soa": 9, "toa": 16}


def member(layout, fmt=A.FMT_S16, eg=1.0, og=1.0, lg=None, thr_db=-1.0, limiter=True, rate=48000):
    return dict(layout=layout, fmt=fmt, eg=eg, og=og, lg=lg, thr_db=thr_db, limiter=limiter, rate=rate)


# Clipped 16-bit input cannot drive a mono rendition of an ambisonics element above 0.7071 of full scale: the mono members'
# thresholds lie below that
A_S16 = member("A")
MONO_S16_M6 = member("MONO", thr_db=-6.0)
A_GAINS_S24 = member("A", fmt=A.FMT_S24, eg=0.9, og=1.1, lg=0.95)
MONO_S32_M9 = member("MONO", fmt=A.FMT_S32, thr_db=-9.0)
MEMBERS = [A_S16, MONO_S16_M6, A_GAINS_S24, MONO_S32_M9]


def gain_product(sp):
    g = 1.0
    for v in (sp["eg"], sp["og"], sp["lg"]):
        if v is not None:
            g *= v
    return g


def make_batch(mx, sp, S, fs):
    oc = A.layout_channels(A.SS[sp["layout"]])
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=sp["fmt"], limiter=sp["limiter"], threshold_db=sp["thr_db"], sample_rate=sp.get("rate", 48000),
                loudness=sp["lg"] is not None, projection=A.PROJ_EXACT if oc > 2 else A.PROJ_AUTO)
    b.set_gains(element=[sp["eg"]] * S, output=[sp["og"]] * S, loudness=None if sp["lg"] is None else [sp["lg"]] * S)
    b.oc, b.bps = oc, BPS[sp["fmt"]]
    return b


def ints16(S, F, m, fs, seed0=500, bps=2):
    """[S][F][m][fs] integer samples: even streams loud (lpcm_util.ints: Gaussian at 0.35 of full scale, every 97th sample
    x 3, clipped), odd streams quiet (level 0.02, no peaks); stream s from seed seed0 + s"""
    full = float(1 << (8 * bps - 1))
    out = np.zeros((S, F, m, fs), dtype=np.int64)
    for s in range(S):
        rng = np.random.default_rng(seed0 + s)
        if s % 2 == 0:
            out[s] = LP.ints(rng, 1, F, m, fs, bps)[0]
        else:
            out[s] = np.clip(np.rint(rng.standard_normal((F, m, fs)) * 0.02 * full), -full, full - 1).astype(np.int64)
    return out


def reversed_rows(ints, fs, bps=2, le=True):
    """packet rows with head 8, pad 8 and reversed channel order (perm[c] = m - 1 - c): every run offset differs and none
    ascend.  Returns (raw [S][F][row], layout, row bytes, x [S][m][F * fs] f32 = what the decoder would hand the renderer)"""
    S, F, m, _ = ints.shape
    perm = [m - 1 - c for c in range(m)]
    raw, L, row = LP.rows(ints, bps, le, [1] * m, perm, head=8, pad=8, frame_size=fs)
    x = decoded(ints, perm, bps)
    return raw, L, row, x


def decoded(ints, perm, bps=2):
    S, F, m, fs = ints.shape
    full = np.float32(1 << (8 * bps - 1))
    x = ints[:, :, perm, :].astype(np.float32) / full     # (16 and 24 bit: exact; 32 bit: int -> f32 rounds first, as the decoder)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)


class Drive:
    """K batches on one device buffer of packet rows.  Every step appends, per member and stream OF THE STEP'S RANGE, the
    bytes the step emitted; PCM rows outside the range must keep their fill."""

    def __init__(self, matrices, specs, raw, L, row, x, fs, packets=None, pcm_layout=None):
        """packets: a packet layout of gpu_util (place_packets) or None: the rows as they are, dense, at the start of a fresh
        allocation.  pcm_layout: the layout of every member's PCM rows (gpu_util.pcm_rows; None: DENSE)."""
        import torch
        import gpu_util as G
        self.torch, self.G = torch, G
        self.S, self.F, _ = raw.shape
        self.m, self.fs, self.L, self.row = L.channels, fs, L, row
        self.raw, self.packets, self.pcm_layout = raw, packets, pcm_layout or G.DENSE
        self.d_raw = torch.from_numpy(raw).cuda() if packets is None else None
        self.keep = None
        # the same samples as planar f32 frames (x None: a drive that makes no f32 call)
        self.xin = None if x is None else torch.from_numpy(G.to_frames(x, fs)).cuda()
        self.batches = [make_batch(mx, sp, self.S, fs) for mx, sp in zip(matrices, specs)]
        self.out = [[[] for _ in range(self.S)] for _ in specs]
        self.emitted = [[] for _ in specs]
        self.reports = []
        self.f0 = [0] * self.S
        self.st = torch.cuda.current_stream().cuda_stream

    def bufs(self, n_samples):
        """-> (the members' pcm_stream_stride_bytes, their PCM rows as torch tensors: S rows under the drive's PCM layout, every
        byte the fill; .rows is the gpu_util.PcmRows, whose d_pcm is the call's pointer — the tensor's own under DENSE)"""
        caps = [(max(n_samples, 240) * b.oc * b.bps + 15) & ~15 for b in self.batches]
        rows = self.G.pcm_rows_of_members(self.S, caps, self.pcm_layout, [b.bps for b in self.batches])
        pcms = []
        for r in rows:
            t = r.tensor[0:]     # a tensor of its own on the same memory (far rows share an allocation)
            t.rows = r
            pcms.append(t)
        return [r.stride for r in rows], pcms

    def _take(self, j, pcm, n, s0, cnt):
        """the emitted runs of the range; every other byte of the allocation must still be the fill (rows_and_rest)"""
        self.torch.cuda.synchronize()
        b = self.batches[j]
        h = self.G.rows_and_rest(pcm.rows, self.pcm_layout, n * b.oc * b.bps, only=(s0, cnt))
        for s in range(s0, s0 + cnt):
            self.out[j][s].append(h[s])
        self.emitted[j].append(n)

    def _range(self, s0, cnt):
        cnt = self.S - s0 if cnt is None else cnt
        f0 = self.f0[s0]
        return cnt, f0

    def lpcm_input(self, f0, first=0):
        inp = A.LpcmInput()
        if self.packets is None:
            inp.d_raw = self.d_raw.data_ptr() + f0 * self.row
            inp.raw_stream_stride = self.F * self.row
            inp.raw_frame_stride = self.row
        else:
            pl = self.G.place_packets(self.raw, self.L, self.packets, f0, keep=self.keep)
            self.keep = pl.keep
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = pl.d_raw, pl.stream_stride, pl.frame_stride
        inp.first_sample = first
        inp.layout = self.L
        return inp

    def _advance(self, s0, cnt, nf):
        for s in range(s0, s0 + cnt):
            self.f0[s] += nf

    def fan(self, nf, first=0, n_samples=0, s0=0, cnt=None):
        """the call under test; returns its report (n_fused, input_fused, n_unpacks)"""
        cnt, f0 = self._range(s0, cnt)
        caps, pcms = self.bufs(n_samples or nf * self.fs)
        ns, rep = A.render_fanout_lpcm(self.batches, self.lpcm_input(f0, first), nf, [p.rows.d_pcm for p in pcms], caps, self.st,
                                       n_samples=n_samples, stream0=s0, n_streams=cnt)
        for j, n in enumerate(ns):
            self._take(j, pcms[j], n, s0, cnt)
        self.reports.append(rep)
        self._advance(s0, cnt, nf)
        return rep

    def single(self, nf, first=0, n_samples=0, s0=0, cnt=None):
        """iamf_hip_batch_render_lpcm_range per member: the twin's path"""
        cnt, f0 = self._range(s0, cnt)
        caps, pcms = self.bufs(n_samples or nf * self.fs)
        inp = self.lpcm_input(f0, first)
        for j, b in enumerate(self.batches):
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n_samples, pcms[j].rows.d_pcm, caps[j], self.st
            self._take(j, pcms[j], b.render_lpcm_range(inp, a, s0, cnt), s0, cnt)
        self._advance(s0, cnt, nf)

    def _f32(self, f0):
        return self.xin.data_ptr() + 4 * f0 * self.m * self.fs, self.F * self.m * self.fs, self.m * self.fs

    def fan_f32(self, nf, s0=0, cnt=None):
        """iamf_hip_batch_render_fanout_range on the same samples as f32; returns n_fused"""
        cnt, f0 = self._range(s0, cnt)
        caps, pcms = self.bufs(nf * self.fs)
        d_in, ss, fstr = self._f32(f0)
        ns, fused = A.render_fanout_range(self.batches, d_in, ss, fstr, nf, [p.rows.d_pcm for p in pcms], caps, s0, cnt, self.st)
        for j, n in enumerate(ns):
            self._take(j, pcms[j], n, s0, cnt)
        self._advance(s0, cnt, nf)
        return fused

    def single_f32(self, nf, s0=0, cnt=None):
        """iamf_hip_batch_render_range per member on the same samples as f32"""
        cnt, f0 = self._range(s0, cnt)
        caps, pcms = self.bufs(nf * self.fs)
        d_in, ss, fstr = self._f32(f0)
        for j, b in enumerate(self.batches):
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = d_in, ss, fstr
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcms[j].rows.d_pcm, caps[j], self.st
            self._take(j, pcms[j], b.render_range(a, s0, cnt), s0, cnt)
        self._advance(s0, cnt, nf)

    def flush(self, s0=0, cnt=None):
        cnt, _ = self._range(s0, cnt)
        caps, pcms = self.bufs(240)
        for j, b in enumerate(self.batches):
            self._take(j, pcms[j], b.flush_range(pcms[j].rows.d_pcm, caps[j], self.st, s0, cnt), s0, cnt)

    def close(self):
        for b in self.batches:
            b.close()
        self.d_raw = self.keep = self.xin = None     # the far layouts hold gigabytes

    def bytes_of(self, j, s):
        return np.concatenate(self.out[j][s])


def assert_same(got, want, what=""):
    assert got.emitted == want.emitted, (what, got.emitted, want.emitted)
    for j in range(len(got.batches)):
        for s in range(got.S):
            assert len(got.out[j][s]) == len(want.out[j][s]), (what, j, s)
            for i, (a, b) in enumerate(zip(got.out[j][s], want.out[j][s])):
                assert np.array_equal(a, b), "%s member %d stream %d step %d differs from the twin" % (what, j, s, i)
