"""The rig of the per-stream lifecycle tests (tests/test_gpu_lifecycle.py, tests/test_gpu_long_positions.py): one batch, its
input tensor indexed by the stream's slot and a wall-clock frame, and the PCM every slot emitted in its current life.
Nothing here needs a GPU until a Rig is made."""
import numpy as np

import oracle_lib as O
import synth

UNIMPLEMENTED, BAD_ARG = -6, -1

# the kernels that keep state differently: render_fast, render_wide4, the LFE generator's filter state, the general
# kernel (a frame size that is no multiple of 64), render_nolim (position only)
CASES = {
    "fast": dict(src="TOA", out="BINAURAL", m=16, fs=1024),
    "wide4": dict(src="L714", out="J", m=12, fs=1024),
    "lfe": dict(src="TOA", out="B", m=16, fs=1024, lfe=True),
    "general": dict(src="STEREO", out="A", m=2, fs=1000),
    "nolim": dict(src="TOA", out="BINAURAL", m=16, fs=1024, limiter=False),
}


def hot(seed, m, frames, fs, cut_frames=2):
    """a programme with a burst across the sample `cut_frames * fs`: a stream cut off there has its limiter engaged and
    its rings full"""
    return synth.hot(seed, m, frames * fs, burst_phase=cut_frames * fs - 130 - seed % 23, burst_period=1500)


class Rig:
    """one batch, its input tensor [S][W wall-clock frames][m][fs] and the PCM every slot emitted in its current life"""

    def __init__(self, case, S, W, batch=None, m=None, fs=None, ch=None):
        import torch
        import iac_amd as A
        self.A, self.torch, self.S, self.W = A, torch, S, W
        if batch is None:
            c = CASES[case]
            self.m, self.fs, self.ch = c["m"], c["fs"], A.layout_channels(A.SS[c["out"]])
            self.limiter, self.lfe = c.get("limiter", True), c.get("lfe", False)
            if c["src"] == "TOA":
                mx, self.omx, proj = A.get_h2m_matrix(3, A.SS[c["out"]]), O.get_h2m(3, O.SS[c["out"]]), A.PROJ_EXACT
            else:
                mx, proj = A.get_m2m_matrix(A.SS[c["src"]], A.SS[c["out"]]), A.PROJ_AUTO
                self.omx = O.get_m2m(O.SS[c["src"]], O.SS[c["out"]])
            batch = A.Batch(S, mx, self.ch, frame_size=self.fs, out_format=A.FMT_S16, limiter=self.limiter, loudness=True,
                            projection=proj, lfe_hoa=self.lfe)
        else:
            self.m, self.fs, self.ch, self.limiter, self.lfe, self.omx = m, fs, ch, True, False, None
        self.b = batch
        self.xin = torch.zeros((S, W, self.m, self.fs), dtype=torch.float32, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        self.out = [[] for _ in range(S)]

    def put(self, s, wall, x):
        """programme x [m][n * fs] of slot s, its first frame at wall-clock frame `wall`"""
        F = x.shape[1] // self.fs
        assert x.shape[1] == F * self.fs and wall + F <= self.W
        fr = np.ascontiguousarray(x.reshape(self.m, F, self.fs).transpose(1, 0, 2))
        self.xin[s, wall:wall + F] = self.torch.from_numpy(fr).cuda()

    def _collect(self, pcm, n, s0, cnt):
        self.torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(self.S):
            if s0 <= s < s0 + cnt:
                self.out[s].append(h[s][:n * self.ch * 2].view(np.int16).reshape(n, self.ch).copy())
            else:
                assert not h[s].any(), "a stream outside the range was written"

    def render(self, wall, s0, cnt, nf, n_samples=0, skip=0):
        A, m, fs = self.A, self.m, self.fs
        cap = max(nf * fs, 240) * self.ch * 2
        pcm = self.torch.zeros((self.S, cap), dtype=self.torch.uint8, device="cuda")
        a = A.RenderArgs()
        a.d_in = self.xin.data_ptr() + 4 * (wall * m * fs + skip)
        a.in_stream_stride, a.in_frame_stride = self.W * m * fs, m * fs
        a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n_samples, pcm.data_ptr(), cap, self.st
        n = self.b.render_range(a, s0, cnt)
        self._collect(pcm, n, s0, cnt)

    def flush(self, s0, cnt):
        cap = 240 * self.ch * 2
        pcm = self.torch.zeros((self.S, cap), dtype=self.torch.uint8, device="cuda")
        n = self.b.flush_range(pcm.data_ptr(), cap, self.st, s0, cnt)
        self._collect(pcm, n, s0, cnt)

    def take(self, s):
        """the PCM of slot s's life so far; the slot starts a new list"""
        got, self.out[s] = np.concatenate(self.out[s], axis=0), []
        return got

    def want(self, x, gains=(1.0, 1.0, 1.0), flush=True):
        """the oracle: this programme alone, with these (element, output, loudness) gains"""
        return O.stream_run(self.omx, self.ch, np.ascontiguousarray(x), self.fs, flush=flush and self.limiter,
                            element_gain=gains[0], output_gain=gains[1], loudness_on=1, loudness_gain=gains[2],
                            limiter_on=1 if self.limiter else 0, lfe_rate=48000 if self.lfe else 0)

    def close(self):
        self.b.close()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), what


def new_gains(s):
    return (1.2 - 0.05 * s, 0.9 + 0.04 * s, 1.1 - 0.03 * s)


def gains_of(A, streams):
    g = [new_gains(s) for s in streams]
    return A.stream_gains(element=[v[0] for v in g], output=[v[1] for v in g], loudness=[v[2] for v in g])
