"""Helpers for the -m gpu tests: drive libiamf_hip.so through its C ABI with torch tensors as
plain device memory."""
import numpy as np
import torch

import iac_amd as A

_NP_OUT = {A.FMT_S16: np.int16, A.FMT_S32: np.int32, A.FMT_F32: np.float32, A.FMT_S24: np.uint8}


def to_frames(x, frame_size):
    """[S][m][total] planar -> [S][F][m][frame_size] (the ABI's input layout)"""
    S, m, total = x.shape
    assert total % frame_size == 0
    F = total // frame_size
    return np.ascontiguousarray(x.reshape(S, m, F, frame_size).transpose(0, 2, 1, 3))


def hip_render(matrix, out_ch, x, frame_size, fmt=A.FMT_S16, limiter=True, flush=True,
               frames_per_call=None, gains=None, loudness=False, threshold_db=-1.0,
               sample_rate=48000, projection=0, fir_taps=0, lfe_hoa=False):
    """x: numpy [S][m][total].  Returns a list (per stream) of arrays [n_out][out_ch] (S24:
    [n_out][out_ch][3] bytes) — everything the calls emitted, concatenated."""
    S, m, total = x.shape
    xin = torch.from_numpy(to_frames(x, frame_size)).cuda()
    F = total // frame_size
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    b = A.Batch(S, matrix, out_ch, frame_size=frame_size, sample_rate=sample_rate, out_format=fmt,
                limiter=limiter, threshold_db=threshold_db, loudness=loudness, projection=projection,
                fir_taps=fir_taps, lfe_hoa=lfe_hoa)
    if gains:
        b.set_gains(**gains)
    calls = frames_per_call or [F]
    assert sum(calls) == F
    stream_stride = F * m * frame_size
    frame_stride = m * frame_size
    outs = [[] for _ in range(S)]
    f0 = 0
    st = torch.cuda.current_stream().cuda_stream
    for nf in calls:
        cap = max(nf * frame_size, 240) * out_ch * bps
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        n = b.render(xin.data_ptr() + 4 * f0 * frame_stride, stream_stride, frame_stride, nf,
                     pcm.data_ptr(), cap, st)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(_view(h[s], n, out_ch, fmt))
        f0 += nf
    if flush:
        cap = 240 * out_ch * bps
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        n = b.flush(pcm.data_ptr(), cap, st)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(_view(h[s], n, out_ch, fmt))
    b.close()
    return [np.concatenate(o, axis=0) for o in outs]


def _view(raw, n, ch, fmt):
    if fmt == A.FMT_S24:
        return raw[:n * ch * 3].reshape(n, ch, 3).copy()
    dt = _NP_OUT[fmt]
    return raw[:n * ch * np.dtype(dt).itemsize].view(dt).reshape(n, ch).copy()


def identity_matrix(ch):
    """an M2M matrix that passes ch channels straight through (for limiter / pack stage tests)"""
    import ctypes as C
    eye = np.eye(ch, dtype=np.float32)
    m = A.Matrix()
    m.kind, m.in_id, m.out_id, m.channels, m.lfe1, m.lfe2, m.m, m.n = A.KIND_M2M, 0, 0, ch, -1, -1, ch, ch
    m.mat = eye.ctypes.data_as(C.POINTER(C.c_float))
    m._keep = eye
    return m


def run_ex(A, G, torch, batch, S, m, x, fs, out_ch, fmt, x2=None, m2=0, ramps=None, dmx_frames=None,
            calls=None, flush=True):
    """x: [S][m][total]; returns list of per-stream outputs"""
    total = x.shape[2]
    F = total // fs
    xin = torch.from_numpy(to_frames(x, fs)).cuda()
    xin2 = torch.from_numpy(to_frames(x2, fs)).cuda() if x2 is not None else None
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    d_ramps = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for k, v in (ramps or {}).items()}
    d_dmx = None
    if dmx_frames is not None:
        raw = np.frombuffer(bytes(dmx_frames), dtype=np.uint8).copy()
        d_dmx = torch.from_numpy(raw).cuda()
    outs = [[] for _ in range(S)]
    st = torch.cuda.current_stream().cuda_stream
    f0 = 0
    for nf in (calls or [F]):
        cap = max(nf * fs, 240) * out_ch * bps
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        a = A.RenderArgs()
        a.d_in = xin.data_ptr() + 4 * f0 * m * fs
        a.in_stream_stride, a.in_frame_stride = F * m * fs, m * fs
        if xin2 is not None:
            a.d_in2 = xin2.data_ptr() + 4 * f0 * m2 * fs
            a.in2_stream_stride, a.in2_frame_stride = F * m2 * fs, m2 * fs
        for key, field in (("element", "d_element_ramp"), ("element2", "d_element2_ramp"), ("output", "d_output_ramp")):
            if key in d_ramps:
                setattr(a, field, d_ramps[key].data_ptr() + 4 * f0 * fs)
        a.ramp_stream_stride = total
        if d_dmx is not None:
            assert calls is None  # one call: frames index from 0
            a.d_dmx_frames = d_dmx.data_ptr()
        a.n_frames = nf
        a.d_pcm = pcm.data_ptr()
        a.pcm_stream_stride_bytes = cap
        a.stream = st
        n = batch.render_ex(a)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(_view(h[s], n, out_ch, fmt))
        f0 += nf
    if flush:
        cap = 240 * out_ch * bps
        pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
        n = batch.flush(pcm.data_ptr(), cap, st)
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[s].append(_view(h[s], n, out_ch, fmt))
    return [np.concatenate(o, axis=0) for o in outs]
