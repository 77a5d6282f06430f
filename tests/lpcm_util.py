"""LPCM packet rows for iamf_hip_batch_render_lpcm and the loop that renders them (shared by tests/test_gpu_lpcm.py,
tests/test_gpu_lpcm24.py, tests/test_gpu_packet_layouts.py and tests/route_cases.py)."""
import numpy as np

import gpu_util as G
import iac_amd as A


def pack(v, bps, le):
    """int samples [..., n] -> bytes [..., n * bps] in the reference's byte orders (24-bit big-endian: bitstream.c:204-208:
    byte 1 is the top one, then byte 2, byte 0 is the low one)"""
    v = v.astype(np.int64)
    u = v & ((1 << (8 * bps)) - 1)
    b = [((u >> (8 * k)) & 0xff).astype(np.uint8) for k in range(bps)]   # b[0] = low byte
    if le:
        order = b
    elif bps == 3:
        order = [b[1], b[2], b[0]]   # reads24be: p[2] | p[0] << 8 | p[1] << 16
    else:
        order = b[::-1]
    return np.stack(order, axis=-1).reshape(v.shape[:-1] + (v.shape[-1] * bps,))


def rows(ints, bps, le, widths, perm, head, pad, frame_size):
    """ints [S][F][ch][fs] -> packet rows [S][F][row bytes] + layout.  Sub-stream j carries widths[j] channels (1 = mono
    packet, 2 = coupled: samples interleaved); perm[c] = the decoded channel output channel c takes."""
    S, F, ch, fs = ints.shape
    assert sum(widths) == ch and fs == frame_size
    off = head
    ch_off, ch_step = [], []
    pieces = []
    c = 0
    for w in widths:
        blk = ints[:, :, c:c + w, :]                       # [S][F][w][fs]
        inter = np.ascontiguousarray(blk.transpose(0, 1, 3, 2)).reshape(S, F, fs * w)
        pieces.append((off, pack(inter, bps, le)))
        for k in range(w):
            ch_off.append(off + k * bps)
            ch_step.append(w * bps)
        off += w * bps * fs + pad
        c += w
    row = (off + 15) & ~15
    raw = np.zeros((S, F, row), dtype=np.uint8)
    for o, data in pieces:
        raw[:, :, o:o + data.shape[-1]] = data
    L = A.LpcmLayout()
    L.sample_bytes, L.little_endian, L.channels, L.frame_size = bps, 1 if le else 0, ch, fs
    for p in range(ch):
        L.src_offset[p] = ch_off[perm[p]]
        L.src_step[p] = ch_step[perm[p]]
    return raw, L, row


def render_lpcm(matrix, out_ch, raw, L, row, frame_size, calls, first=0, n_samples=0, fmt=A.FMT_S16, layout=G.DENSE,
                packets=None, trims=None, emitted=None, refused=None, sample_rate=48000, threshold_db=-1.0):
    """sample_rate, threshold_db: the batch's (the limiter's step counts and threshold).  layout: of the PCM rows (gpu_util.pcm_rows).  packets: a packet layout of gpu_util (place_packets: the rows placed
    under it, every byte outside the runs the 0x7F / 0x80 fill); None: the rows as they are, dense, at the start of a fresh
    allocation.  trims: {call number: (first_sample, n_samples)} in place of first / n_samples for every call.  emitted:
    a list that receives what every call and the flush said it emitted.  refused: (packet layout, error code, frames) —
    before anything is rendered a call of that many frames is made under that packet layout and must be refused with that
    code, leaving its PCM rows and (as the result shows) the batch untouched."""
    S, F, _ = raw.shape
    import torch
    bps_out = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    st = torch.cuda.current_stream().cuda_stream
    outs = [[] for _ in range(S)]
    d_raw = keep = pcm = None
    b = A.Batch(S, matrix, out_ch, frame_size=frame_size, out_format=fmt, limiter=True, sample_rate=sample_rate,
                threshold_db=threshold_db)

    def packets_at(pk, f0, nf, keep):
        """-> (iamf_hip_lpcm_input of the call, what holds its memory)"""
        inp = A.LpcmInput()
        if pk is None:
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = d_raw.data_ptr() + f0 * row, F * row, row
        else:
            pl = G.place_packets(raw, L, pk, f0, nf, keep=keep)
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, keep = pl.d_raw, pl.stream_stride, pl.frame_stride, pl.keep
        inp.layout = L
        return inp, keep

    def call(inp, nf, trim):
        cap = max(nf * frame_size, 240) * out_ch * bps_out
        pcm, d_pcm, stride = G.pcm_rows(S, cap, layout, bps_out)
        inp.first_sample = trim[0]
        a = A.RenderArgs()
        a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, trim[1], d_pcm, stride, st
        return pcm, a

    try:
        if packets is None:
            d_raw = torch.from_numpy(raw).cuda()
        if refused:
            r_pk, code, nf = refused
            inp, r_keep = packets_at(r_pk, 0, nf, None)
            pcm, a = call(inp, nf, (0, 0))
            try:
                b.render_lpcm(inp, a)
                raise AssertionError("a call under %s was not refused" % r_pk.name)
            except A.IamfHipError as e:
                assert e.code == code, (r_pk.name, e.code, code)
            torch.cuda.synchronize()
            G.rows_and_rest(pcm, layout, 0)
            pcm = r_keep = None
        f0 = 0
        for k, nf in enumerate(calls):
            inp, keep = packets_at(packets, f0, nf, keep)
            pcm, a = call(inp, nf, (trims or {}).get(k, (first, n_samples)))
            n = b.render_lpcm(inp, a)
            torch.cuda.synchronize()
            h = G.rows_and_rest(pcm, layout, n * out_ch * bps_out)
            pcm = None
            for s in range(S):
                outs[s].append(h[s])
            if emitted is not None:
                emitted.append(n)
            f0 += nf
        cap = 240 * out_ch * bps_out
        pcm, d_pcm, stride = G.pcm_rows(S, cap, layout, bps_out)
        n = b.flush(d_pcm, stride, st)
        torch.cuda.synchronize()
        h = G.rows_and_rest(pcm, layout, n * out_ch * bps_out)
        for s in range(S):
            outs[s].append(h[s])
        if emitted is not None:
            emitted.append(n)
    finally:
        d_raw = keep = pcm = None     # the far layouts hold gigabytes
        b.close()
    return [np.concatenate(o) for o in outs]


def ints(rng, S, F, ch, fs, bps, level=0.35):
    full = float(1 << (8 * bps - 1))
    v = rng.standard_normal((S, F, ch, fs)) * level * full
    v[:, :, :, ::97] *= 3.0   # peaks: the limiter works
    return np.clip(np.rint(v), -full, full - 1).astype(np.int64)
