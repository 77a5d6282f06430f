"""Helpers for the -m gpu tests: drive libiamf_hip.so through its C ABI with torch tensors as
plain device memory."""
from collections import namedtuple

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


# ------------------------------------------------------------------------------------------
# buffer layouts: where a runner's input, second element, ramps and PCM rows lie in device memory
# ------------------------------------------------------------------------------------------
# include/iamf_hip.h lets a caller place its buffers freely: sample i of channel c, frame f, stream s is
# d_in[s * in_stream_stride + f * in_frame_stride + c * frame_size + i] (strides in floats), PCM row s starts at byte
# s * pcm_stream_stride_bytes.  Every runner of the GPU tests takes its buffers from place_input / place_ramp / pcm_rows and
# reads its PCM back through rows_and_rest, under one of these layouts (need: the row's bytes of a call, bps: bytes per
# sample, r16: rounded up to 16):
#
#   name         d_in - base  frame stride   stream stride      d_pcm - base  row stride
#   DENSE        0            m*fs           F*m*fs             0             need           what the runners always did
#   PAD16        4            m*fs + 4       F*(m*fs+4) + 12    16            r16(need)+48   every rule of the vector kernels holds; nothing is dense or more than 16-byte aligned
#   FRAME_MAJOR  4            S*(m*fs + 8)   m*fs + 8           16            r16(need)+16   [F][S][m][fs]: stream stride < frame stride
#   OFF_IN       1            m*fs + 1       F*(m*fs+1) + 2     0             r16(need)      only the input breaks the 16-byte rules
#   OFF_PCM      0            m*fs           F*m*fs             bps           need + bps     only the PCM breaks them
#   FAR_IN       4            2^29 + 4       m*fs + 4           0             r16(need)      frame 1 lies 2^31 + 16 bytes from frame 0, frame 2 2^32 + 32
#   FAR_PCM      0            m*fs           F*m*fs             16            2^31 + 16      row 1 crosses the signed 32-bit byte offset, row 2 the unsigned one
#
# base is 256-byte aligned.  A second element follows the same row with its own channel count, a ramp with its total in
# place of m*fs (pad +4 / offset 4 floats under PAD16, FRAME_MAJOR and the far layouts, +1 / 1 under OFF_IN); under the two
# far layouts both are placed as under PAD16.  Every float between the samples is a quiet NaN, so that a kernel that uses
# one shows it in its output; every PCM byte starts as 0xA5 and rows_and_rest asserts that all but the emitted runs still are.

# ------------------------------------------------------------------------------------------
# packet layouts: where the LPCM packet rows of iamf_hip_batch_render_lpcm and the packet-fed fan-out lie
# ------------------------------------------------------------------------------------------
# Sample i of channel c, frame f, stream s is at d_raw + s * raw_stream_stride + f * raw_frame_stride + src_offset[c] +
# src_step[c] * i (include/iamf_hip.h).  The fused kernels (render_fast_kernel<.., LP>, render_fanout_kernel<.., LP>) read
# the rows as they lie if lpcm_form() (iac_amd/csrc/lpcm_form.hpp) admits them: d_raw 16-byte aligned, both strides on the
# form's grid g (8 bytes for 16-bit samples, 4 for 24-bit), and if the call's frames fit 32-bit byte offsets
# (fast_shape_ok: (frames + 2) * raw_frame_stride + 2^24 < 2^31); every other call is unpacked to f32 first.  `row` is the
# packet row of lpcm_util.rows, a multiple of 16; B(n) = pk_bound(n) is the largest multiple of 16 that keeps the 32-bit
# rule for a call of n frames (n = 3: the longest call of the tests):
#
#   name            d_raw - base  frame stride  stream stride        meant to
#   PK_DENSE        0             row           F*row                what the runners always did
#   PK_PAD16        16            row + 16      F*(row+16) + 48      nothing dense, everything 16-byte aligned: fused on every call
#   PK_GRID         16            row + g       F*(row+g) + g        strides only on the form's grid: a call from an odd frame has d_raw off 16 bytes
#   PK_OFF_BASE     8             row + 16      F*(row+16)           d_raw & 15 != 0: every call unfused
#   PK_OFF_STRIDE   0             row + g/2     F*(row+g/2)          frame stride off the grid: every call unfused
#   PK_FAR_STREAMS  16            row           2^31 + 16            stream 1 crosses the signed 32-bit byte offset, stream 2 the unsigned one
#   PK_BOUND        0             B(n)          F*B(n)               the largest frame stride at which the call of n frames is still fused
#   PK_BEYOND       0             B(n) + 16     F*(B(n)+16)          the call of n frames unfused (the unpacker at far frame strides), shorter ones fused
#   PK_FRAME_MAJOR  16            S*(row+16)    row + 16             [F][S][row]: stream stride < frames * frame stride, which the ABI refuses
#
# base is 256-byte aligned.  Every byte that belongs to no channel's run is 0x7F at an even address and 0x80 at an odd
# one: a load that strays yields a sample near full scale.

Layout = namedtuple("Layout", "name")
DENSE, PAD16, FRAME_MAJOR, OFF_IN, OFF_PCM, FAR_IN, FAR_PCM = [
    Layout(n) for n in ("DENSE", "PAD16", "FRAME_MAJOR", "OFF_IN", "OFF_PCM", "FAR_IN", "FAR_PCM")]
SMALL_LAYOUTS = [DENSE, PAD16, FRAME_MAJOR, OFF_IN, OFF_PCM]
FAR_LAYOUTS = [FAR_IN, FAR_PCM]

NAN_BITS = 0x7FC00000
FILL = 0xA5
FAR_GUARD = 64 * 1024     # far layouts: the bytes written (and looked at) on each side of a frame / a PCM row
PCM_HEAD = 256            # non-dense layouts: the bytes in front of the base and behind the last row


def r16(x):
    return (x + 15) & ~15


def input_geometry(layout, S, F, m, fs):
    """-> (d_in - base, frame stride, stream stride) in floats, the table above"""
    e = m * fs
    if layout in (DENSE, OFF_PCM, FAR_PCM):
        return 0, e, F * e
    if layout == PAD16:
        return 4, e + 4, F * (e + 4) + 12
    if layout == FRAME_MAJOR:
        return 4, S * (e + 8), e + 8
    if layout == OFF_IN:
        return 1, e + 1, F * (e + 1) + 2
    if layout == FAR_IN:
        return 4, 2 ** 29 + 4, e + 4
    raise ValueError(layout)


def ramp_geometry(layout, total):
    """-> (pointer - base, ramp_stream_stride) in floats"""
    if layout in (DENSE, OFF_PCM):
        return 0, total
    if layout == OFF_IN:
        return 1, total + 1
    return 4, total + 4


def pcm_geometry(layout, need, bps):
    """-> (d_pcm - base, pcm_stream_stride_bytes)"""
    if layout == DENSE:
        return 0, need
    if layout == PAD16:
        return 16, r16(need) + 48
    if layout == FRAME_MAJOR:
        return 16, r16(need) + 16
    if layout in (OFF_IN, FAR_IN):
        return 0, r16(need)
    if layout == OFF_PCM:
        return bps, need + bps
    if layout == FAR_PCM:
        return 16, 2 ** 31 + 16
    raise ValueError(layout)


def second_layout(layout):
    """the layout of a second element and of the ramps beside an input under `layout`"""
    return PAD16 if layout in FAR_LAYOUTS else layout


class TorchBackend:
    """device memory as flat torch tensors"""

    def upload(self, host):
        return torch.from_numpy(host).cuda()

    def empty(self, n, dtype):
        return torch.empty(n, dtype={np.float32: torch.float32, np.uint8: torch.uint8}[dtype], device="cuda")

    def assign(self, t, start, host):
        t[start:start + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()

    def read(self, t, start, stop):
        return t[start:stop].cpu().numpy()

    def ptr(self, t):
        return t.data_ptr()


class NumpyBackend:
    """host memory in its place, for tests/test_layouts_cpu.py"""

    def upload(self, host):
        return host.copy()

    def empty(self, n, dtype):
        return np.empty(n, dtype=dtype)

    def assign(self, t, start, host):
        t[start:start + host.size] = np.ascontiguousarray(host).reshape(-1)

    def read(self, t, start, stop):
        return t[start:stop].copy()

    def ptr(self, t):
        return t.ctypes.data


TORCH = TorchBackend()

Placed = namedtuple("Placed", "keep d_in stream_stride frame_stride")


class _Input:
    """a placed [S][F][m][fs] array: the allocation and the float index of sample [0][0][0][0] in it"""

    def __init__(self, tensor, first, backend):
        self.tensor, self.first, self.backend = tensor, first, backend

    def ptr(self, floats):
        return self.backend.ptr(self.tensor) + 4 * (self.first + floats)


def _nans(n):
    return np.full(n, NAN_BITS, dtype=np.uint32).view(np.float32)


def _place(x, off, fst, sst, backend):
    """x [S][F][m][fs] with sample [s][f][c][i] at float first + s*sst + f*fst + c*fs + i of a fresh allocation, which
    covers every address that formula names plus one frame (m*fs floats, rounded up to 256 bytes) in front and behind;
    every other float a quiet NaN.  Where that is too much for a host image (FAR_IN) the allocation is left as it comes
    and only the frames, with FAR_GUARD bytes of NaN around each, are written."""
    S, F, m, fs = x.shape
    e = m * fs
    slack = (e + 63) & ~63
    first = slack + off
    span = (S - 1) * sst + (F - 1) * fst + e
    n = first + span + slack
    if n * 4 < (1 << 28):
        host = _nans(n)
        for s in range(S):
            for f in range(F):
                a = first + s * sst + f * fst
                host[a:a + e] = x[s, f].reshape(-1)
        return _Input(backend.upload(host), first, backend)
    assert sst < fst, "a far layout keeps the streams of a frame together"
    t = backend.empty(n, np.float32)
    g = FAR_GUARD // 4
    for f in range(F):
        lo = max(first + f * fst - g, 0)
        hi = min(first + f * fst + (S - 1) * sst + e + g, n)
        host = _nans(hi - lo)
        for s in range(S):
            a = first + f * fst + s * sst - lo
            host[a:a + e] = x[s, f].reshape(-1)
        backend.assign(t, lo, host)
    return _Input(t, first, backend)


def place_input(x_frames, layout, f0=0, nf=None, backend=TORCH, keep=None):
    """x_frames: numpy [S][F][m][fs].  Returns Placed(keep, d_in, in_stream_stride, in_frame_stride) for the call that
    starts at frame f0 and takes nf frames; keep is what holds the device memory (pass it back for the next call of the
    same array instead of placing it again)."""
    S, F, m, fs = x_frames.shape
    assert 0 <= f0 and f0 + (nf or 0) <= F
    off, fst, sst = input_geometry(layout, S, F, m, fs)
    if keep is None:
        if (off, fst, sst) == (0, m * fs, F * m * fs):     # dense: the array as it is
            keep = _Input(backend.upload(np.ascontiguousarray(x_frames, dtype=np.float32)), 0, backend)
        else:
            keep = _place(np.asarray(x_frames, dtype=np.float32), off, fst, sst, backend)
    return Placed(keep, keep.ptr(f0 * fst), sst, fst)


def place_ramp(ramp, layout, backend=TORCH):
    """ramp: numpy [S][total].  Returns (keep, ramp_stream_stride); keep.ptr(i) is the pointer of a call that starts at
    sample i"""
    S, total = ramp.shape
    off, stride = ramp_geometry(layout, total)
    r = np.ascontiguousarray(ramp, dtype=np.float32)
    if (off, stride) == (0, total):
        return _Input(backend.upload(r), 0, backend), stride
    return _place(r.reshape(S, 1, 1, total), off, stride, stride, backend), stride


class PcmRows:
    """an allocation of S PCM rows under a layout; .d_pcm and .stride are the call's arguments.  room: bytes kept free
    behind the last row; share / lead: no allocation of its own — the rows lie in the allocation of `share` (far rows of
    the same layout, made with room for them), `lead` bytes behind its rows: the members of a fan-out under a far layout
    then take one allocation between them, their guard zones apart"""

    def __init__(self, S, need, layout, bps, backend, room=0, share=None, lead=0):
        off, stride = pcm_geometry(layout, need, bps)
        head = 0 if layout == DENSE else PCM_HEAD
        self.S, self.need, self.layout, self.backend, self.stride = S, need, layout, backend, stride
        self.first = head + off + lead
        self.size = self.first + (S - 1) * stride + need + head + room
        self.far = self.size >= (1 << 28)
        if share is not None:
            assert share.far and self.far and share.layout == layout and share.stride == stride and self.size <= share.size
            self.tensor = share.tensor
        elif not self.far:
            self.tensor = backend.upload(np.full(self.size, FILL, dtype=np.uint8))
        else:
            self.tensor = backend.empty(self.size, np.uint8)
        if self.far:
            for lo, hi in self._zones():
                backend.assign(self.tensor, lo, np.full(hi - lo, FILL, dtype=np.uint8))
        self.d_pcm = backend.ptr(self.tensor) + self.first

    def _zones(self):
        """far rows: each row with FAR_GUARD bytes on either side, clipped to the allocation"""
        return [(max(self.first + s * self.stride - FAR_GUARD, 0),
                 min(self.first + s * self.stride + self.need + FAR_GUARD, self.size)) for s in range(self.S)]


def pcm_rows(S, need_bytes, layout, bps=2, backend=TORCH, **kw):
    """Returns (rows, d_pcm, pcm_stream_stride_bytes): S rows of need_bytes under `layout`, every byte of the allocation
    0xA5 (under FAR_PCM: FAR_GUARD bytes on each side of every row; the rest is never looked at).  kw: PcmRows' room,
    share and lead."""
    rows = PcmRows(S, need_bytes, layout, bps, backend, **kw)
    return rows, rows.d_pcm, rows.stride


def pcm_rows_of_members(S, needs, layout, bpss, backend=TORCH):
    """one PcmRows per member of a fan-out: allocations of their own, or, where the layout puts the rows far apart, one
    allocation for all of them with every member's rows 2 * FAR_GUARD (and a little) behind the member's before"""
    if pcm_geometry(layout, needs[0], bpss[0])[1] < (1 << 28):
        return [PcmRows(S, n, layout, b, backend) for n, b in zip(needs, bpss)]
    leads = [0]
    for n in needs[:-1]:
        leads.append(leads[-1] + r16(n) + 2 * FAR_GUARD + 256)
    first = PcmRows(S, needs[0], layout, bpss[0], backend, room=leads[-1] + needs[-1])
    return [first] + [PcmRows(S, n, layout, b, backend, share=first, lead=l) for n, b, l in zip(needs[1:], bpss[1:], leads[1:])]


def rows_and_rest(rows, layout, n_bytes, only=None):
    """Per stream the first n_bytes of its row (numpy uint8), having asserted that every other byte of the allocation is
    still 0xA5: the head, the rest of each row beyond the emitted run, the gaps between rows and the tail.  only: (s0, cnt) —
    a call over that range of streams: the rows outside it must be untouched and come back empty."""
    assert layout == rows.layout and 0 <= n_bytes <= rows.need
    zones = rows._zones() if rows.far else [(0, rows.size)]
    out = [None] * rows.S
    want = [n_bytes if only is None or only[0] <= s < only[0] + only[1] else 0 for s in range(rows.S)]
    for lo, hi in zones:
        h = rows.backend.read(rows.tensor, lo, hi)
        for s in range(rows.S):
            a = rows.first + s * rows.stride
            if lo <= a and a + want[s] <= hi:
                out[s] = h[a - lo:a - lo + want[s]].copy()
                h[a - lo:a - lo + want[s]] = FILL
        bad = np.flatnonzero(h != FILL)
        if bad.size:
            at = int(bad[0]) + lo - rows.first
            s = min(max(at // rows.stride, 0), rows.S - 1) if rows.stride else 0
            raise AssertionError("%s: %d bytes outside the emitted runs were written, the first at byte %d of row %d "
                                 "(%d bytes emitted, rows of %d, stride %d)"
                                 % (layout.name, bad.size, at - s * rows.stride, s, want[s], rows.need, rows.stride))
    assert all(o is not None for o in out)
    return out


# ---- the packet layouts (the second table at the top of the file) ----

PK_DENSE, PK_PAD16, PK_GRID, PK_OFF_BASE, PK_OFF_STRIDE, PK_FAR_STREAMS, PK_BOUND, PK_BEYOND, PK_FRAME_MAJOR = [
    Layout(n) for n in ("PK_DENSE", "PK_PAD16", "PK_GRID", "PK_OFF_BASE", "PK_OFF_STRIDE", "PK_FAR_STREAMS", "PK_BOUND", "PK_BEYOND",
                        "PK_FRAME_MAJOR")]
PK_SMALL = [PK_DENSE, PK_PAD16, PK_GRID, PK_OFF_BASE, PK_OFF_STRIDE]
PK_FAR = [PK_FAR_STREAMS, PK_BOUND, PK_BEYOND]
PK_LAYOUTS = PK_SMALL + PK_FAR
PK_LONGEST = 3            # frames of the longest call of the tests: the n of B(n)


def pk_grid(sample_bytes):
    """the alignment grid of the fusable form with that many bytes per sample (lpcm_form.hpp)"""
    return {2: 8, 3: 4}[sample_bytes]


def pk_bound(n):
    """B(n): the largest multiple of 16 with (n + 2) * B + 2^24 < 2^31"""
    return ((2 ** 31 - 2 ** 24 - 1) // (n + 2)) & ~15


def packet_geometry(layout, S, F, row, sample_bytes, longest=PK_LONGEST):
    """-> (d_raw - base, raw_frame_stride, raw_stream_stride) in bytes, the table above"""
    g = pk_grid(sample_bytes)
    if layout == PK_DENSE:
        return 0, row, F * row
    if layout == PK_PAD16:
        return 16, row + 16, F * (row + 16) + 48
    if layout == PK_GRID:
        return 16, row + g, F * (row + g) + g
    if layout == PK_OFF_BASE:
        return 8, row + 16, F * (row + 16)
    if layout == PK_OFF_STRIDE:
        return 0, row + g // 2, F * (row + g // 2)
    if layout == PK_FAR_STREAMS:
        return 16, row, 2 ** 31 + 16
    if layout == PK_BOUND:
        return 0, pk_bound(longest), F * pk_bound(longest)
    if layout == PK_BEYOND:
        return 0, pk_bound(longest) + 16, F * (pk_bound(longest) + 16)
    if layout == PK_FRAME_MAJOR:
        return 16, S * (row + 16), row + 16
    raise ValueError(layout)


def packet_fill(lo, hi):
    """the bytes [lo, hi) of an allocation that holds no packets: 0x7F / 0x80 alternating by byte address"""
    return np.where(np.arange(lo, hi) % 2 == 0, 0x7F, 0x80).astype(np.uint8)


def packet_run_mask(L, row):
    """[row] bool: the bytes of a packet row that belong to a channel's run"""
    used = np.zeros(row, dtype=bool)
    i = np.arange(L.frame_size)[:, None]
    for c in range(L.channels):
        if L.src_offset[c] >= 0:
            used[(L.src_offset[c] + L.src_step[c] * i + np.arange(L.sample_bytes)[None, :]).reshape(-1)] = True
    return used


class _Packets:
    """placed packet rows [S][F][row]: the allocation, the byte index of row [0][0] in it, and the zones that were written
    ([(lo, hi)]: the whole allocation unless it is a far one)"""

    def __init__(self, tensor, first, size, zones, backend):
        self.tensor, self.first, self.size, self.zones, self.backend = tensor, first, size, zones, backend

    def ptr(self, nbytes):
        return self.backend.ptr(self.tensor) + self.first + nbytes


def _place_packets(raw, L, off, fst, sst, dense, backend):
    """raw [S][F][row] with row [s][f] at byte first + s*sst + f*fst of a fresh allocation, which covers every row plus a
    row (rounded up to 256 bytes) in front and behind (dense: the rows and nothing else); the bytes of the rows that are
    in no run, and every byte between the rows, are the fill.  Where that exceeds 2^28 bytes the allocation is left as it
    comes and only the rows, with FAR_GUARD bytes of fill on either side, are written."""
    S, F, row = raw.shape
    used = packet_run_mask(L, row)
    slack = 0 if dense else (row + 255) & ~255
    first = slack + off
    starts = sorted(first + s * sst + f * fst for s in range(S) for f in range(F))
    assert all(b - a >= row for a, b in zip(starts, starts[1:])), "rows overlap"
    n = starts[-1] + row + slack

    def image(lo, hi):
        host = packet_fill(lo, hi)
        for s in range(S):
            for f in range(F):
                a = first + s * sst + f * fst
                if lo <= a and a + row <= hi:
                    host[a - lo:a - lo + row] = np.where(used, raw[s, f], host[a - lo:a - lo + row])
        return host

    if n < (1 << 28):
        return _Packets(backend.upload(image(0, n)), first, n, [(0, n)], backend)
    t = backend.empty(n, np.uint8)
    zones = []
    for a in starts:        # rows closer than the guards share a zone
        lo, hi = max(a - FAR_GUARD, 0), min(a + row + FAR_GUARD, n)
        if zones and lo <= zones[-1][1]:
            zones[-1] = (zones[-1][0], hi)
        else:
            zones.append((lo, hi))
    for lo, hi in zones:
        backend.assign(t, lo, image(lo, hi))
    return _Packets(t, first, n, zones, backend)


PlacedPackets = namedtuple("PlacedPackets", "keep d_raw stream_stride frame_stride")


def place_packets(raw, L, layout, f0=0, nf=None, backend=TORCH, keep=None, longest=PK_LONGEST):
    """raw: numpy uint8 [S][F][row] and L, the rows and the layout of lpcm_util.rows.  Returns PlacedPackets(keep, d_raw,
    raw_stream_stride, raw_frame_stride) for the call that starts at frame f0 and takes nf frames; keep is what holds the
    device memory (pass it back for the next call of the same rows instead of placing them again)."""
    S, F, row = raw.shape
    assert row % 16 == 0 and 0 <= f0 and f0 + (nf or 0) <= F
    off, fst, sst = packet_geometry(layout, S, F, row, L.sample_bytes, longest)
    if keep is None:
        keep = _place_packets(np.ascontiguousarray(raw, dtype=np.uint8), L, off, fst, sst, layout == PK_DENSE, backend)
    return PlacedPackets(keep, keep.ptr(f0 * fst), sst, fst)


def hip_render(matrix, out_ch, x, frame_size, fmt=A.FMT_S16, limiter=True, flush=True,
               frames_per_call=None, gains=None, loudness=False, threshold_db=-1.0,
               sample_rate=48000, projection=0, fir_taps=0, lfe_hoa=False, layout=DENSE, refused=None):
    """x: numpy [S][m][total].  Returns a list (per stream) of arrays [n_out][out_ch] (S24:
    [n_out][out_ch][3] bytes) — everything the calls emitted, concatenated.
    refused: (layout, error code, frames) — before anything is rendered, a call of that many frames is made under that
    layout and must be refused with that code, leaving its PCM rows and (as the result shows) the batch's state untouched."""
    S, m, total = x.shape
    xf = to_frames(x, frame_size)
    F = total // frame_size
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    b = A.Batch(S, matrix, out_ch, frame_size=frame_size, sample_rate=sample_rate, out_format=fmt,
                limiter=limiter, threshold_db=threshold_db, loudness=loudness, projection=projection,
                fir_taps=fir_taps, lfe_hoa=lfe_hoa)
    if gains:
        b.set_gains(**gains)
    calls = frames_per_call or [F]
    assert sum(calls) == F
    outs = [[] for _ in range(S)]
    st = torch.cuda.current_stream().cuda_stream
    if refused:
        r_layout, code, nf = refused
        cap = max(nf * frame_size, 240) * out_ch * bps
        rows = pl = None
        try:
            rows, d_pcm, stride = pcm_rows(S, cap, r_layout, bps)
            pl = place_input(xf, r_layout, 0, nf)
            try:
                b.render(pl.d_in, pl.stream_stride, pl.frame_stride, nf, d_pcm, stride, st)
                raise AssertionError("a call under %s was not refused" % r_layout.name)
            except A.IamfHipError as e:
                assert e.code == code, (r_layout.name, e.code, code)
            torch.cuda.synchronize()
            rows_and_rest(rows, r_layout, 0)
        finally:
            rows = pl = None
    rows = pl = keep = None
    f0 = 0
    try:
        for nf in calls:
            cap = max(nf * frame_size, 240) * out_ch * bps
            pl = place_input(xf, layout, f0, nf, keep=keep)
            keep = pl.keep
            rows, d_pcm, stride = pcm_rows(S, cap, layout, bps)
            n = b.render(pl.d_in, pl.stream_stride, pl.frame_stride, nf, d_pcm, stride, st)
            torch.cuda.synchronize()
            h = rows_and_rest(rows, layout, n * out_ch * bps)
            rows = None
            for s in range(S):
                outs[s].append(_view(h[s], n, out_ch, fmt))
            f0 += nf
        if flush:
            cap = 240 * out_ch * bps
            rows, d_pcm, stride = pcm_rows(S, cap, layout, bps)
            n = b.flush(d_pcm, stride, st)
            torch.cuda.synchronize()
            h = rows_and_rest(rows, layout, n * out_ch * bps)
            rows = None
            for s in range(S):
                outs[s].append(_view(h[s], n, out_ch, fmt))
    finally:
        rows = pl = keep = None     # the far layouts hold gigabytes
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
            calls=None, flush=True, layout=DENSE):
    """x: [S][m][total]; returns list of per-stream outputs"""
    total = x.shape[2]
    F = total // fs
    xf = to_frames(x, fs)
    xf2 = to_frames(x2, fs) if x2 is not None else None
    lay2 = second_layout(layout)
    bps = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}[fmt]
    d_ramps = {k: place_ramp(np.ascontiguousarray(v, dtype=np.float32).reshape(S, total), lay2)
               for k, v in (ramps or {}).items()}
    d_dmx = None
    if dmx_frames is not None:
        raw = np.frombuffer(bytes(dmx_frames), dtype=np.uint8).copy()
        d_dmx = torch.from_numpy(raw).cuda()
    outs = [[] for _ in range(S)]
    st = torch.cuda.current_stream().cuda_stream
    f0 = 0
    rows = pl = pl2 = keep = keep2 = None
    try:
        for nf in (calls or [F]):
            cap = max(nf * fs, 240) * out_ch * bps
            rows, d_pcm, stride = pcm_rows(S, cap, layout, bps)
            a = A.RenderArgs()
            pl = place_input(xf, layout, f0, nf, keep=keep)
            keep = pl.keep
            a.d_in, a.in_stream_stride, a.in_frame_stride = pl.d_in, pl.stream_stride, pl.frame_stride
            if xf2 is not None:
                pl2 = place_input(xf2, lay2, f0, nf, keep=keep2)
                keep2 = pl2.keep
                a.d_in2, a.in2_stream_stride, a.in2_frame_stride = pl2.d_in, pl2.stream_stride, pl2.frame_stride
            a.ramp_stream_stride = ramp_geometry(lay2, total)[1]
            for key, field in (("element", "d_element_ramp"), ("element2", "d_element2_ramp"), ("output", "d_output_ramp")):
                if key in d_ramps:
                    setattr(a, field, d_ramps[key][0].ptr(f0 * fs))
            if d_dmx is not None:
                assert calls is None  # one call: frames index from 0
                a.d_dmx_frames = d_dmx.data_ptr()
            a.n_frames = nf
            a.d_pcm = d_pcm
            a.pcm_stream_stride_bytes = stride
            a.stream = st
            n = batch.render_ex(a)
            torch.cuda.synchronize()
            h = rows_and_rest(rows, layout, n * out_ch * bps)
            rows = None
            for s in range(S):
                outs[s].append(_view(h[s], n, out_ch, fmt))
            f0 += nf
        if flush:
            cap = 240 * out_ch * bps
            rows, d_pcm, stride = pcm_rows(S, cap, layout, bps)
            n = batch.flush(d_pcm, stride, st)
            torch.cuda.synchronize()
            h = rows_and_rest(rows, layout, n * out_ch * bps)
            rows = None
            for s in range(S):
                outs[s].append(_view(h[s], n, out_ch, fmt))
    finally:
        rows = pl = pl2 = keep = keep2 = None
    return [np.concatenate(o, axis=0) for o in outs]
