"""The buffer layouts of tests/gpu_util.py (place_input, place_ramp, pcm_rows, rows_and_rest), without a GPU: the helper
runs on numpy arrays in place of device memory.  The GPU tests trust it to put every sample where the ABI's formula of
include/iamf_hip.h looks for it, to leave a NaN everywhere else and to notice a single PCM byte written outside the
emitted runs; tests/test_gpu_layouts.py then proves nothing about a kernel unless that holds."""
import numpy as np
import pytest

import gpu_util as G

NP = G.NumpyBackend()
S, F, M, FS = 3, 4, 2, 24
SMALL = G.SMALL_LAYOUTS
IDS = [l.name for l in SMALL]


def _x(m=M):
    return (np.arange(S * F * m * FS, dtype=np.float32) + 1.0).reshape(S, F, m, FS)


def _floats(keep):
    return keep.tensor.reshape(-1), NP.ptr(keep.tensor)      # (dense: the array in its own shape)


@pytest.mark.parametrize("layout", SMALL, ids=IDS)
def test_every_sample_is_where_the_header_formula_looks_and_the_rest_is_nan(layout):
    x = _x()
    keep = None
    named = None
    for f0, nf in ((0, 1), (1, 2), (3, 1)):
        pl = G.place_input(x, layout, f0, nf, backend=NP, keep=keep)
        assert keep is None or pl.keep is keep, "one allocation for the calls of one array"
        keep = pl.keep
        buf, p0 = _floats(keep)
        assert (pl.d_in - p0) % 4 == 0
        base = (pl.d_in - p0) // 4
        named = np.zeros(buf.size, dtype=bool) if named is None else named
        for s in range(S):
            for f in range(nf):
                for c in range(M):
                    a = base + s * pl.stream_stride + f * pl.frame_stride + c * FS
                    assert 0 <= a and a + FS <= buf.size
                    assert np.array_equal(buf[a:a + FS], x[s, f0 + f, c]), (layout.name, s, f0 + f, c)
                    assert not named[a:a + FS].any(), "two samples share an address"
                    named[a:a + FS] = True
    assert int(named.sum()) == x.size
    rest = buf.view(np.uint32)[~named]
    assert (rest == G.NAN_BITS).all(), "every float that is no sample is the quiet NaN"
    if layout in (G.DENSE, G.OFF_PCM):
        assert rest.size == 0 and buf.size == x.size
    else:
        first = int(np.flatnonzero(named)[0])
        last = int(np.flatnonzero(named)[-1])
        assert first >= M * FS and buf.size - 1 - last >= M * FS, "a frame of slack in front and behind"
        assert rest.size > 0


def test_the_geometry_is_the_table_of_the_layouts():
    e = M * FS
    assert G.input_geometry(G.DENSE, S, F, M, FS) == (0, e, F * e)
    assert G.input_geometry(G.PAD16, S, F, M, FS) == (4, e + 4, F * (e + 4) + 12)
    assert G.input_geometry(G.FRAME_MAJOR, S, F, M, FS) == (4, S * (e + 8), e + 8)
    assert G.input_geometry(G.OFF_IN, S, F, M, FS) == (1, e + 1, F * (e + 1) + 2)
    assert G.input_geometry(G.OFF_PCM, S, F, M, FS) == (0, e, F * e)
    assert G.pcm_geometry(G.DENSE, 1000, 2) == (0, 1000)
    assert G.pcm_geometry(G.PAD16, 1000, 2) == (16, 1008 + 48)
    assert G.pcm_geometry(G.FRAME_MAJOR, 1000, 2) == (16, 1008 + 16)
    assert G.pcm_geometry(G.OFF_IN, 1000, 2) == (0, 1008)
    assert G.pcm_geometry(G.OFF_PCM, 1000, 3) == (3, 1003)
    assert [G.ramp_geometry(l, 96) for l in SMALL] == [(0, 96), (4, 100), (4, 100), (1, 97), (0, 96)]
    assert [G.second_layout(l) for l in SMALL + G.FAR_LAYOUTS] == SMALL + [G.PAD16, G.PAD16]


@pytest.mark.parametrize("layout", SMALL, ids=IDS)
def test_which_rules_of_the_vector_kernels_a_layout_keeps(layout):
    """16-byte pointers and strides that are multiples of 4 floats / 16 bytes: kept by DENSE, PAD16 and FRAME_MAJOR, broken
    on the input side alone by OFF_IN and on the PCM side alone by OFF_PCM; PAD16 and FRAME_MAJOR are not 32-byte aligned"""
    pl = G.place_input(_x(), layout, 1, 2, backend=NP)
    _, p0 = _floats(pl.keep)
    rel = pl.d_in - 4 * pl.frame_stride - p0 - 4 * pl.keep.first        # frame 0 against the allocation's base
    assert rel == 0
    off = 4 * (pl.keep.first % 64)                                       # bytes beyond a 256-byte boundary
    in_ok = off % 16 == 0 and pl.stream_stride % 4 == 0 and pl.frame_stride % 4 == 0
    rows, d_pcm, stride = G.pcm_rows(S, 1024, layout, 2, backend=NP)         # rows of whole 16-byte pieces, as the cases have
    poff = rows.first % 256
    pcm_ok = poff % 16 == 0 and stride % 16 == 0
    assert in_ok == (layout != G.OFF_IN) and pcm_ok == (layout != G.OFF_PCM)
    if layout in (G.PAD16, G.FRAME_MAJOR):
        assert off % 32 == 16 and poff % 32 == 16
        assert stride > 1024 and pl.frame_stride > M * FS


@pytest.mark.parametrize("layout", SMALL, ids=IDS)
def test_second_element_and_ramps_follow_the_layout(layout):
    x2 = _x(1)
    pl = G.place_input(x2, layout, 2, 1, backend=NP)
    buf, p0 = _floats(pl.keep)
    base = (pl.d_in - p0) // 4
    for s in range(S):
        assert np.array_equal(buf[base + s * pl.stream_stride:][:FS], x2[s, 2, 0])
    total = F * FS
    ramp = np.linspace(0.5, 1.5, S * total, dtype=np.float32).reshape(S, total)
    keep, stride = G.place_ramp(ramp, layout, backend=NP)
    buf, p0 = _floats(keep)
    assert stride == G.ramp_geometry(layout, total)[1]
    at = (keep.ptr(FS) - p0) // 4                                        # the call that starts at frame 1
    named = np.zeros(buf.size, dtype=bool)
    for s in range(S):
        assert np.array_equal(buf[at + s * stride:][:total - FS], ramp[s, FS:])
        named[at - FS + s * stride:][:total] = True
    assert (buf.view(np.uint32)[~named] == G.NAN_BITS).all()


def test_dense_is_what_the_runners_always_passed():
    """the literal expressions of gpu_util.hip_render, run_ex and route_cases._ex_loop before they took a layout"""
    x = _x()
    for f0 in range(F):
        pl = G.place_input(x, G.DENSE, f0, 1, backend=NP)
        buf, p0 = _floats(pl.keep)
        assert pl.keep.tensor.shape == x.shape
        assert np.array_equal(np.asarray(buf).reshape(-1), np.ascontiguousarray(x).reshape(-1))
        assert (pl.d_in, pl.stream_stride, pl.frame_stride) == (p0 + 4 * f0 * M * FS, F * M * FS, M * FS)
    cap = max(1 * 1024, 240) * 2 * 2
    rows, d_pcm, stride = G.pcm_rows(S, cap, G.DENSE, 2, backend=NP)
    assert (d_pcm, stride, rows.tensor.size) == (NP.ptr(rows.tensor), cap, S * cap)
    keep, rs = G.place_ramp(np.ones((S, 96), dtype=np.float32), G.DENSE, backend=NP)
    assert rs == 96 and keep.ptr(24) == NP.ptr(keep.tensor) + 4 * 24 and keep.tensor.size == S * 96


@pytest.mark.parametrize("layout", SMALL, ids=IDS)
def test_rows_and_rest_returns_the_runs_and_sees_every_other_byte(layout):
    need, n = 1000, 600
    rows, d_pcm, stride = G.pcm_rows(S, need, layout, 2, backend=NP)
    t = rows.tensor
    assert (t == G.FILL).all()
    assert [r.size for r in G.rows_and_rest(rows, layout, 0)] == [0] * S     # untouched: accepted
    row0 = d_pcm - NP.ptr(t)
    for s in range(S):                                                       # what a kernel emits
        t[row0 + s * stride:][:n] = (np.arange(n) + s) & 0x7F
    got = G.rows_and_rest(rows, layout, n)
    for s in range(S):
        assert np.array_equal(got[s], ((np.arange(n) + s) & 0x7F).astype(np.uint8))
    places = {"the tail of a row": [row0 + n, row0 + need - 1, row0 + (S - 1) * stride + n,
                                    row0 + (S - 1) * stride + need - 1]}
    if stride > need:
        places["between rows"] = [row0 + need, row0 + stride - 1]
    if row0 > 0:
        places["before row 0"] = [0, row0 - 1]
    if t.size > row0 + (S - 1) * stride + need:
        places["after the last row"] = [row0 + (S - 1) * stride + need, t.size - 1]
    if layout != G.DENSE:
        assert {"before row 0", "after the last row"} <= set(places)
    if layout in (G.PAD16, G.FRAME_MAJOR, G.OFF_IN, G.OFF_PCM):
        assert "between rows" in places
    for what, at in places.items():
        for a in at:
            old = t[a]
            t[a] = 0x00
            with pytest.raises(AssertionError, match="outside the emitted runs"):
                G.rows_and_rest(rows, layout, n)
            t[a] = old
    G.rows_and_rest(rows, layout, n)


def test_far_layouts_arithmetic():
    """no allocation: only where the frames and rows lie"""
    m, fs = 16, 1024
    off, fst, sst = G.input_geometry(G.FAR_IN, 3, 4, m, fs)
    assert (off, fst, sst) == (4, 2 ** 29 + 4, m * fs + 4)
    assert 4 * fst == 2 ** 31 + 16 and 4 * 2 * fst == 2 ** 32 + 32           # frames 1 and 2 of a call, in bytes
    assert 3 * sst < fst, "the streams of a frame do not reach the next frame"
    assert off % 4 == 0 and fst % 4 == 0 and sst % 4 == 0, "every 16-byte rule holds: only the 32-bit rule refuses it"
    assert 3 * fst * 4 + 4 * (3 * sst + 2 * m * fs) < 7 * 2 ** 30, "about 6 GiB for a programme of 4 frames"
    assert G.input_geometry(G.FAR_PCM, 3, 4, m, fs) == G.input_geometry(G.DENSE, 3, 4, m, fs)
    need = 3 * 1024 * 12 * 2
    poff, stride = G.pcm_geometry(G.FAR_PCM, need, 2)
    assert (poff, stride) == (16, 2 ** 31 + 16) and stride % 16 == 0
    assert stride > 2 ** 31 - 1 and 2 * stride > 2 ** 32 - 1                  # row 1: signed, row 2: unsigned
    assert G.pcm_geometry(G.FAR_IN, need, 2) == (0, G.r16(need))
    assert 2 * stride + need + 2 * G.PCM_HEAD < 5 * 2 ** 30, "about 4 GiB for 3 rows"
