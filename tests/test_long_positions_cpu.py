"""The cases of tests/test_gpu_long_positions.py, without a GPU: every shift puts its boundary where the case is meant
to have it, and every programme has the limiter at work there, judged by the oracle's limiter trace alone.  Without
that, a position bug in the look-ahead would meet only unity gain."""
import numpy as np
import pytest

import long_positions as LPOS
import oracle_lib as O


def test_shifts():
    names = [n for n, _, _ in LPOS.SHIFTS]
    assert names == ["across_2^31", "across_2^32", "at_2^40"]
    d31, d32, d40 = [d for _, d, _ in LPOS.SHIFTS]
    assert d31 % 512 == 0 and d31 % 1280 != 0               # a multiple of one ring length only
    assert d32 % 512 != 0 and d32 % 1280 != 0               # of neither
    assert d40 % 512 == 0 and d40 % 1280 == 0               # of both
    assert LPOS.ODD[1] % 2 == 1


@pytest.mark.parametrize("fam", LPOS.FAMILIES, ids=lambda f: f.id)
def test_boundary_falls_inside_the_two_frame_call(fam):
    """Q = P + D keeps P's place on the 16-sample grid, lies about a frame and a half below the boundary, and the boundary
    falls inside the target's second call, off that call's 1024-sample chunks; the landing at 2^40 crosses nothing"""
    P, fs = fam.pos, fam.fs
    assert fam.frames * fs == fam.n + fam.trim and sum(fam.calls) * fs == 4096 - 96 * (fs == 1000)
    lo, hi = P + fam.calls[0] * fs, P + (fam.calls[0] + fam.calls[1]) * fs
    for name, D, edge in fam.shifts:
        Q = P + D
        if name != "odd":
            assert Q % 16 == P % 16
        if edge is None:
            assert Q > LPOS.B40 and (Q + 4096) >> 40 == 1
            continue
        B = D + edge
        assert B in (LPOS.B31, LPOS.B32)
        assert lo < edge < hi and (edge - lo) % 1024 != 0, (name, lo, edge, hi)
        assert abs((B - Q) - (fam.calls[0] * fs + 512)) <= 512, (name, B - Q)


@pytest.mark.parametrize("fam", [f for f in LPOS.FAMILIES if f.limiter], ids=lambda f: f.id)
def test_limiter_is_at_work_on_both_sides_of_the_boundary(fam):
    """for every stream (and member) and every boundary: the gain applied to the boundary sample and the gain applied at
    the boundary step (to the sample 240 earlier) are below 1, and a trigger falls within 240 samples on either side.  The
    same at the export, sample P: the stream leaves its source with the limiter engaged (a stream whose first frame was
    trimmed leaves it in the release of the burst before, with no trigger that near)."""
    fam.make()
    sizes = [fam.fs] * fam.frames
    sizes[0] -= fam.trim
    for j in range(len(fam.ocs)):
        for s in range(LPOS.S):
            z = fam.limiter_input(s, j)
            assert z.shape == (fam.ocs[j], fam.n)
            y, t = O.limiter_trace(z, sizes)
            trig = np.flatnonzero(t & O.LIM_TRIGGER)
            edges = sorted({e for _, _, e in fam.shifts if e is not None} | {fam.pos})
            for e in edges:
                what = (fam.id, j, s, e)
                for k in (e, e - 240):     # (the output lags the input by 240 samples: y[:, k] is g * z[:, k])
                    c = int(np.argmax(np.abs(z[:, k])))
                    assert z[c, k] != 0.0 and abs(y[c, k]) < abs(z[c, k]), what
                assert (t[e] & 3) != O.LIM_IDLE, what
                if e == fam.pos and fam.trim:
                    continue
                assert ((trig >= e - 240) & (trig < e)).any() and ((trig > e) & (trig <= e + 240)).any(), what
