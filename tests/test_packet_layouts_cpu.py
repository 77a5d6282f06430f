"""The packet layouts of tests/gpu_util.py (place_packets), without a GPU: the helper runs on numpy arrays in place of
device memory.  tests/test_gpu_packet_layouts.py trusts it to put every sample where the call's own arguments look for it
(d_raw + s * raw_stream_stride + f * raw_frame_stride + src_offset[c] + sample_bytes * i), to leave the 0x7F / 0x80 fill
everywhere else, and to give each layout the residues that decide whether lpcm_form() admits the call."""
import numpy as np
import pytest

import gpu_util as G
import lpcm_util as LP

NP = G.NumpyBackend()
S, F, M, FS = 3, 4, 3, 8
PERM = [2, 0, 1]
ALL = G.PK_LAYOUTS + [G.PK_FRAME_MAJOR]
SMALL = G.PK_SMALL + [G.PK_FRAME_MAJOR]


def _rows(sb):
    """every sample its own value, the extremes among them; head 8 / pad 8 (16 bit) or head 4 / pad 4 (24 bit)"""
    full = 1 << (8 * sb - 1)
    ints = (np.arange(S * F * M * FS, dtype=np.int64) * 2654435761 % (2 * full) - full).reshape(S, F, M, FS)
    ints[0, 0, 0, 0], ints[S - 1, F - 1, M - 1, FS - 1] = full - 1, -full
    raw, L, row = LP.rows(ints, sb, True, [1] * M, PERM, head=G.pk_grid(sb), pad=G.pk_grid(sb), frame_size=FS)
    return ints, raw, L, row


def _read(buf, at, sb):
    """little-endian, sign-extended"""
    v = sum(int(buf[at + k]) << (8 * k) for k in range(sb))
    return v - (1 << (8 * sb)) if v >> (8 * sb - 1) else v


class _Recording(G.NumpyBackend):
    """a backend that allocates nothing beyond the zones it is asked to write: {zone start: bytes}, for the far layouts"""

    def __init__(self):
        self.zones, self.size = {}, None

    def empty(self, n, dtype):
        assert dtype == np.uint8
        self.size = n
        return self

    def assign(self, t, start, host):
        assert t is self and start not in self.zones
        self.zones[start] = np.ascontiguousarray(host).reshape(-1).copy()

    def ptr(self, t):
        return 1 << 40          # 256-byte aligned, as device memory is


def _check_image(layout, sb, byte_at, placed_for):
    """the samples through the call's arguments for calls from frames 0 and 1; -> the set of run bytes"""
    ints, raw, L, row = _rows(sb)
    runs = set()
    for f0 in (0, 1):
        pl, base = placed_for(f0)
        for s in range(S):
            for f in range(F - f0):
                for c in range(M):
                    for i in range(FS):
                        at = pl.d_raw - base + s * pl.stream_stride + f * pl.frame_stride + L.src_offset[c] + sb * i
                        got = byte_at(at, sb)
                        assert got == ints[s, f0 + f, PERM[c], i], (layout.name, f0, s, f, c, i)
                        runs.update(range(at, at + sb))
    assert len(runs) == ints.size * sb
    return runs


@pytest.mark.parametrize("sb", [2, 3])
@pytest.mark.parametrize("layout", SMALL, ids=lambda l: l.name)
def test_every_sample_is_where_the_call_looks_and_the_rest_is_the_fill(layout, sb):
    ints, raw, L, row = _rows(sb)
    keep = G.place_packets(raw, L, layout, backend=NP).keep
    buf, p0 = keep.tensor, NP.ptr(keep.tensor)

    def placed_for(f0):
        pl = G.place_packets(raw, L, layout, f0, F - f0, backend=NP, keep=keep)
        assert pl.keep is keep, "one allocation for the calls of one programme"
        return pl, p0

    runs = _check_image(layout, sb, lambda at, n: _read(buf, at, n), placed_for)
    rest = np.ones(buf.size, dtype=bool)
    rest[sorted(runs)] = False
    assert np.array_equal(buf[rest], G.packet_fill(0, buf.size)[rest]), "every byte outside the runs is the fill"
    assert keep.zones == [(0, buf.size)] and keep.size == buf.size
    if layout == G.PK_DENSE:
        assert buf.size == S * F * row and keep.first == 0
    else:
        assert min(runs) >= row and buf.size - 1 - max(runs) >= row, "a row of slack in front and behind"


@pytest.mark.parametrize("sb", [2, 3])
@pytest.mark.parametrize("layout", G.PK_FAR, ids=lambda l: l.name)
def test_far_layouts_write_the_rows_and_their_guards_only(layout, sb):
    ints, raw, L, row = _rows(sb)
    rec = _Recording()
    keep = G.place_packets(raw, L, layout, backend=rec).keep
    assert rec.size == keep.size >= 1 << 28 and keep.tensor is rec
    assert sorted(rec.zones) == [lo for lo, hi in keep.zones]
    assert all(rec.zones[lo].size == hi - lo for lo, hi in keep.zones)
    assert all(a[1] < b[0] for a, b in zip(keep.zones, keep.zones[1:])), "zones neither overlap nor touch"
    assert sum(hi - lo for lo, hi in keep.zones) <= S * F * (row + 2 * G.FAR_GUARD)

    def byte(at):
        for lo, hi in keep.zones:
            if lo <= at < hi:
                return int(rec.zones[lo][at - lo])
        raise AssertionError("byte %d lies in no zone that was written" % at)

    def read(at, n):
        v = sum(byte(at + k) << (8 * k) for k in range(n))
        return v - (1 << (8 * n)) if v >> (8 * n - 1) else v

    def placed_for(f0):
        return G.place_packets(raw, L, layout, f0, F - f0, backend=rec, keep=keep), rec.ptr(rec)

    runs = _check_image(layout, sb, read, placed_for)
    off, fst, sst = G.packet_geometry(layout, S, F, row, sb)
    for lo, hi in keep.zones:
        z = rec.zones[lo]
        rest = np.ones(hi - lo, dtype=bool)
        rest[[a - lo for a in runs if lo <= a < hi]] = False
        assert np.array_equal(z[rest], G.packet_fill(lo, hi)[rest]), "within the guard zones every byte outside the runs is the fill"
    for s in range(S):                      # FAR_GUARD bytes on either side of every row (clipped to the allocation)
        for f in range(F):
            a = keep.first + s * sst + f * fst
            assert any(lo <= max(a - G.FAR_GUARD, 0) and min(a + row + G.FAR_GUARD, keep.size) <= hi for lo, hi in keep.zones)


@pytest.mark.parametrize("sb", [2, 3])
def test_the_geometry_is_the_table_of_the_layouts(sb):
    row, g = 1040, G.pk_grid(sb)
    assert g == (8 if sb == 2 else 4)
    B = G.pk_bound(3)
    want = {
        G.PK_DENSE: (0, row, F * row),
        G.PK_PAD16: (16, row + 16, F * (row + 16) + 48),
        G.PK_GRID: (16, row + g, F * (row + g) + g),
        G.PK_OFF_BASE: (8, row + 16, F * (row + 16)),
        G.PK_OFF_STRIDE: (0, row + g // 2, F * (row + g // 2)),
        G.PK_FAR_STREAMS: (16, row, 2 ** 31 + 16),
        G.PK_BOUND: (0, B, F * B),
        G.PK_BEYOND: (0, B + 16, F * (B + 16)),
        G.PK_FRAME_MAJOR: (16, S * (row + 16), row + 16),
    }
    assert set(want) == set(ALL)
    for layout, geo in want.items():
        assert G.packet_geometry(layout, S, F, row, sb) == geo, layout.name


def _admitted(d_raw, fst, sst, g):
    """lpcm_form()'s three address rules, restated: the base on 16 bytes, both strides on the grid"""
    return d_raw % 16 == 0 and fst % g == 0 and sst % g == 0


@pytest.mark.parametrize("sb", [2, 3])
@pytest.mark.parametrize("layout", G.PK_SMALL, ids=lambda l: l.name)
def test_residues_of_bases_and_strides(layout, sb):
    """what each layout is meant to keep or break, mod 16, mod g and mod g / 2, for the calls from frame 0 and frame 1"""
    ints, raw, L, row = _rows(sb)
    g = G.pk_grid(sb)
    pl0 = G.place_packets(raw, L, layout, 0, 1, backend=NP)
    pl1 = G.place_packets(raw, L, layout, 1, 3, backend=NP, keep=pl0.keep)
    p0 = NP.ptr(pl0.keep.tensor)
    assert p0 % 16 == 0, "numpy's allocation stands in for a 256-byte aligned device base"
    base = p0 + pl0.keep.first - G.packet_geometry(layout, S, F, row, sb)[0]
    assert (base - p0) % 256 == 0
    r0, r1 = (pl0.d_raw - p0) % 16, (pl1.d_raw - p0) % 16
    fst, sst = pl0.frame_stride, pl0.stream_stride
    assert (pl1.frame_stride, pl1.stream_stride) == (fst, sst) and pl1.d_raw - pl0.d_raw == fst
    assert sst >= F * fst, "frames of a stream before the next stream: the ABI's rule"
    fused = [_admitted(r, fst, sst, g) for r in (r0, r1)]
    if layout == G.PK_DENSE:
        assert (r0, r1, fst % 16, sst % 16) == (0, 0, 0, 0) and fused == [True, True]
    elif layout == G.PK_PAD16:
        assert (r0, r1, fst % 16, sst % 16) == (0, 0, 0, 0) and fst > row and sst > F * fst and fused == [True, True]
        assert (pl0.d_raw - p0) % 32 == 16 and sst % 32 == 16
    elif layout == G.PK_GRID:
        assert (r0, r1) == (0, g) and fst % 16 == g and fst % g == 0 and sst % g == 0 and sst % 16 != 0
        assert fused == [True, False]
    elif layout == G.PK_OFF_BASE:
        assert (r0, r1, fst % 16, sst % 16) == (8, 8, 0, 0) and fused == [False, False]
    elif layout == G.PK_OFF_STRIDE:
        assert r0 == 0 and fst % g == g // 2 and fst % (g // 2) == 0 and sst % (g // 2) == 0 and fused == [False, False]


@pytest.mark.parametrize("sb", [2, 3])
def test_far_layouts_arithmetic(sb):
    """no allocation: where the rows lie, and the 32-bit rule of fast_shape_ok in Python integers"""
    row = 16 * 1024 * sb + 16
    rule = lambda n, stride: (n + 2) * stride + 2 ** 24 < 2 ** 31
    B = G.pk_bound(3)
    assert B == 426141280 and B % 16 == 0
    assert rule(3, B) and not rule(3, B + 16), "B(3) is the last multiple of 16 within the rule"
    assert rule(1, B + 16), "the one-frame call of PK_BEYOND is still fused"
    for n in (1, 2, 3, 4, 7):
        assert G.pk_bound(n) % 16 == 0 and rule(n, G.pk_bound(n)) and not rule(n, G.pk_bound(n) + 16)
    off, fst, sst = G.packet_geometry(G.PK_FAR_STREAMS, S, F, row, sb)
    assert off % 16 == 0 and fst % 16 == 0 and sst % 16 == 0, "every alignment rule holds: only the distance is unusual"
    assert sst > 2 ** 31 - 1 and 2 * sst > 2 ** 32 - 1 and F * fst < sst      # stream 1: signed, stream 2: unsigned
    assert rule(3, fst)
    far_in = 4 * (3 * (2 ** 29 + 4) + 3 * (16 * 1024 + 4) + 2 * 16 * 1024)      # FAR_IN's allocation, tests/test_layouts_cpu.py
    for layout in G.PK_FAR:
        off, fst, sst = G.packet_geometry(layout, S, F, row, sb)
        assert sst >= F * fst and off % 16 == 0 and fst % 16 == 0 and sst % 16 == 0
        size = off + (S - 1) * sst + (F - 1) * fst + row + 2 * ((row + 255) & ~255)
        assert 2 ** 32 < size < far_in, (layout.name, size)


def test_the_fill_follows_the_byte_address_and_a_stray_load_is_loud():
    f = G.packet_fill(3, 11)
    assert list(f) == [0x80, 0x7F, 0x80, 0x7F, 0x80, 0x7F, 0x80, 0x7F]
    for at in (0, 1):
        for sb in (2, 3):
            v = abs(_read(G.packet_fill(at, at + sb), 0, sb))
            assert v >= 0.99 * (1 << (8 * sb - 1)), (at, sb, v)


def test_the_run_mask_names_the_runs_of_interleaved_and_missing_channels():
    ints = np.zeros((1, 1, 3, FS), dtype=np.int64)
    raw, L, row = LP.rows(ints, 2, True, [2, 1], [0, 1, 2], head=4, pad=2, frame_size=FS)
    used = G.packet_run_mask(L, row)
    assert used[4:4 + 2 * 2 * FS].all() and not used[:4].any() and not used[4 + 4 * FS:4 + 4 * FS + 2].any()
    assert int(used.sum()) == 3 * FS * 2
    L.src_offset[2] = -1
    assert int(G.packet_run_mask(L, row).sum()) == 2 * FS * 2


def test_the_members_of_a_fan_out_share_one_far_pcm_allocation():
    """gpu_util.pcm_rows_of_members under FAR_PCM: one allocation, every member's rows and guards clear of the others', the
    same stride and alignment for all; rows_and_rest of a member sees a byte written into its own guards and no other's"""
    class Zones(_Recording):
        def assign(self, t, start, host):
            self.zones[start] = np.ascontiguousarray(host).reshape(-1).copy()

        def read(self, t, lo, hi):
            return self.zones[lo][:hi - lo].copy()

    rec = Zones()
    needs, bpss = [4096, 2048, 6144, 4096], [2, 2, 3, 4]
    rows = G.pcm_rows_of_members(S, needs, G.FAR_PCM, bpss, backend=rec)
    assert all(r.tensor is rec and r.far for r in rows) and rec.size == rows[0].size
    assert all(r.stride == 2 ** 31 + 16 and r.d_pcm % 16 == 0 and r.size <= rec.size for r in rows)
    zones = sorted(z for r in rows for z in r._zones())
    assert len(zones) == S * len(rows) and all(a[1] <= b[0] for a, b in zip(zones, zones[1:])), "no two zones share a byte"
    assert rec.size < 2 * (2 ** 31 + 16) + 2 ** 21, "about 4 GiB for all members"
    for j, r in enumerate(rows):
        assert [o.size for o in G.rows_and_rest(r, G.FAR_PCM, 0)] == [0] * S
    lo, hi = rows[2]._zones()[1]
    rec.zones[lo][5] = 0
    with pytest.raises(AssertionError, match="outside the emitted runs"):
        G.rows_and_rest(rows[2], G.FAR_PCM, 0)
    for j in (0, 1, 3):
        G.rows_and_rest(rows[j], G.FAR_PCM, 0)
    small = G.pcm_rows_of_members(S, needs, G.PAD16, bpss, backend=NP)
    assert len({id(r.tensor) for r in small}) == len(needs) and not any(r.far for r in small)
