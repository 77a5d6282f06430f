"""The structured programmes of tests/programmes.py, without a GPU: the oracle reproduces the reference's pinned results
on every one of them (tests/golden/programmes.json, written by oracle/gen_golden_programmes.py), and each programme
still reaches the branch it is for, judged by the oracle's limiter trace and the oracle's demixer alone."""
import hashlib
import json
import os

import numpy as np
import pytest

import demix_cases as D
import oracle_lib as O
import programmes as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "programmes.json")
with open(GOLD) as _f:
    PINS = json.load(_f)
KEYS = sorted(k for k in PINS if not k.startswith("_"))
TRIG = O.LIM_TRIGGER
LENGTHS = (6144, 12288, 13000)    # the pins' length, the GPU tests' 12 frames of 1024 and their 13 frames of 1000


def _sizes(n, call):
    return [call] * (n // call) + ([n % call] if n % call else [])


def _trace(x, rate=48000, call=1024):
    with np.errstate(all="ignore"):
        return O.limiter_trace(x, _sizes(x.shape[1], call), rate=rate)


def _longest_run(mask):
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return int((e - s).max()) if len(s) else 0


def test_pins_cover_every_programme():
    assert "NaN" in PINS["_note"]
    named = {PINS[k]["programme"] for k in KEYS}
    assert named == {f.__name__ for f in P.LIMITER + P.DEMIXER} | {"retrigger_sweep", "attack_across_chunks"}
    for f in P.LIMITER:
        if f is not P.release_to_idle:
            assert {"limiter/%s/c%d" % (f.__name__, c) for c in (1024, 960)} <= set(KEYS)
    assert {"limiter/release_to_idle/%d/c1024" % r for r in P.RATES} <= set(KEYS)
    # the other rates (tests/test_gpu_rates.py): release_to_idle and the eight sweep streams at frames(rate) frames, and the
    # plateau pair at 0 and -6 dB
    for r in P.SWEEP_RATES:
        assert "limiter/release_to_idle/%d/f%d/c1024" % (r, P.frames(r)) in KEYS
        assert {"limiter/retrigger_sweep/%d/k%d/c1024" % (r, k) for k in range(P.SWEEP)} <= set(KEYS)
    assert {"limiter/attack_across_chunks/%d/c1024" % r for r in (48000,) + P.SWEEP_RATES} <= set(KEYS)
    for db in (0, -6):
        assert {"limiter/%s/%ddB/c1024" % (nm, db) for nm in ("dc_at_threshold", "dc_one_ulp_above")} <= set(KEYS)
    for f in P.LIMITER + P.DEMIXER + [P.retrigger_sweep, P.attack_across_chunks]:
        assert f.__doc__, f.__name__


@pytest.mark.parametrize("key", KEYS)
def test_oracle_reproduces_the_reference(key):
    pin = PINS[key]
    with np.errstate(all="ignore"):
        if key.startswith("limiter/"):
            x = getattr(P, pin["programme"])(pin["ch"], pin["n"], pin["rate"], **pin["args"])
            y, _ = O.limiter_run(x, _sizes(pin["n"], pin["call"]), rate=pin["rate"], **({"thr_db": pin["thr_db"]} if "thr_db" in pin else {}))
            assert y.shape == (pin["ch"], pin["out_len"])
        else:
            c = P.demix_case(pin["fs"])
            y = D.drive_demixer(O.lib(), "orc_demixer_", c, P.demix_input(getattr(P, pin["programme"]), c))
            assert y.shape[:2] == (pin["frames"], pin["ch"]) and y.size == pin["out_len"]
    assert hashlib.sha256(P.canonical_bytes(y)).hexdigest() == pin["sha256"]


def test_trace_is_the_limiter():
    """the traced entry computes what orc_limiter_process computes"""
    x = P.impulses(2, 6144)
    y, t = _trace(x)
    z, _ = O.limiter_run(x, _sizes(6144, 1024))
    assert np.array_equal(y.view(np.uint32), z.view(np.uint32)) and t.shape == (6144 + 240,)


# (rate, frames): the four rates of RELEASE_FRAMES at their lengths, and every rate of RATE_STEPS at frames(rate)
RELEASE_CASES = sorted({(r, P.RELEASE_FRAMES[r]) for r in P.RATES} | {(r, P.frames(r)) for r in P.SWEEP_RATES})
RELEASE_IDS = ["%d" % r if P.RELEASE_FRAMES.get(r) == f else "%d-f%d" % (r, f) for r, f in RELEASE_CASES]


def test_the_rates_are_what_they_are_for():
    """(n_atk, n_end) of every rate of tests/test_gpu_rates.py from limiter_steps, the library's f32 accumulation: both sides
    of the two staged windows (kWWin = 320 of render_wide.hpp, kFWin = 1088 of the others), n_atk % 4 of every kind, attacks
    of more than one, three and four 64-sample blocks.  A change of the window constants or of the accumulation shows here."""
    for table in (P.RATE_STEPS, P.WINDOW_RATES):
        for rate, steps in table.items():
            assert P.limiter_steps(rate) == steps, rate
    assert P.limiter_steps(1587)[1] == 320 - 1 and P.limiter_steps(1588)[1] == 320          # kWWin
    assert P.limiter_steps(5407)[1] == 1088 - 1 and P.limiter_steps(5408)[1] == 1088        # kFWin
    assert P.RATE_STEPS[8000][1] < 2 * 1024
    assert P.RATE_STEPS[22050][0] % 4 == 3 and P.RATE_STEPS[44100][0] % 4 == 1 and P.RATE_STEPS[44100][1] % 4 == 0
    assert 64 < P.RATE_STEPS[96000][0] and 3 * 64 < P.RATE_STEPS[192000][0] and 256 < P.RATE_STEPS[384000][0] > 240
    assert [P.frames(r) for r in P.SWEEP_RATES] == [4, 4, 7, 11, 22, 41, 78] and P.frames(48000) == 12
    for f in (4, 5, 7, 11, 12, 21, 22, 41, 78):
        c = P.cut_calls(f)
        assert sum(c) == f and min(c) >= 1 and c[:2] == [1, 3], (f, c)
    assert P.cut_calls(12) == [1, 3, 2, 5, 1] and P.cut_calls(21) == [1, 3, 2, 5, 1, 9]
    assert P.cut_calls(11) == [1, 3, 2, 4, 1] and P.cut_calls(5) == [1, 3, 1]


@pytest.mark.parametrize("rate,frames", RELEASE_CASES, ids=RELEASE_IDS)
def test_release_to_idle_runs_to_idle(rate, frames):
    n = 1024 * frames
    x = P.release_to_idle(2, n, rate)
    y, t = _trace(x, rate)
    trig, phase = (t & TRIG) != 0, t & 3
    assert trig.any()
    last_trig = int(np.flatnonzero(trig)[-1])
    n_atk, n_end = P.limiter_steps(rate)
    last_rel = int(np.flatnonzero(phase == O.LIM_RELEASE)[-1])
    assert last_rel == last_trig + n_end == P.release_last_step(rate, frames)
    assert (phase[last_trig + 1:last_trig + n_atk + 1] == O.LIM_ATTACK).all()
    assert (phase[last_trig + n_atk + 1:last_rel + 1] == O.LIM_RELEASE).all()      # the whole release curve, in one piece
    assert (phase[last_rel + 1:] == O.LIM_IDLE).all() and len(t) - (last_rel + 1) >= 1024
    # gain exactly 1.0 once idle (the output lags the input by 240 samples), and not before
    assert np.array_equal(y[:, last_rel + 1 - 240:].view(np.uint32), x[:, last_rel + 1 - 240:].view(np.uint32))
    assert not np.array_equal(y[:, last_rel - 1024 - 240:last_rel - 240], x[:, last_rel - 1024 - 240:last_rel - 240])
    # at least one whole 1024-chunk of the input starts idle and stays idle
    first_idle_chunk = -(-(last_rel + 1) // 1024)
    assert first_idle_chunk + 1 <= frames


@pytest.mark.parametrize("grid", [0, 16, 24], ids=["f32", "grid16", "grid24"])
@pytest.mark.parametrize("rate", (48000,) + P.SWEEP_RATES)
def test_retrigger_sweep_hits_the_phase_boundaries(rate, grid):
    """grid: the sweep on the 16- or 24-bit packet grid (programmes.on_packet_grid), as the packet-fed kernels render it"""
    n = 1024 * P.frames(rate)
    quant = (lambda x: P.on_packet_grid(x, grid)) if grid else (lambda x: x)
    n_atk, n_end = P.limiter_steps(rate)
    base = P.retrigger_sweep(2, n, rate, k=0)
    base[:, np.flatnonzero(base[0] == 3.0)] = 0.0      # the first impulse alone
    base = quant(base)
    _, t = _trace(base, rate)
    last_trig = int(np.flatnonzero(t & TRIG)[-1])
    last_atk = int(np.flatnonzero((t & 3) == O.LIM_ATTACK)[-1])
    last_rel = int(np.flatnonzero((t & 3) == O.LIM_RELEASE)[-1])
    assert last_trig == P.LAST_TRIGGER and last_atk == last_trig + n_atk and last_rel == last_trig + n_end
    hit = set()
    firsts = []
    for k in range(P.SWEEP):
        _, tk = _trace(quant(P.retrigger_sweep(2, n, rate, k=k)), rate)
        assert np.array_equal(tk[:last_trig + 1], t[:last_trig + 1])
        new = np.flatnonzero((tk & TRIG) & ~(t & TRIG))
        first = int(new[0])                                # the step the second impulse first triggers at
        assert not (tk[last_trig + 1:first] & TRIG).any()
        hit.add((first, int(tk[first] & 3)))
        firsts.append(first - last_trig)
    # the eight streams re-trigger on the last two attack, first two and last two release and first two idle steps
    assert firsts == [n_atk - 1, n_atk, n_atk + 1, n_atk + 2, n_end - 1, n_end, n_end + 1, n_end + 2]
    assert {(last_atk, O.LIM_ATTACK), (last_atk + 1, O.LIM_RELEASE), (last_rel, O.LIM_RELEASE),
            (last_rel + 1, O.LIM_IDLE)} <= hit, sorted(hit)


@pytest.mark.parametrize("rate", (48000,) + P.SWEEP_RATES)
def test_attack_across_chunks_starts_chunks_inside_the_attack(rate):
    n = 1024 * max(P.frames(rate), 4)
    n_atk, n_end = P.limiter_steps(rate)
    tails = P.attack_tails(n)
    assert len(tails) >= 3 and n_atk > max(j for _, j in tails)
    _, t = _trace(P.attack_across_chunks(2, n, rate), rate)
    trig, phase = (t & TRIG) != 0, t & 3
    seen = set()
    for c, j in tails:
        last = 1024 * c - j                              # the run's last trigger: j steps before the chunk
        assert trig[last - 239:last + 1].all() and not trig[last + 1:last + 700].any(), (rate, c)
        # the chunk's first n_atk - j steps are attack steps, the next one is a release step: the boundary lies in the chunk
        assert (phase[1024 * c:last + n_atk + 1] == O.LIM_ATTACK).all() and phase[last + n_atk + 1] == O.LIM_RELEASE, (rate, c)
        assert 0 < last + n_atk + 1 - 1024 * c < 1024
        seen.add((last + n_atk + 1) % 4)
    assert len(seen) >= 3                                # the boundary in three or four different places of a lane's quad


@pytest.mark.parametrize("n", LENGTHS)
def test_limiter_programmes_reach_their_branches(n):
    call = 1000 if n == 13000 else 1024
    trig = {f.__name__: (_trace(f(2, n), call=call)[1] & TRIG) != 0 for f in
            (P.silence, P.ramp_up, P.dc_at_threshold, P.dc_one_ulp_above, P.impulses, P.onset_after_silence, P.loud_then_silence,
             P.square_full_scale, P.square_4x, P.denormal)}
    assert _longest_run(trig["ramp_up"]) >= 2048
    assert not trig["dc_at_threshold"].any() and not trig["silence"].any() and not trig["denormal"].any()
    assert trig["dc_one_ulp_above"][240:].all()           # once the window is full: every step, the flush included
    assert trig["impulses"][n:].any()                     # during the flush
    assert trig["square_full_scale"][240:].all() and trig["square_4x"][240:].all()
    on = trig["onset_after_silence"]
    assert not on[:1358].any() and on[1358]               # the window's maximum was 0 up to the step before
    assert trig["loud_then_silence"][:1740].any() and not trig["loud_then_silence"][1741:].any()


def test_threshold_programmes_sit_on_the_threshold():
    """the threshold as the limiter derives it, (float)pow(10, -1.0f / 20); that the oracle's own threshold is this value is
    what dc_at_threshold (never a trigger) and dc_one_ulp_above (always one) show above"""
    assert P.THR == np.float32(10.0 ** (np.float32(-1.0) / np.float32(20.0)))
    assert P.dc_at_threshold(1, 4)[0, 0] == P.THR and P.dc_one_ulp_above(1, 4)[0, 0] == np.nextafter(P.THR, np.float32(2))


@pytest.mark.parametrize("rate,frames", RELEASE_CASES, ids=RELEASE_IDS)
def test_the_release_ends_on_steps_of_gain_one(rate, frames):
    """Why a shift of n_end by one step cannot show in any output, here or on the GPU: the last release steps have the curve
    value exactly 1.0f (ease() rounds to 1 once (x - 1)^2 < 2^-25), and ge + 1.0f * (1 - ge) is exactly 1.0f for every ge
    in (0, 1): fl(1 - ge) is off by at most 2^-25, and 1 - 2^-25 rounds to the even 1.0f.  So the step n_end - 1 has gain 1.0
    whether it counts as release or as idle, and a re-trigger there starts from gs = 1.0 either way.  Further back the
    curve is below 1 and the release programmes pin it: that is where a larger shift shows.
    How many steps that is grows with the rate: x advances by 1 / (0.2 * rate) per step, and (1 - x)^2 < 2^-25 holds for the
    last 0.2 * rate * 2^-12.5 steps (0.2 at 5408 Hz, 1.7 at 48 kHz, 13 at 384 kHz); the product with 1 - ge, which is
    below 1, rounds to 1 a little earlier still, by at most as much again."""
    n_atk, n_end = P.limiter_steps(rate)
    x = P.release_to_idle(2, 1024 * frames, rate)
    y, t = _trace(x, rate)
    last_rel = int(np.flatnonzero((t & 3) == O.LIM_RELEASE)[-1])
    same = (y[:, :last_rel + 1 - 240].view(np.uint32) == x[:, :last_rel + 1 - 240].view(np.uint32)).all(axis=0)
    tail = int(np.flatnonzero(~same)[-1]) + 240            # the last release step whose gain is not 1.0
    flat = 0.2 * rate * 2.0 ** -12.5
    print("rate %d: %d steps of gain 1.0 at the end of the release (curve alone: %.1f)" % (rate, last_rel - tail, flat))
    assert 1 <= last_rel - tail <= 2 * flat + 16, (rate, last_rel - tail)
    if rate in P.RATES:
        assert 2 <= last_rel - tail <= 16, (rate, last_rel - tail)      # the bound these four rates have always had


def test_one_times_the_rest_is_one():
    F = np.float32
    ge = np.concatenate([np.random.default_rng(5).uniform(0, 1, 200000), 2.0 ** -np.arange(1, 120)]).astype(F)
    assert (ge + F(1.0) * (F(1.0) - ge) == F(1.0)).all()


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("rate", (48000,) + P.SWEEP_RATES)
def test_packet_grid_programmes_reach_their_branches(rate, bits):
    """the programmes a packet-fed kernel gets (programmes.boundary_set on the packet grid): every sample is PACKET_WEIGHT
    times a packet integer over full scale, exactly; release_to_idle still runs its whole release and ends idle, the onset
    still meets a window of zeros, loud_then_silence still drops to 0 inside its release (the sweep:
    test_retrigger_sweep_hits_the_phase_boundaries)"""
    n = 1024 * P.frames(rate)
    n_atk, n_end = P.limiter_steps(rate)
    full = 2 ** (bits - 1)
    progs = dict(P.boundary_set(2, n, rate, packet_bits=bits))
    assert len(progs) == P.SWEEP + len(P.PACKET)
    for nm, x in progs.items():
        k = x.astype(np.float64) * (full / P.PACKET_WEIGHT)
        assert (k == np.rint(k)).all() and k.min() >= -full and k.max() <= full - 1, nm
        assert np.array_equal(P.from_packet_grid(P.to_packet_grid(x, bits), bits).view(np.uint32) & 0x7fffffff,
                              x.view(np.uint32) & 0x7fffffff), nm
    y, t = _trace(progs["release_to_idle"], rate)
    trig, phase = (t & TRIG) != 0, t & 3
    last_trig = int(np.flatnonzero(trig)[-1])
    last_rel = int(np.flatnonzero(phase == O.LIM_RELEASE)[-1])
    assert last_rel == last_trig + n_end and (phase[last_trig + n_atk + 1:last_rel + 1] == O.LIM_RELEASE).all()
    assert (phase[last_rel + 1:] == O.LIM_IDLE).all() and len(t) - (last_rel + 1) >= 1024
    on = (_trace(progs["onset_after_silence"], rate)[1] & TRIG) != 0
    assert not on[:1358].any() and on[1358]
    loud = (_trace(progs["loud_then_silence"], rate)[1] & TRIG) != 0
    assert loud[:1740].any() and not loud[1741:].any()
    assert not (_trace(progs["silence"], rate)[1] & TRIG).any()


@pytest.mark.parametrize("rate", [48000, 96000])
@pytest.mark.parametrize("db", [0.0, -6.0, -1.0])
def test_the_plateau_pair_sits_on_the_threshold(db, rate):
    """DC at thr(db) never triggers; one ulp above it triggers on every step once the window is full, the flush included.
    At 0 dB the threshold is exactly 1.0f."""
    assert P.thr(0.0) == np.float32(1.0) and P.thr(-1.0) == P.THR
    assert P.thr(db) == np.float32(10.0 ** float(np.float32(db) / np.float32(20.0)))
    n = 6144
    with np.errstate(all="ignore"):
        _, at = O.limiter_trace(P.dc_at_threshold(2, n, rate, db=db), _sizes(n, 1024), rate=rate, thr_db=db)
        _, above = O.limiter_trace(P.dc_one_ulp_above(2, n, rate, db=db), _sizes(n, 1024), rate=rate, thr_db=db)
    assert not (at & TRIG).any()
    assert ((above & TRIG) != 0)[240:].all()


@pytest.mark.parametrize("bd,scale,lo,hi", [(16, 32768.0, -32768.0, 32767.0), (24, 8388608.0, -8388608.0, 8388607.0),
                                            (32, 2147483648.0, -2147483648.0, 2147483647.0)])
def test_pack_edges_classes(bd, scale, lo, hi):
    cls = P.pack_edge_values()
    x = P.pack_edges(2, 1024)
    for name, vs in cls.items():
        for v in vs:
            for c in range(2):
                assert (x[c].view(np.uint32) == np.float32(v).view(np.uint32)).any(), (name, v)   # by bits: -0.0 too
    v = (x[0] * np.float32(scale)).astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    assert (v > hi).any() and (v < lo).any()              # both clamps
    for b in (lo, hi):                                    # and a neighbour on either side of each bound, and the bound
        assert (v < b).any() and (v > b).any() and (v == b).any()
        if bd < 32:                                       # (32 bit: the neighbours of 2^31 in f32 are 128 and 256 LSB away)
            assert b - v[v < b].max() <= 1 and v[v > b].min() - b <= 1, (bd, b)
    inside = v[(v > lo) & (v < hi)].astype(np.float64)
    frac = np.abs(inside) - np.floor(np.abs(inside))
    ties = inside[frac == 0.5]
    k = np.floor(np.abs(ties)).astype(np.int64)
    for sign in (1, -1):                                  # ties above an even and above an odd integer, both signs
        assert ((k % 2 == 0) & (np.sign(ties) == sign)).any() and ((k % 2 == 1) & (np.sign(ties) == sign)).any(), (bd, sign)
    assert (x[0].view(np.uint32) == 0x80000000).any() and (x[0] == 1.0).any() and (x[0] == -1.0).any()
    assert (np.abs(x[0]) == 1.5).any() and (np.abs(x[0]) == 100.0).any()
    # the oracle's packed values reach both ends of the format's range (32 bit: its upper bound is 2^31 in f32, which the
    # reference's conversion does not hold; what comes out there is pinned by the GPU comparison, not here)
    p = O.pack(x[:1], bd)
    if bd == 24:
        p = (p[..., 0].astype(np.int32) | (p[..., 1].astype(np.int32) << 8) | (p[..., 2].astype(np.int8).astype(np.int32) << 16))
    assert int(p.min()) == int(lo)
    if bd < 32:
        assert int(p.max()) == int(hi)


def test_demixer_programmes_leave_the_fast_quotient():
    """the quotient channels that reach the output (7.1.4: BL7 / BR7 = numerator / beta, HBL / HBR = numerator / gamma, then
    a recon gain of 120/255 .. 1): a quotient of 0 had a numerator of 0, one below 2^-103 a numerator below 2^-100, one of
    1.5 * 2^126 or more a numerator of at least 2^126 (divisors: 0.707 .. 1).  Per wave = 256 consecutive samples."""
    c = P.demix_case(1024)
    seen = {}
    with np.errstate(all="ignore"):
        for f in P.DEMIXER:
            o = D.drive_demixer(O.lib(), "orc_demixer_", c, P.demix_input(f, c))
            F, ch, fs = o.shape
            assert ch == 12 and np.isfinite(o).all(), f.__name__
            for pair in ((6, 7), (10, 11)):
                q = np.abs(o[:, pair, :].astype(np.float64)).transpose(0, 2, 1).reshape(F * fs // 256, 512)
                zero, tiny = (q == 0).any(1), ((q > 0) & (q < 2.0 ** -103)).any(1)
                huge, normal = (q >= 1.5 * 2.0 ** 126).any(1), ((q > 2.0 ** -90) & (q < 2.0 ** 120)).any(1)
                seen[f.__name__, pair] = (zero, tiny, huge, normal)
    any_of = lambda i: {k for k, v in seen.items() if v[i].any()}
    assert any_of(0) and any_of(1) and any_of(2)
    # in different waves: a wave of zeros only, one of tiny values only, one of huge values only
    assert any((v[0] & ~v[1] & ~v[2] & ~v[3]).any() for v in seen.values())
    assert any((v[1] & ~v[0] & ~v[2] & ~v[3]).any() for v in seen.values())
    assert any((v[2] & ~v[0] & ~v[1]).any() for v in seen.values())
    # and a wave that holds a mix: numerators out of the range beside normal ones
    assert any(((v[0] | v[1]) & v[3]).any() for v in seen.values())
    assert all(v[0].all() for k, v in seen.items() if k[0] == "dm_silence")


# ---- the demixer's quotients: what dropping div8's IEEE branch (render_wide4.hpp) could change ----

def _rn32(fr):
    """a Fraction rounded to the nearest float32, ties to even, subnormals and overflow included (as a Fraction; inf: None)"""
    from fractions import Fraction
    if fr == 0:
        return Fraction(0)
    a, e = abs(fr), 0
    while a >= 2:
        a, e = a / 2, e + 1
    while a < 1:
        a, e = a * 2, e - 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    k = abs(fr) / quantum
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    v = n * quantum
    if v >= Fraction(2) ** 128:
        return None
    return v if fr > 0 else -v


def _w4_quot(n, d, r):
    """w4_quot of render_common.hpp in exact arithmetic: q = n r; e = fma(-d, q, n); q' = fma(e, r, q)"""
    q = _rn32(n * r)
    if q is None:
        return None
    e = _rn32(n - d * q)
    return _rn32(e * r + q)


def test_the_quotients_fallback_cannot_show_in_16_bit_pcm():
    """render_wide4_kernel<.., DMX> divides the IEEE way when a wave holds a numerator of 0, below 2^-100 or from 2^126
    (div8), and its only output format is 16-bit PCM behind the limiter.  On those numerators the reciprocal form differs
    from the division by the sign of a zero, by less than 2^-120 in absolute terms on the tiny ones, and not at all on the
    huge ones whose quotient is finite — the demixer programmes' results are finite (asserted above).  A deviation of
    2^-120 in a quotient is absorbed by the first f32 sum with a normal term, and where every term is that small the
    sample is 0; it cannot move the limiter's peak across the threshold either.  So removing the branch is an equivalent
    mutation as far as any output of this kernel goes, and the demixer programmes on the GPU pin the branch's RESULT, not
    the choice of branch."""
    from fractions import Fraction
    rng = np.random.default_rng(77)
    for d32 in (np.float32(1.0), np.float32(0.707), np.float32(0.866)):
        d = Fraction(float(d32))
        r = Fraction(float(np.float32(1.0) / d32))
        mant = rng.integers(1 << 23, 1 << 24, size=400)
        tiny = [Fraction(int(m)) * Fraction(2) ** int(e) for m, e in zip(mant[:200], rng.integers(-149 - 23, -100 - 23, size=200))]
        tiny = [_rn32(t) for t in tiny] + [Fraction(2) ** -149, Fraction(2) ** -126, Fraction(2) ** -100 - Fraction(2) ** -124]
        huge = [Fraction(int(m)) * Fraction(2) ** int(e) for m, e in zip(mant[200:], rng.integers(126 - 23, 128 - 23, size=200))]
        for n in tiny:
            for s in (1, -1):
                ieee, got = _rn32(s * n / d), _w4_quot(s * n, d, r)
                assert abs(got - ieee) < Fraction(2) ** -120, (float(d32), float(n))
        checked = 0
        for n in huge:
            ieee = _rn32(n / d)
            if ieee is not None:                       # a finite quotient
                assert _w4_quot(n, d, r) == ieee and _w4_quot(-n, d, r) == -ieee, (float(d32), float(n))
                checked += 1
        assert checked >= 100
        assert _w4_quot(Fraction(0), d, r) == 0
