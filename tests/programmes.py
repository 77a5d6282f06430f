"""Named structured programmes: the signals whose VALUES steer the render kernels into branches noise never takes.

Every programme is a deterministic function (channels, n, rate) -> float32 [channels][n]; its docstring names the branch
it is for.  tests/test_programmes_cpu.py proves with the oracle's limiter trace (orc_limiter_process_trace) that each one
still reaches that branch, oracle/gen_golden_programmes.py pins the reference's results on them
(tests/golden/programmes.json), and tests/test_gpu_programmes.py feeds them to the kernels, one programme per stream.
Importing this module needs numpy only.
"""
import numpy as np

F32 = np.float32
THR = F32(10.0 ** (-1.0 / 20.0))          # the limiter's threshold at -1 dB, (float)pow(10, -1.0f / 20)
RATES = (48000, 44100, 16000, 96000)
# frames of 1024 of release_to_idle per rate: at least one whole 1024-chunk is idle after the release has ended
RELEASE_FRAMES = {48000: 12, 44100: 11, 16000: 5, 96000: 21}
# release_to_idle: the last gain step of the release per rate (the step input sample k enters at is step k; the output is
# 240 samples behind), recorded from the oracle's trace and asserted in tests/test_programmes_cpu.py
RELEASE_LAST_STEP = {48000: 10204, 44100: 9387, 16000: 3792, 96000: 19849}
BURST_AT, BURST_LEN = 100, 240
# the rates the limiter kernels are run at beside 48 kHz (tests/test_gpu_rates.py), with (n_atk, n_end) as limiter_steps
# gives them; tests/test_programmes_cpu.py asserts the table.  5408 Hz: n_end is the staged window of the fast, wide4 and
# fan-out kernels exactly (1088 words); 8000: a release shorter than two chunks; 22050 / 44100: n_atk % 4 = 3 / 1; 96000
# and up: an attack longer than one, three and four 64-sample blocks (384 kHz: than the 240-sample look-ahead).
RATE_STEPS = {5408: (6, 1088), 8000: (8, 1608), 22050: (23, 4433), 44100: (45, 8864), 96000: (97, 19298),
              192000: (193, 38574), 384000: (385, 77114)}
SWEEP_RATES = tuple(RATE_STEPS)
# both sides of the two window bounds: the last rate a kernel must refuse and the first it takes (kWWin = 320 of
# render_wide.hpp, kFWin = 1088 of the other vector kernels)
WINDOW_RATES = {1587: (2, 319), 1588: (2, 320), 5407: (6, 1087), 5408: (6, 1088)}
# release_to_idle at frames(rate) frames of 1024: the last release step, from the oracle's trace like RELEASE_LAST_STEP
# (the noise of channel 1 depends on the length, so 96 kHz has one entry per length)
RELEASE_LAST_STEP_AT = {(5408, 4): 1667, (8000, 4): 2187, (22050, 7): 4984, (44100, 11): 9387, (96000, 22): 19732,
                        (192000, 41): 39100, (384000, 78): 77693}


def _noise(seed, channels, n, sigma):
    x = np.random.default_rng(seed).standard_normal((channels, n)).astype(F32) * F32(sigma)
    return np.clip(x, -1.0, F32(1.0 - 2.0 ** -24)).astype(F32)


def _const(channels, n, v):
    return np.full((channels, n), v, dtype=F32)


def limiter_steps(rate):
    """(n_atk, n_end): after a trigger, gain steps 1..n_atk are attack steps, n_atk+1..n_end release steps and step
    n_end+1 is idle.  The time constant is accumulated in f32, one 1/rate per step, as the reference does."""
    inc, t, k = F32(1) / F32(rate), F32(0), 0
    atk, rel = F32(0.001), F32(0.200)
    n_atk = None
    while t < rel + atk:
        if n_atk is None and not t < atk:
            n_atk = k
        t = F32(t + inc)
        k += 1
    return n_atk, k


def frames(rate):
    """frames of 1024 that hold the re-trigger sweep at `rate` (its last impulse enters at LAST_TRIGGER + n_end + 2) and one
    more whole chunk, plus one: release_to_idle then ends at least one idle chunk before the end as well"""
    n_end = limiter_steps(rate)[1]
    return -(-(LAST_TRIGGER + n_end + 2 + 1024) // 1024) + 1


def release_frames(rate):
    """frames of release_to_idle: RELEASE_FRAMES where it has the rate, else frames(rate)"""
    return RELEASE_FRAMES.get(rate, frames(rate))


def release_last_step(rate, n_frames=None):
    """the last release step of release_to_idle(2, 1024 * n_frames, rate) as recorded from the oracle's trace"""
    n_frames = release_frames(rate) if n_frames is None else n_frames
    if RELEASE_FRAMES.get(rate) == n_frames:
        return RELEASE_LAST_STEP[rate]
    return RELEASE_LAST_STEP_AT[(rate, n_frames)]


_FIRST_CALLS = [1, 3, 2, 5, 1]
_CALLS_BY_FRAMES = {11: [1, 3, 2, 4, 1], 5: [1, 3, 1]}     # what the tests at 44.1 and 16 kHz have always used


def cut_calls(n_frames):
    """n_frames cut into calls: 1, 3, 2, 5, 1 as far as they fit, then the rest in one call, or in two of unequal length
    from ten frames on, so that chunk, call and release boundaries fall in different places"""
    if n_frames in _CALLS_BY_FRAMES:
        return list(_CALLS_BY_FRAMES[n_frames])
    out = []
    for c in _FIRST_CALLS:
        if sum(out) + c > n_frames:
            break
        out.append(c)
    rest = n_frames - sum(out)
    if rest >= 10:
        out += [rest // 3, rest - rest // 3]
    elif rest:
        out.append(rest)
    return out


def thr(db=-1.0):
    """the limiter's threshold as the library derives it: (float)pow(10, (float)db / 20), the quotient in f32"""
    return F32(10.0 ** float(F32(db) / F32(20.0)))


# ---- limiter programmes ----

def silence(channels, n, rate=48000):
    """all zeros: the chunk that starts and stays idle, pk == 0 everywhere; the demixer's zero numerators"""
    return np.zeros((channels, n), dtype=F32)


def onset_after_silence(channels, n, rate=48000):
    """zeros, then 1.0 from sample 1357 (no multiple of 64): the first trigger meets a window maximum that was 0"""
    x = np.zeros((channels, n), dtype=F32)
    x[:, 1357:] = 1.0
    return x


def loud_then_silence(channels, n, rate=48000):
    """1.3 for 1500 samples, then zeros: pk drops to 0 while the gain is still in its release"""
    x = np.zeros((channels, n), dtype=F32)
    x[:, :1500] = 1.3
    return x


def dc_at_threshold(channels, n, rate=48000, db=-1.0):
    """DC exactly at the threshold: peak * 1.0 > thr is false, no trigger ever"""
    return _const(channels, n, thr(db))


def dc_one_ulp_above(channels, n, rate=48000, db=-1.0):
    """DC one ulp above the threshold: a trigger on every step the window holds it at gain 1"""
    return _const(channels, n, np.nextafter(thr(db), F32(2)))


def _square(channels, n, amp):
    t = np.arange(n)
    x = np.where((t // 37) % 2 == 0, F32(amp), F32(-amp)).astype(F32)
    return np.tile(x, (channels, 1))


def square_full_scale(channels, n, rate=48000):
    """+-1.0 square, half period 37: the window maximum is a tie everywhere"""
    return _square(channels, n, 1.0)


def square_4x(channels, n, rate=48000):
    """+-4.0 square: ties, and the gain settles far below 1"""
    return _square(channels, n, 4.0)


def ramp_up(channels, n, rate=48000):
    """0 -> 2 over n: a new maximum every sample, one trigger run across blocks, chunks and calls"""
    return np.tile((np.arange(n, dtype=np.float64) * (2.0 / n)).astype(F32), (channels, 1))


def ramp_down(channels, n, rate=48000):
    """2 -> 0 over n: the maximum is always the oldest sample of the window"""
    return np.tile((2.0 - np.arange(n, dtype=np.float64) * (2.0 / n)).astype(F32), (channels, 1))


def impulse_positions(n):
    return [0, 239, 240, 1023, 1024, 1279, 1280, 2047, 2048, n - 241, n - 240, n - 120, n - 1]


def impulses(channels, n, rate=48000):
    """+-1.5 impulses on block (256), delay (240), chunk / call (1024) boundaries and in the last 240 samples, where the
    trigger run goes on in the flush; alternating channel and sign"""
    x = np.zeros((channels, n), dtype=F32)
    for i, p in enumerate(impulse_positions(n)):
        x[i % channels, p] = 1.5 if i % 2 == 0 else -1.5
    return x


def release_to_idle(channels, n, rate=48000):
    """one 240-sample 1.5 burst at 100..339 over noise of sigma 0.05: the whole release, down to gain exactly 1.0 and at
    least one idle chunk after it (n = 1024 * RELEASE_FRAMES[rate])"""
    x = _noise(4100, channels, n, 0.05)
    t = np.arange(BURST_AT, BURST_AT + BURST_LEN)
    x[:, t] += (F32(1.5) * np.where(t % 2 == 0, 1.0, -1.0)).astype(F32)
    return x


SWEEP = 8   # streams of retrigger_sweep


def retrigger_sweep(channels, n, rate=48000, k=0, last_trigger=None):
    """release_to_idle's noise with a single 1.5 impulse at 100 and a 3.0 impulse that makes gain step
    last_trigger + n_atk - 1 + k (k = 0..3: the last two attack and first two release steps) or
    last_trigger + n_end - 1 + (k - 4) (k = 4..7: the last two release and first two idle steps) trigger again.
    last_trigger: the step of the first run's last trigger, from the oracle's trace (LAST_TRIGGER)."""
    n_atk, n_end = limiter_steps(rate)
    t0 = LAST_TRIGGER if last_trigger is None else last_trigger
    step = t0 + (n_atk - 1 + k if k < 4 else n_end - 1 + (k - 4))
    x = _noise(4100, channels, n, 0.05)
    x[:, BURST_AT] = 1.5
    x[:, step - 1] = 3.0        # the sample enters the window after step - 1: the first step that sees it is `step`
    return x


def attack_tails(n):
    """[(chunk c, j)] of attack_across_chunks: chunks 1 .. 4 as far as n holds one more chunk behind them, j = c"""
    return [(c, c) for c in range(1, 5) if 1024 * (c + 1) <= n]


def attack_across_chunks(channels, n, rate=48000):
    """impulses of 1.5 * 2^(c-1) at 1024 c - 240 - c over noise of sigma 0.05, c = 1 .. 4: each triggers on every step it is in
    the window, the last one c steps before the 1024-chunk c; that chunk starts c steps into the attack, so its first
    hypothesis (no trigger in the chunk) changes from the attack to the release formula n_atk - c samples in: in another lane
    of a quad for every c, whatever n_atk % 4 is.  At the low rates the gain has all but settled by then (gs within an ulp or
    so of ge), and the two formulas differ by less than a 16-bit step: f32 output shows them apart."""
    x = _noise(4600, channels, n, 0.05)
    for c, j in attack_tails(n):
        x[:, 1024 * c - 240 - j] = 1.5 * 2.0 ** (c - 1)
    return x


# the step (= index of the input sample that enters at it) of the last trigger the lone 1.5 impulse at 100 causes: the
# gain approaches thr / 1.5 from above, so every step that has the impulse in its window triggers.  From the oracle's
# trace; tests/test_programmes_cpu.py asserts it.
LAST_TRIGGER = BURST_AT + 240


# ---- the packet grid: what an LPCM-fed kernel can be given ----
# Packets cannot carry samples beyond full scale, so a packet-fed family gets a programme divided by 4 and rounded to the
# packet's integers, and renders it through a selection matrix of weight 4.0: a power of two, so every product is exact and
# the rendered signal is from_packet_grid(to_packet_grid(x)).  tests/test_programmes_cpu.py proves from the oracle's trace
# that the sweep still hits its four boundaries on that grid.
PACKET_WEIGHT = 4.0
PACKET = ["release_to_idle", "onset_after_silence", "loud_then_silence", "silence"]     # and the eight sweep streams


def to_packet_grid(x, bits=16):
    """[..] float32 -> int64 packet samples of x / PACKET_WEIGHT"""
    full = 2 ** (bits - 1)
    q = np.rint(np.asarray(x, dtype=np.float64) * (full / PACKET_WEIGHT))
    return np.clip(q, -full, full - 1).astype(np.int64)


def from_packet_grid(ints, bits=16):
    """the signal a weight of PACKET_WEIGHT renders from those packet samples, exact in f32"""
    return ((np.asarray(ints).astype(np.float64) / 2 ** (bits - 1)).astype(F32) * F32(PACKET_WEIGHT)).astype(F32)


def on_packet_grid(x, bits=16):
    return from_packet_grid(to_packet_grid(x, bits), bits)


def boundary_set(m, n, rate=48000, packet_bits=0):
    """[(name, x [m][n])]: the eight sweep streams, release_to_idle, onset_after_silence, loud_then_silence and silence
    (tests/test_gpu_rates.py, every family but the five limiter copies); packet_bits: on that packet grid"""
    out = [("retrigger_sweep_k%d" % k, retrigger_sweep(m, n, rate, k=k)) for k in range(SWEEP)]
    out += [(nm, globals()[nm](m, n, rate)) for nm in PACKET]
    if packet_bits:
        out = [(nm, on_packet_grid(x, packet_bits)) for nm, x in out]
    return out


def pack_edge_values():
    """{class: [values]} of pack_edges"""
    def both(v):
        return [F32(v), F32(-v)]
    c = {}
    c["tie16"] = [y for k in (0, 1, 2, 3, 100, 101, 32765, 32766) for y in both((k + 0.5) / 32768.0)]
    c["tie24"] = [y for k in (0, 1, 2, 3, 1000, 1001, 8388605, 8388606) for y in both((k + 0.5) / 8388608.0)]
    c["tie32"] = [y for k in (0, 1, 2, 3) for y in both((k + 0.5) / 2.0 ** 31)]
    c["unit"] = [F32(1.0), F32(-1.0), F32(1.0 - 2.0 ** -24), F32(-1.0 - 2.0 ** -23)]
    c["beyond"] = both(1.5) + both(100.0) + [F32(-0.0)]
    edge = []
    for scale, hi, lo in ((32768.0, 32767.0, -32768.0), (8388608.0, 8388607.0, -8388608.0),
                          (2147483648.0, 2147483647.0, -2147483648.0)):
        for b in (F32(F32(hi) / F32(scale)), F32(F32(lo) / F32(scale))):
            edge += [np.nextafter(b, F32(-4)), b, np.nextafter(b, F32(4))]
    c["edge"] = edge
    return c


def pack_edges(channels, n, rate=48000):
    """rounding ties of the three integer formats, +-1.0 and its neighbours, values beyond full scale, -0.0 and both
    neighbours of each format's clamp bounds: for the pack code behind a limiter that stays at gain 1 (threshold 60 dB)
    or is off.  Channel c starts c values further on in the list."""
    v = np.array([y for vs in pack_edge_values().values() for y in vs], dtype=F32)
    return np.stack([np.resize(np.roll(v, -c), n) for c in range(channels)]).astype(F32)


def denormal(channels, n, rate=48000):
    """1e-40 for the first half, then 1e-39 * noise: subnormal input, for f32 output"""
    x = (_noise(4200, channels, n, 1.0).astype(np.float64) * 1e-39).astype(F32)
    x[:, :n // 2] = F32(1e-40)
    return x


def loud(channels, n, rate=48000):
    """1e4 * noise, then 1e30 DC whose sign differs per channel: input far beyond full scale"""
    x = (_noise(4300, channels, n, 0.3) * F32(1e4)).astype(F32)
    for c in range(channels):
        x[c, n // 2:] = F32(1e30) if c % 2 == 0 else F32(-1e30)
    return x


def nonfinite(channels, n, rate=48000):
    """noise of sigma 0.3 with one NaN, one +inf and one -inf in different channels and chunks, and one stretch of
    alternating +-3e38 whose matrix sums overflow; n >= 4096"""
    x = _noise(4400, channels, n, 0.3)
    x[0, 700] = np.nan
    x[1 % channels, 1024 + 333] = np.inf
    x[2 % channels, 3 * 1024 + 1] = -np.inf
    t0 = min(4 * 1024 + 500, n - 564)         # (four frames, the shortest programmes: the stretch ends the fourth chunk)
    t = np.arange(t0, t0 + 64)
    x[:, t] = (F32(3e38) * np.where(t % 2 == 0, 1.0, -1.0)).astype(F32)
    return x


def dc_1e30(channels, n, rate=48000):
    """1e30 DC, sign per channel: thr / peak underflows towards 0"""
    return np.stack([_const(1, n, 1e30 if c % 2 == 0 else -1e30)[0] for c in range(channels)])


def alternating_3e38(channels, n, rate=48000):
    """+-3e38 on every sample"""
    t = np.arange(n)
    return np.tile((F32(3e38) * np.where(t % 2 == 0, 1.0, -1.0)).astype(F32), (channels, 1))


def dc_1e_40(channels, n, rate=48000):
    """subnormal DC"""
    return _const(channels, n, 1e-40)


# programmes the limiter itself is pinned on (oracle/gen_golden_programmes.py), in file order
LIMITER = [silence, onset_after_silence, loud_then_silence, dc_at_threshold, dc_one_ulp_above, square_full_scale, square_4x,
           ramp_up, ramp_down, impulses, dc_1e30, alternating_3e38, dc_1e_40, nonfinite, loud, denormal, release_to_idle]
# the finite ones a limiter kernel is fed with a selection matrix (nonfinite is added where the kernel takes it)
LIMITER_FINITE = [silence, onset_after_silence, loud_then_silence, dc_at_threshold, dc_one_ulp_above, square_full_scale,
                  square_4x, ramp_up, ramp_down, impulses, release_to_idle, loud]


# ---- demixer programmes: what the decoded layers hold ----

def _dm_base(channels, n):
    return np.random.default_rng(4500).uniform(-0.9, 0.9, size=(channels, n)).astype(F32)


def dm_silence(channels, n, rate=48000):
    """every numerator of every wave is 0"""
    return np.zeros((channels, n), dtype=F32)


def dm_gap(channels, n, rate=48000):
    """a gap of zeros at 200..799, inside a chunk: waves that are silent, waves that are partly silent, waves that are not"""
    x = _dm_base(channels, n)
    x[:, 200:800] = 0.0
    return x


def dm_three_silent(channels, n, rate=48000):
    """three decoded channels silent"""
    x = _dm_base(channels, n)
    x[[0, 2, 5][:max(1, min(3, channels - 1))]] = 0.0
    return x


def dm_tiny(channels, n, rate=48000):
    """x 1e-33: numerators below 2^-100"""
    return (_dm_base(channels, n) * F32(1e-33)).astype(F32)


def dm_subnormal(channels, n, rate=48000):
    """x 1e-39: subnormal samples"""
    return (_dm_base(channels, n).astype(np.float64) * 1e-39).astype(F32)


def dm_huge(channels, n, rate=48000):
    """x 4e37: numerators of 2^126 and more, every intermediate still finite (x 2e37 leaves the quotients that reach the
    output short of the size at which their numerators are provably 2^126 or more)"""
    return (_dm_base(channels, n) * F32(4e37)).astype(F32)


def dm_mixed(channels, n, rate=48000):
    """zero, tiny and normal samples in turn: every wave holds a mix"""
    x = _dm_base(channels, n)
    t = np.arange(n)
    x[:, t % 3 == 0] = 0.0
    x[:, t % 3 == 1] *= F32(1e-33)
    return x.astype(F32)


def dm_equal(channels, n, rate=48000):
    """all channels equal: differences of channels are exactly 0"""
    return np.tile(_dm_base(1, n), (channels, 1))


DEMIXER = [dm_silence, dm_gap, dm_three_silent, dm_tiny, dm_subnormal, dm_huge, dm_mixed, dm_equal]


def demix_case(fs):
    """the scalable element the demixer programmes are decoded layers of: stereo -> 5.1.2 -> 7.1.4 with output gains and
    recon gains (demix_cases.make_case), 4 frames of 1024 or 8 of 256"""
    import demix_cases as D
    c = D.make_case([1, 3, 7], {0: (0b110000, 0.7079458), 1: (0b001111, 1.4125376)}, offset=40 if fs == 1024 else 8, fs=fs,
                    seed=770)
    c["schedule"] = c["schedule"][:4096 // fs if fs == 1024 else 8]
    return c


def demix_input(f, c):
    """programme f as the case's decoded channels, [frames][channels][fs]"""
    ch, fs, F = len(c["order"]), c["fs"], len(c["schedule"])
    return np.ascontiguousarray(f(ch, F * fs).reshape(ch, F, fs).transpose(1, 0, 2))


def canonical_bytes(a):
    """the bytes of a float32 array with every NaN replaced by the one quiet NaN 0x7fc00000 (payloads and signs of NaN
    differ between compilers and machines; their positions do not)"""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b.tobytes()
