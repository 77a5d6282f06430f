"""iamf_hip_batch_render_fanout_lpcm and iamf_hip_batch_render_fanout_range: one element held as LPCM packets rendered into
several batches, the packets read once (render_fanout_kernel<M, K, LP>, iac_amd/csrc/render_fanout.hpp).

Expected bytes come from two independent sources and both are asserted: (a) TWIN batches of the same configuration driven
by K single iamf_hip_batch_render_lpcm_range calls on the same packets; (b) for s16 members the oracle
(oracle_lib.stream_run) on x = ints / 32768.  Equality is exact: PCM bytes, n_emitted, every member's flush tail.  The
report and both launch tallies are asserted wherever a kernel is named, so no test here passes by another route.

Inputs: even streams loud, odd streams quiet (fanout_lpcm_util.ints16), packet rows with head 8, pad 8 and reversed channel
order.  assert_condition runs on the CPU before any GPU call: every loud stream exceeds every member's threshold in every
1024-sample chunk and no quiet stream ever does."""
import hashlib

import numpy as np
import pytest
import torch

import fanout_lpcm_util as U
import iac_amd as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

BAD_ARG, TOO_SMALL, INVALID_STATE = -1, -2, -5
MEMBERS = U.MEMBERS


def mats(element, layout):
    """(product matrix, oracle matrix) of an element into a layout"""
    if element in U.ORDER:
        return A.get_h2m_matrix(U.ORDER[element], A.SS[layout]), O.get_h2m(U.ORDER[element], O.SS[layout])
    return A.get_m2m_matrix(A.SS[element], A.SS[layout]), O.get_m2m(O.SS[element], O.SS[layout])


def assert_condition(element, specs, x, chunk=1024):
    for sp in specs:
        oc = A.layout_channels(A.SS[sp["layout"]])
        omx = mats(element, sp["layout"])[1]
        thr = 10.0 ** (sp["thr_db"] / 20.0)
        g = U.gain_product(sp)
        assert 0.7 <= g <= 1.25
        for s in range(x.shape[0]):
            y = np.abs(O.render(omx, x[s], oc)).max(axis=0) * g
            peaks = [float(y[c0:c0 + chunk].max()) for c0 in range(0, y.size, chunk)]
            print("condition %s -> %s %.0f dB stream %d (%s): chunk peaks %.3f .. %.3f against %.3f"
                  % (element, sp["layout"], sp["thr_db"], s, "loud" if s % 2 == 0 else "quiet", min(peaks), max(peaks), thr))
            if s % 2 == 0:
                assert min(peaks) > thr, (element, sp["layout"], s, min(peaks), thr)
            else:
                assert max(peaks) < thr, (element, sp["layout"], s, max(peaks), thr)


def assert_oracle(d, element, specs, x, fs):
    """s16 members against the oracle, stream by stream; x: [S][m][samples] = what was rendered"""
    for j, sp in enumerate(specs):
        if sp["fmt"] != A.FMT_S16:
            continue
        oc = d.batches[j].oc
        omx = mats(element, sp["layout"])[1]
        for s in range(d.S):
            want = O.stream_run(omx, oc, x[s], fs, element_gain=sp["eg"], output_gain=sp["og"], loudness_on=int(sp["lg"] is not None),
                                loudness_gain=sp["lg"] if sp["lg"] is not None else 1.0, limiter_on=int(sp["limiter"]), thr_db=sp["thr_db"])
            assert np.array_equal(d.bytes_of(j, s).view(np.int16).reshape(-1, oc), want), "member %d stream %d differs from the oracle" % (j, s)


def pair(element, specs, S, F, fs, bps=2, le=True, condition=None):
    """(got, twin, x): two drives on the same packets"""
    m = U.CHANNELS[element]
    raw, L, row, x = U.reversed_rows(U.ints16(S, F, m, fs, bps=bps), fs, bps, le)
    assert_condition(element, specs if condition is None else condition, x)
    mxs = [mats(element, sp["layout"])[0] for sp in specs]
    return U.Drive(mxs, specs, raw, L, row, x, fs), U.Drive(mxs, specs, raw, L, row, x, fs), x


def reset_tallies():
    A.route_reset()
    A.route_tally_ext(reset=True)


def lpcm_rows(tally):
    return {k: v for k, v in tally.items() if k[0] == "LPCM"}


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("element", ["foa", "soa", "toa"])
def test_shared_packet_kernel_parity(element, K):
    """a lone chunk, prefetch across chunks and frames, state carried over"""
    S, fs, calls = 4, 1024, [1, 3, 2]
    specs = MEMBERS[:K]
    m = U.CHANNELS[element]
    got, twin, x = pair(element, specs, S, sum(calls), fs)
    reset_tallies()
    for nf in calls:
        assert got.fan(nf) == (K, 1, 0)
    got.flush()
    assert A.route_tally_ext() == {("FANOUT_LPCM", 0, m, 0, K): len(calls)}
    assert A.route_tally() == {("GENERIC", 0, m, 0, 0): K}       # the members' flushes and nothing else: no NONE row
    for nf in calls:
        twin.single(nf)
    twin.flush()
    single = A.route_tally()
    assert single.pop(("GENERIC", 0, m, 0, 0)) == K and sum(single.values()) == K * len(calls)
    assert all(k[0] == "LPCM" and k[2] == m for k in single), single
    assert A.route_tally_ext() == {}
    U.assert_same(got, twin)
    assert_oracle(got, element, specs, x, fs)
    got.close()
    twin.close()


def test_frames_that_are_not_whole_chunks():
    """3072 samples: lanes divide by the frame size; 192: less than the 256 samples of saved state; 960: a short last chunk"""
    S, fs, K, calls = 4, 192, 3, [16, 1, 5, 2]
    specs = MEMBERS[:K]
    got, twin, x = pair("toa", specs, S, sum(calls), fs)
    reset_tallies()
    for nf in calls:
        assert got.fan(nf) == (K, 1, 0)
        twin.single(nf)
    assert A.route_tally_ext() == {("FANOUT_LPCM", 0, 16, 0, K): len(calls)}
    got.flush()
    twin.flush()
    U.assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_one_state_format():
    """packet fan-out -> single LPCM calls -> f32 fan-out on the same samples as f32 -> packet fan-out -> flush"""
    S, fs, K = 4, 1024, 4
    specs = [U.A_S16, U.A_GAINS_S24, U.MONO_S32_M9, U.member("A", fmt=A.FMT_F32, eg=1.2)]
    got, twin, x = pair("toa", specs, S, 6, fs)
    reset_tallies()
    assert got.fan(2) == (K, 1, 0)
    got.single(1)
    assert got.fan_f32(1) == K
    assert got.fan(2) == (K, 1, 0)
    got.flush()
    assert A.route_tally_ext() == {("FANOUT_LPCM", 0, 16, 0, K): 2}
    base = A.route_tally()
    assert base.pop(("FANOUT", 0, 16, 0, K)) == 1 and base.pop(("GENERIC", 0, 16, 0, 0)) == K
    assert sum(lpcm_rows(base).values()) == K and len(lpcm_rows(base)) == len(base), base
    for nf in (2, 1, 1, 2):
        twin.single(nf)
    twin.flush()
    U.assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_trim_and_an_off_grid_position():
    """A trimmed first frame of 1000 samples is no call of the packet-fed kernels (they take whole 64-sample blocks: the single
    call unpacks and renders on the general kernel), so by the entry's rules every member needs f32 and the packets are
    unpacked once: report (0, 0, 1).  (The issue's text expects (0, 0, 0) and single fused calls for this call; with 1000
    samples neither the single call nor the rules it states give that.)  The streams then stand at 1000 — neither a multiple
    of 16 nor below 240 — and whole frames are fused there; so is a trim of 896 samples from sample 60."""
    S, fs, K = 4, 1024, 3
    specs = MEMBERS[:K]
    got, twin, x = pair("toa", specs, S, 4, fs)
    reset_tallies()
    assert got.fan(1, first=24, n_samples=1000) == (0, 0, 1)
    assert A.route_tally_ext() == {} and A.route_tally() == {("GENERIC", 0, 16, 0, 0): K}
    assert got.fan(2) == (K, 1, 0)
    assert got.fan(1, first=60, n_samples=896) == (K, 1, 0)
    assert A.route_tally_ext() == {("FANOUT_LPCM", 0, 16, 0, K): 2} and A.route_tally() == {}
    got.flush()
    twin.single(1, first=24, n_samples=1000)
    twin.single(2)
    twin.single(1, first=60, n_samples=896)
    twin.flush()
    U.assert_same(got, twin)
    kept = np.concatenate([x[:, :, 24:1024], x[:, :, 1024:3072], x[:, :, 3072 + 60:3072 + 60 + 896]], axis=2)
    assert_oracle(got, "toa", specs, kept, fs)
    got.close()
    twin.close()


def run_mixed(got, twin, calls):
    """-> (reports, ext tally, base tally of got, base tally of the twin); flushes included"""
    reset_tallies()
    reports = [got.fan(nf) for nf in calls]
    got.flush()
    ext, base = A.route_tally_ext(), A.route_tally()
    for nf in calls:
        twin.single(nf)
    twin.flush()
    return reports, ext, base, A.route_tally()


def test_mixed_wide_members_beside_the_shared_pair():
    S, fs, calls = 4, 1024, [2, 1]
    specs = [U.A_S16, U.MONO_S16_M6, U.member("B"), U.member("J", fmt=A.FMT_S24)]
    got, twin, x = pair("toa", specs, S, sum(calls), fs, condition=specs[:2])
    reports, ext, base, single = run_mixed(got, twin, calls)
    assert reports == [(2, 1, 1)] * len(calls)
    assert ext == {("FANOUT_LPCM", 0, 16, 0, 2): len(calls)}
    # the wide members run what their single calls run; the pair's single calls are the twin's only LPCM rows
    assert sum(lpcm_rows(single).values()) == 2 * len(calls) and not lpcm_rows(base)
    assert base == {k: v for k, v in single.items() if k[0] != "LPCM"}     # (the four flushes included)
    U.assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_mixed_24_bit_packets_take_the_f32_fan_out():
    S, fs, calls, K = 4, 1024, [2, 1], 3
    specs = MEMBERS[:K]
    got, twin, x = pair("toa", specs, S, sum(calls), fs, bps=3, le=False)
    reports, ext, base, single = run_mixed(got, twin, calls)
    assert reports == [(K, 0, 1)] * len(calls)
    assert ext == {}
    assert base == {("FANOUT", 0, 16, 0, K): len(calls), ("GENERIC", 0, 16, 0, 0): K}
    assert not lpcm_rows(single)
    U.assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_mixed_coupled_element_takes_the_f32_fan_out():
    """a 5.1 element in 16 bit, its L/R and Ls/Rs pairs as coupled sub-streams, into {A, MONO}"""
    import lpcm_util as LP
    S, fs, calls = 4, 1024, [2, 1]
    specs = [U.A_S16, U.MONO_S16_M6]
    ints = U.ints16(S, sum(calls), 6, fs)
    perm = [0, 1, 4, 5, 2, 3]
    raw, L, row = LP.rows(ints, 2, True, [2, 2, 1, 1], perm, head=8, pad=8, frame_size=fs)
    x = U.decoded(ints, perm)
    assert_condition("L51", specs, x)
    mxs = [mats("L51", sp["layout"])[0] for sp in specs]
    got, twin = U.Drive(mxs, specs, raw, L, row, x, fs), U.Drive(mxs, specs, raw, L, row, x, fs)
    reports, ext, base, single = run_mixed(got, twin, calls)
    assert reports == [(2, 0, 1)] * len(calls)
    assert ext == {}
    assert base == {("FANOUT", 0, 6, 0, 2): len(calls), ("GENERIC", 0, 6, 0, 0): 2}
    U.assert_same(got, twin)
    assert_oracle(got, "L51", specs, x, fs)
    got.close()
    twin.close()


def test_mixed_limiter_on_and_off():
    S, fs, calls = 4, 1024, [2, 1]
    specs = [U.A_S16, U.member("A", limiter=False)]
    got, twin, x = pair("toa", specs, S, sum(calls), fs, condition=specs[:1])
    reports, ext, base, single = run_mixed(got, twin, calls)
    assert reports == [(0, 0, 1)] * len(calls)
    assert ext == {}
    # one LPCM row and one NOLIM row; the flush of the member with the limiter
    assert base == {("LPCM", 1, 16, 2, 0): len(calls), ("NOLIM", 0, 16, 0, 0): len(calls), ("GENERIC", 0, 16, 0, 0): 1}
    assert base == single
    U.assert_same(got, twin)
    assert got.emitted[0][0] == 2 * fs - 240 and got.emitted[1][0] == 2 * fs   # 240 withheld by the limiter's look-ahead
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


@pytest.mark.parametrize("entry", ["lpcm", "f32"])
def test_ranges(entry):
    S, fs, K = 6, 1024, 3
    specs = MEMBERS[:K]
    got, twin, x = pair("toa", specs, S, 3, fs)
    fan = (lambda *a, **k: got.fan(*a, **k)[0]) if entry == "lpcm" else got.fan_f32
    single = twin.single if entry == "lpcm" else twin.single_f32
    reset_tallies()
    assert fan(2, s0=0, cnt=3) == K
    # a range spanning two positions: refused, nothing changes
    caps, pcms = got.bufs(fs)
    ptrs = [p.data_ptr() for p in pcms]
    sentinel = A.FanoutReport(-7, -7, -7, -7)
    with pytest.raises(A.IamfHipError) as e:
        if entry == "lpcm":
            A.render_fanout_lpcm(got.batches, got.lpcm_input(0), 1, ptrs, caps, got.st, stream0=0, n_streams=S, report=sentinel)
        else:
            A.render_fanout_range(got.batches, got.xin.data_ptr(), got.F * got.m * fs, got.m * fs, 1, ptrs, caps, 0, S, got.st)
    assert e.value.code == INVALID_STATE
    assert (sentinel.n_fused, sentinel.input_fused, sentinel.n_unpacks, sentinel.reserved) == (-7, -7, -7, -7)
    torch.cuda.synchronize()
    assert all(bool((p == U.FILL).all()) for p in pcms)
    assert fan(1, s0=3, cnt=3) == K
    assert fan(1, s0=3, cnt=3) == K
    assert fan(1) == K
    got.flush()
    if entry == "lpcm":
        assert A.route_tally_ext() == {("FANOUT_LPCM", 0, 16, 0, K): 4} and A.route_tally() == {("GENERIC", 0, 16, 0, 0): K}
    else:
        assert A.route_tally_ext() == {} and A.route_tally() == {("FANOUT", 0, 16, 0, K): 4, ("GENERIC", 0, 16, 0, 0): K}
    single(2, s0=0, cnt=3)
    single(1, s0=3, cnt=3)
    single(1, s0=3, cnt=3)
    single(1)
    twin.flush()
    U.assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_refusals_change_nothing():
    S, fs = 4, 1024
    specs = [U.A_S16, U.MONO_S16_M6]
    got, twin, x = pair("toa", specs, S, 4, fs)
    assert got.fan(1) == (2, 1, 0)
    twin.single(1)
    caps, pcms = got.bufs(fs)
    ptrs = [p.data_ptr() for p in pcms]
    good = got.lpcm_input(1)

    def refused(batches, code, inp=None, caps_=None, ptrs_=None, n_samples=0):
        """every buffer and stride of the call is valid for its member unless the case says otherwise"""
        pp, cc = ptrs_ or ptrs, caps_ or caps
        assert len(pp) == len(cc) == len(batches) and all(pp)
        sentinel = A.FanoutReport(-7, -7, -7, -7)
        with pytest.raises(A.IamfHipError) as e:
            A.render_fanout_lpcm(batches, inp or good, 1, pp, cc, got.st, n_samples=n_samples, report=sentinel)
        assert e.value.code == code, (e.value.code, code)
        assert (sentinel.n_fused, sentinel.input_fused, sentinel.n_unpacks, sentinel.reserved) == (-7, -7, -7, -7)

    def with_layout(**kw):
        inp = got.lpcm_input(1)
        for k, v in kw.items():
            setattr(inp.layout, k, v)
        return inp

    a, b = got.batches
    refused([a, b], BAD_ARG, with_layout(channels=15))
    refused([a, b], BAD_ARG, with_layout(frame_size=960))
    refused([a, b], BAD_ARG, with_layout(sample_bytes=5))
    refused([a, b], BAD_ARG, got.lpcm_input(1, first=8))          # a trimmed start needs n_samples
    mono = mats("toa", "MONO")[0]
    other_streams = U.make_batch(mono, specs[1], S + 1, fs)
    other_m = U.make_batch(mats("foa", "MONO")[0], specs[1], S, fs)
    other_fs = U.make_batch(mono, specs[1], S, 960)
    ahead = U.make_batch(mono, specs[1], S, fs)
    big = torch.zeros((S, 2 * caps[1]), dtype=torch.uint8, device="cuda")
    ss, fstr = got.F * got.m * fs, got.m * fs
    ahead.render(got.xin.data_ptr(), ss, fstr, 2, big.data_ptr(), 2 * caps[1], got.st)    # stands at 2 frames, `a` at 1
    flushed = U.make_batch(mono, specs[1], S, fs)
    flushed.render(got.xin.data_ptr(), ss, fstr, 1, big.data_ptr(), 2 * caps[1], got.st)
    flushed.flush(big.data_ptr(), 2 * caps[1], got.st)                                    # at 1 frame like `a`, but flushed
    torch.cuda.synchronize()
    refused([a, other_streams], BAD_ARG)
    refused([a, other_m], BAD_ARG)
    refused([a, other_fs], BAD_ARG)
    third = torch.zeros((S, caps[0]), dtype=torch.uint8, device="cuda")
    refused([a, b, a], BAD_ARG, caps_=caps + [caps[0]], ptrs_=ptrs + [third.data_ptr()])
    refused([a, ahead], INVALID_STATE)
    refused([a, flushed], INVALID_STATE)
    refused([a, b], TOO_SMALL, caps_=[caps[0], fs * 2 - 16])
    for extra in (other_streams, other_m, other_fs, ahead, flushed):
        extra.close()
    torch.cuda.synchronize()
    assert all(bool((p == U.FILL).all()) for p in pcms)
    # nothing moved: the rest of the programme still equals the twins'
    assert got.fan(3) == (2, 1, 0)
    twin.single(3)
    got.flush()
    twin.flush()
    U.assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_at_the_size_that_is_timed():
    S, F, fs, base = 512, 8, 1024, 16
    specs = [U.A_S16, U.MONO_S16_M6]
    raw, L, row, x = U.reversed_rows(U.ints16(base, F, 16, fs), fs)
    assert_condition("toa", specs, x)
    raw = np.ascontiguousarray(np.tile(raw, (S // base, 1, 1)))            # 16 seeded streams, tiled over the batch
    mxs = [mats("toa", sp["layout"])[0] for sp in specs]
    got, twin = U.Drive(mxs, specs, raw, L, row, None, fs), U.Drive(mxs, specs, raw, L, row, None, fs)
    reset_tallies()
    assert got.fan(F) == (2, 1, 0)
    assert A.route_tally_ext() == {("FANOUT_LPCM", 0, 16, 0, 2): 1}
    twin.single(F)
    got.flush()
    twin.flush()
    assert got.emitted == twin.emitted
    for j in range(2):
        hg = hashlib.sha256(b"".join(got.bytes_of(j, s).tobytes() for s in range(S))).hexdigest()
        ht = hashlib.sha256(b"".join(twin.bytes_of(j, s).tobytes() for s in range(S))).hexdigest()
        assert hg == ht, "member %d" % j
    got.close()
    twin.close()
