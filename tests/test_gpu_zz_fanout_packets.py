"""iamf_hip_batch_render_fanout_packets: one element held as 24-bit or coupled LPCM packets rendered into several batches,
the packets read once (render_fanout_kernel<M, K, true, LPB, LPC>, iac_amd/csrc/render_fanout.hpp).

Expected bytes come from two independent sources and both are asserted: (a) TWIN batches of the same configuration driven by
K single iamf_hip_batch_render_packets calls on the same packets, in member order; (b) for s16 members the oracle
(oracle_lib.stream_run) on the decoded samples.  Equality is exact: PCM bytes, n_emitted, every member's flush tail and, where
stated, every member's exported stream state.  The report and every launch tally are asserted wherever a kernel is named, so
no test here passes by another route.

Inputs: S = 4, even streams loud, odd streams quiet (fanout_lpcm_util.ints16), packet rows with head 8 and pad 8; mono-coded
forms in reversed channel order, coupled forms with their sub-streams permuted (fanout_packets_util.coupled_order).  The
members' thresholds are chosen per element on the CPU and the condition — every loud stream exceeds every member's threshold
in every 1024-sample chunk, no quiet stream ever does — is asserted there before any GPU call (fanout_packets_util.case)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fanout_lpcm_util as U
import fanout_packets_util as PU
import iac_amd as A
import lpcm_util as LP

pytestmark = pytest.mark.gpu

BAD_ARG, TOO_SMALL, INVALID_STATE = -1, -2, -5
MEMBERS = U.MEMBERS
FAM = PU.FAM
INSTANCES = [(f, m, k) for f in ("s24", "s16c", "s24c") for m in PU.FORM_M[f] for k in PU.FAN_K]
# one element per form where a test takes one case per form
ONE_M = {"s24": 16, "s16c": 6, "s24c": 12}


def gen(m):
    return ("GENERIC", 0, m, 0, 0)


def close(*drives):
    for d in drives:
        d.close()


@pytest.mark.parametrize("form,m,K", INSTANCES, ids=["%s-%d-%d" % i for i in INSTANCES])
def test_every_instance_runs_once(form, m, K):
    """a lone chunk, prefetch across chunks and frames, state carried over; then the flush and the exported state"""
    S, fs, calls = 4, 1024, [1, 3, 2]
    got, twin, element, specs, x = PU.pair(form, m, MEMBERS[:K], S, sum(calls), fs)
    PU.reset_tallies()
    for nf in calls:
        assert got.fan(nf) == (K, 1, 0)
    blobs = got.export()
    got.flush()
    # the shared launches in the family's tally, the members' flushes in the base table, and nothing else anywhere
    assert PU.tallies() == {FAM: {PU.instance(form, m, K): len(calls)}, "base": {gen(m): K}}
    for nf in calls:
        twin.single(nf)
    twin_blobs = twin.export()
    twin.flush()
    single = PU.tallies()
    assert single.pop("base") == {gen(m): K} and list(single) == [PU.FORMS[form][3]], single
    assert sum(single[PU.FORMS[form][3]].values()) == K * len(calls)
    PU.U.assert_same(got, twin)
    for j in range(K):
        assert np.array_equal(blobs[j], twin_blobs[j]), "member %d: exported state differs from the twin's" % j
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


@pytest.mark.parametrize("form", ["s24", "s16c", "s24c"])
def test_frames_that_are_not_whole_chunks(form):
    """3072 samples: lanes divide by the frame size; 192: less than the 256 samples of saved state; 960: a short last chunk"""
    S, fs, K, calls, m = 4, 192, 3, [16, 1, 5, 2], ONE_M[form]
    got, twin, element, specs, x = PU.pair(form, m, MEMBERS[:K], S, sum(calls), fs)
    PU.reset_tallies()
    for nf in calls:
        assert got.fan(nf) == (K, 1, 0)
        twin.single(nf)
    assert A.route_family_tally(FAM) == {PU.instance(form, m, K): len(calls)}
    got.flush()
    twin.flush()
    U.assert_same(got, twin)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def test_one_state_format():
    """new entry -> single packet calls -> f32 fan-out on the same samples as f32 -> the old entry -> new entry -> flush, on
    the same batches: members in s16 / s24 / s32 / f32, 7.1.4 as coupled 24-bit packets"""
    S, fs, K, form, m = 4, 1024, 4, "s24c", 12
    base = [U.A_S16, U.A_GAINS_S24, U.MONO_S32_M9, U.member("A", fmt=A.FMT_F32, eg=1.2)]
    got, twin, element, specs, x = PU.pair(form, m, base, S, 7, fs)
    PU.reset_tallies()
    assert got.fan(2) == (K, 1, 0)
    got.single(1)
    assert got.fan_f32(1) == K
    assert got.fan_lpcm(1) == (K, 0, 1)
    assert got.fan(2) == (K, 1, 0)
    got.flush()
    t = PU.tallies()
    assert t.pop(FAM) == {PU.instance(form, m, K): 2}
    assert t.pop("base") == {("FANOUT", 0, m, 0, K): 2, gen(m): K}
    assert sum(t.pop("LPCM24_COUPLED").values()) == K and t == {}, t
    for nf in (2, 1, 1, 1, 2):
        twin.single(nf)
    twin.flush()
    U.assert_same(got, twin)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


@pytest.mark.parametrize("form", ["s24", "s16c", "s24c"])
def test_trim_and_position(form):
    """A trimmed first frame of 1000 samples is no whole number of 64-sample blocks: the old entry's report and tallies (a third
    drive on the old entry shows them).  The streams then stand at 1000 — neither a multiple of 16 nor below 240 — and whole
    frames are fused there; so is a trim of 896 samples from sample 60.  On 24-bit mono-coded packets a trim from sample 2
    leaves the dword grid (3 * 2 bytes): the old entry's route and report again."""
    S, fs, K, m = 4, 1024, 3, ONE_M[form]
    F = 5 if form == "s24" else 4
    element, specs, raw, L, row, x = PU.case(form, m, MEMBERS[:K], S, F, fs)
    mxs = [PU.mats(element, sp["layout"])[0] for sp in specs]
    got, twin, old = [PU.Drive(mxs, specs, raw, L, row, x, fs) for _ in range(3)]
    inst = PU.instance(form, m, K)

    def both(nf, **kw):
        """the call through the new entry and, on the third drive, through the old one: (report, tallies) of each"""
        PU.reset_tallies()
        r_new = got.fan(nf, **kw)
        t_new = PU.tallies()
        r_old = old.fan_lpcm(nf, **kw)
        return (r_new, t_new), (r_old, PU.tallies())

    new, was = both(1, first=24, n_samples=1000)
    assert new == was and FAM not in new[1]
    new, was = both(2)
    assert new == ((K, 1, 0), {FAM: {inst: 1}})
    new, was = both(1, first=60, n_samples=896)
    assert new == ((K, 1, 0), {FAM: {inst: 1}})
    twin.single(1, first=24, n_samples=1000)
    twin.single(2)
    twin.single(1, first=60, n_samples=896)
    kept = [x[:, :, 24:1024], x[:, :, 1024:3072], x[:, :, 3072 + 60:3072 + 60 + 896]]
    if form == "s24":
        new, was = both(1, first=2, n_samples=960)
        assert new == was and FAM not in new[1]
        twin.single(1, first=2, n_samples=960)
        kept.append(x[:, :, 4096 + 2:4096 + 2 + 960])
    for d in (got, twin, old):
        d.flush()
    U.assert_same(got, twin)
    U.assert_same(old, twin, "the old entry")
    PU.assert_oracle(got, element, specs, np.concatenate(kept, axis=2), fs)
    close(got, twin, old)


def totality_case(what):
    """-> (element, raw, L, row, x) of a call the new kernel does not read"""
    S, F, fs = 4, 3, 1024
    if what == "s16 mono-coded":
        return ("toa",) + U.reversed_rows(U.ints16(S, F, 16, fs), fs)
    if what == "big-endian 24 bit":
        return ("toa",) + U.reversed_rows(U.ints16(S, F, 16, fs, bps=3), fs, 3, False)
    if what == "32 bit":
        return ("toa",) + U.reversed_rows(U.ints16(S, F, 16, fs, bps=4), fs, 4, True)
    assert what == "5.1 as six mono sub-streams"
    ints = U.ints16(S, F, 6, fs)
    perm = [5, 4, 3, 2, 1, 0]
    raw, L, row = LP.rows(ints, 2, True, [1] * 6, perm, head=8, pad=8, frame_size=fs)
    return "L51", raw, L, row, U.decoded(ints, perm)


@pytest.mark.parametrize("what", ["s16 mono-coded", "big-endian 24 bit", "32 bit", "5.1 as six mono sub-streams"])
def test_totality(what):
    """calls whose packets the new kernel does not read: through the new entry and, on a twin, through the old one — reports,
    every tally and bytes identical"""
    fs, K, calls = 1024, 3, [2, 1]
    element, raw, L, row, x = totality_case(what)
    specs = PU.members_for(element, x, MEMBERS[:K])
    PU.assert_condition(element, specs, x)
    mxs = [PU.mats(element, sp["layout"])[0] for sp in specs]
    got, old = PU.Drive(mxs, specs, raw, L, row, x, fs), PU.Drive(mxs, specs, raw, L, row, x, fs)
    PU.reset_tallies()
    r_new = [got.fan(nf) for nf in calls]
    got.flush()
    t_new = PU.tallies()
    r_old = [old.fan_lpcm(nf) for nf in calls]
    old.flush()
    t_old = PU.tallies()
    assert r_new == r_old and t_new == t_old and FAM not in t_new
    if what == "s16 mono-coded":     # still the 16-bit packet-fed fan-out kernel
        assert r_new == [(K, 1, 0)] * len(calls) and t_new["ext"] == {("FANOUT_LPCM", 0, 16, 0, K): len(calls)}
    else:
        assert all(r[1] == 0 and r[2] == 1 for r in r_new)
    U.assert_same(got, old)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, old)


def test_mixed_wide_members_beside_the_shared_pair():
    """7.1.4 as coupled 24-bit packets into {A s16, MONO s16, B, J s24}: the pair shares the packets, the wide members run what
    their single calls run behind one unpack pass"""
    S, fs, calls, form, m = 4, 1024, [2, 1], "s24c", 12
    base = [U.A_S16, U.MONO_S16_M6, U.member("B"), U.member("J", fmt=A.FMT_S24)]
    got, twin, element, specs, x = PU.pair(form, m, base, S, sum(calls), fs)
    PU.reset_tallies()
    reports = [got.fan(nf) for nf in calls]
    got.flush()
    t = PU.tallies()
    for nf in calls:
        twin.single(nf)
    twin.flush()
    single = PU.tallies()
    assert reports == [(2, 1, 1)] * len(calls)
    assert t.pop(FAM) == {PU.instance(form, m, 2): len(calls)}
    assert sum(single.pop("LPCM24_COUPLED").values()) == 2 * len(calls)      # the pair's single calls, and only theirs
    assert t == single and "LPCM24_COUPLED" not in t                         # the wide members' rows and the four flushes
    U.assert_same(got, twin)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def test_a_limiter_off_member_beside_a_limiter_on_one():
    S, fs, calls, form, m = 4, 1024, [2, 1], "s24", 16
    base = [U.A_S16, U.member("A", limiter=False)]
    got, twin, element, specs, x = PU.pair(form, m, base, S, sum(calls), fs)
    PU.reset_tallies()
    reports = [got.fan(nf) for nf in calls]
    got.flush()
    t = PU.tallies()
    for nf in calls:
        twin.single(nf)
    twin.flush()
    single = PU.tallies()
    assert reports == [(0, 0, 1)] * len(calls)
    assert t == single and FAM not in t and t["LPCM24"] == {("LPCM24", 1, 16, 2, 0): len(calls)}
    U.assert_same(got, twin)
    assert got.emitted[0][0] == 2 * fs - 240 and got.emitted[1][0] == 2 * fs   # 240 withheld by the limiter's look-ahead
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def test_ranges():
    """sub-ranges (0, 2), (2, 3) and (5, 1) of six streams, out of step; rows outside a range keep their fill (Drive._take)"""
    S, fs, K, form, m = 6, 1024, 3, "s16c", 8
    got, twin, element, specs, x = PU.pair(form, m, MEMBERS[:K], S, 3, fs)
    inst = PU.instance(form, m, K)
    PU.reset_tallies()
    steps = [(2, 0, 2), (1, 2, 3), (1, 5, 1)]
    for nf, s0, cnt in steps:
        assert got.fan(nf, s0=s0, cnt=cnt) == (K, 1, 0)
    # a range spanning two positions: refused, nothing changes
    caps, pcms = got.bufs(fs)
    sentinel = A.FanoutReport(-7, -7, -7, -7)
    with pytest.raises(A.IamfHipError) as e:
        A.render_fanout_packets(got.batches, got.lpcm_input(0), 1, [p.data_ptr() for p in pcms], caps, got.st, stream0=0, n_streams=S,
                                report=sentinel)
    assert e.value.code == INVALID_STATE
    assert (sentinel.n_fused, sentinel.input_fused, sentinel.n_unpacks, sentinel.reserved) == (-7, -7, -7, -7)
    torch.cuda.synchronize()
    assert all(bool((p == U.FILL).all()) for p in pcms)
    rest = [(1, 5, 1), (2, 2, 3), (1, 0, 2), (1, 5, 1)]
    for nf, s0, cnt in rest:
        assert got.fan(nf, s0=s0, cnt=cnt) == (K, 1, 0)
    got.flush()
    assert PU.tallies() == {FAM: {inst: len(steps) + len(rest)}, "base": {gen(m): K}}
    for nf, s0, cnt in steps + rest:
        twin.single(nf, s0=s0, cnt=cnt)
    twin.flush()
    U.assert_same(got, twin)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def test_refusals_change_nothing():
    """the cases of test_gpu_fanout_lpcm.test_refusals_change_nothing on the new entry, 24-bit packets"""
    S, fs, form, m = 4, 1024, "s24", 16
    got, twin, element, specs, x = PU.pair(form, m, [U.A_S16, U.MONO_S16_M6], S, 4, fs)
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
        n = len(batches)
        hs = (A.hipabi.C.c_void_p * n)(*[b.h for b in batches])
        em = (A.hipabi.C.c_int32 * n)(*([-9] * n))
        call = A.PacketCall()
        call.in_ = inp or good
        call.args.n_frames, call.args.n_samples, call.args.stream = 1, n_samples, got.st
        r = A.lib().iamf_hip_batch_render_fanout_packets(hs, n, A.hipabi.C.byref(call), (A.hipabi.C.c_void_p * n)(*pp),
                                                         (A.hipabi.C.c_int64 * n)(*cc), 0, S, em, A.hipabi.C.byref(sentinel))
        assert r == code, (r, code)
        assert (sentinel.n_fused, sentinel.input_fused, sentinel.n_unpacks, sentinel.reserved) == (-7, -7, -7, -7)
        assert list(em) == [-9] * n

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
    mono = PU.mats("toa", "MONO")[0]
    other_streams = U.make_batch(mono, specs[1], S + 1, fs)
    other_m = U.make_batch(PU.mats("foa", "MONO")[0], specs[1], S, fs)
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
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def layouts():
    import gpu_util as G
    return [(G.PK_PAD16, "s24"), (G.PK_GRID, "s16c"), (G.PK_OFF_BASE, "s24c"), (G.PK_OFF_STRIDE, "s24"), (G.PK_BOUND, "s16c"),
            (G.PK_BEYOND, "s24c")]


@pytest.mark.parametrize("i", range(6), ids=["PAD16-s24", "GRID-s16c", "OFF_BASE-s24c", "OFF_STRIDE-s24", "BOUND-s16c", "BEYOND-s24c"])
def test_packet_layouts(i):
    """wherever a caller may put the packets (gpu_util.place_packets): the shared launch exactly where the member's single call
    reads the packets itself, else the twin's route; no byte outside the emitted runs is written (Drive._take)"""
    pk, form = layouts()[i]
    S, fs, K, calls, m = 4, 1024, 2, [3], ONE_M[form]
    got, twin, element, specs, x = PU.pair(form, m, [U.A_S16, U.MONO_S16_M6], S, sum(calls), fs, packets=pk)
    PU.reset_tallies()
    for nf in calls:
        twin.single(nf)
    twin.flush()
    single = PU.tallies()
    fused = PU.FORMS[form][3] in single         # what the member's single call decided
    reports = [got.fan(nf) for nf in calls]
    got.flush()
    t = PU.tallies()
    print("layout %s, %s: the single call %s the packets itself" % (pk.name, form, "reads" if fused else "does not read"), single)
    if fused:
        assert reports == [(K, 1, 0)] * len(calls)
        assert t == {FAM: {PU.instance(form, m, K): len(calls)}, "base": {gen(m): K}}
    else:       # the old entry's route and report, shown by a third drive on the old entry
        old = PU.Drive([PU.mats(element, sp["layout"])[0] for sp in specs], specs, got.raw, got.L, got.row, x, fs, packets=pk)
        r_old = [old.fan_lpcm(nf) for nf in calls]
        old.flush()
        assert reports == r_old and all(r[1] == 0 for r in reports) and FAM not in t and t == PU.tallies()
        U.assert_same(old, twin, "the old entry")
        old.close()
    U.assert_same(got, twin)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def test_on_a_stalled_non_blocking_stream():
    """the entry on a caller-owned stream proven hipStreamNonBlocking, with stream_util's 10 ms stall queued on that stream in
    front of the call: the call returns while the stall still runs, and renders the same"""
    import stream_util as SU
    S, fs, K, form, m = 4, 1024, 2, "s16c", 12
    with SU.side_stream() as side:
        h = side.cuda_stream
        got, twin, element, specs, x = PU.pair(form, m, [U.A_S16, U.MONO_S16_M6], S, 3, fs)
        assert got.st == h and twin.st == h

        def before_call(st):
            assert st == h
            SU.assert_non_blocking(st)
            ev = SU.stall(SU.torch_stream(st))
            assert not ev.query(), "the stall in front of the call had finished before the call was made"
            return lambda: not ev.query()

        PU.reset_tallies()
        assert got.fan(1) == (K, 1, 0)          # (the kernel is loaded)
        assert got.fan(2, before_call=before_call) == (K, 1, 0)
        assert got.notes == [True], "the call returned only after the stall in front of it"
        got.flush()
        assert A.route_family_tally(FAM) == {PU.instance(form, m, K): 2}
        twin.single(1)
        twin.single(2)
        twin.flush()
    U.assert_same(got, twin)
    PU.assert_oracle(got, element, specs, x, fs)
    close(got, twin)


def test_the_environment_switch_in_a_fresh_process():
    """IAMF_HIP_FANOUT_PACKETS_UNFUSED=1 in a child process: the family's tally stays empty, the old entry's report, equal bytes"""
    form = "s24c"
    got, twin, element, specs, x = PU.pair(form, PU.FORM_M[form][-1], [U.A_S16, U.MONO_S16_M6], 4, 2, 1024)
    PU.reset_tallies()
    assert got.fan(2) == (2, 1, 0)
    got.flush()
    assert A.route_family_tally(FAM) == {PU.instance(form, 12, 2): 1}
    sha = hashlib.sha256()
    for j in range(2):
        for s in range(4):
            sha.update(got.bytes_of(j, s).tobytes())
    close(got, twin)
    env = dict(os.environ)
    env["IAMF_HIP_FANOUT_PACKETS_UNFUSED"] = "1"
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(PU.__file__)), "fanout_packets_util.py"), "child", form],
                       capture_output=True, text=True, env=env, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["fam"] == {} and out["report"] == [2, 0, 1]
    assert out["sha"] == sha.hexdigest()
