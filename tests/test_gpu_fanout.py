"""iamf_hip_batch_render_fanout: one element rendered into several batches, the input read once.

Expected bytes come from two independent sources and both are asserted: (a) TWIN batches of the same configuration driven
by iamf_hip_batch_render alone on the same device input; (b) for s16 members the oracle (oracle_lib.stream_run).  Equality
is exact: PCM bytes, n_emitted, every member's flush tail.  n_fused is asserted wherever the shared-input kernel
(render_fanout_kernel, iac_amd/csrc/render_fanout.hpp) must run, so no test here passes by the plain route alone."""
import hashlib

import numpy as np
import pytest
import torch

import gpu_util as G
import iac_amd as A
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

BAD_ARG, TOO_SMALL, INVALID_STATE = -1, -2, -5
BPS = {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4, A.FMT_F32: 4}

# element -> (channels, product matrix for a layout, oracle matrix for a layout)
ELEMENTS = {
    "foa": (4, lambda o: A.get_h2m_matrix(1, A.SS[o]), lambda o: O.get_h2m(1, O.SS[o])),
    "soa": (9, lambda o: A.get_h2m_matrix(2, A.SS[o]), lambda o: O.get_h2m(2, O.SS[o])),
    "toa": (16, lambda o: A.get_h2m_matrix(3, A.SS[o]), lambda o: O.get_h2m(3, O.SS[o])),
    "L51": (6, lambda o: A.get_m2m_matrix(A.SS["L51"], A.SS[o]), lambda o: O.get_m2m(O.SS["L51"], O.SS[o])),
    "L71": (8, lambda o: A.get_m2m_matrix(A.SS["L71"], A.SS[o]), lambda o: O.get_m2m(O.SS["L71"], O.SS[o])),
    "L714": (12, lambda o: A.get_m2m_matrix(A.SS["L714"], A.SS[o]), lambda o: O.get_m2m(O.SS["L714"], O.SS[o])),
}


def member(layout, fmt=A.FMT_S16, eg=1.0, og=1.0, lg=None, thr_db=-1.0, limiter=True):
    return dict(layout=layout, fmt=fmt, eg=eg, og=og, lg=lg, thr_db=thr_db, limiter=limiter)


# the four renditions the parity test draws from: they differ in matrix, gains, threshold or format
A_S16 = member("A")
MONO_S16 = member("MONO")
A_GAINS_S24 = member("A", fmt=A.FMT_S24, eg=0.9, og=1.1, lg=0.95)     # gain product 0.9405
MONO_S32_M3 = member("MONO", fmt=A.FMT_S32, thr_db=-3.0)
MEMBERS = [A_S16, MONO_S16, A_GAINS_S24, MONO_S32_M3]


def gain_product(sp):
    g = 1.0
    for v in (sp["eg"], sp["og"], sp["lg"]):
        if v is not None:
            g *= v
    return g


def make_batch(element, sp, S, fs):
    oc = A.layout_channels(A.SS[sp["layout"]])
    b = A.Batch(S, ELEMENTS[element][1](sp["layout"]), oc, frame_size=fs, out_format=sp["fmt"], limiter=sp["limiter"],
                threshold_db=sp["thr_db"], loudness=sp["lg"] is not None,
                # wide layouts of an ambisonics element default to the MFMA projection, which is within a tolerance of the
                # reference, not equal to it: the oracle comparison here wants the exact one
                projection=A.PROJ_EXACT if oc > 2 else A.PROJ_AUTO)
    b.set_gains(element=[sp["eg"]] * S, output=[sp["og"]] * S, loudness=None if sp["lg"] is None else [sp["lg"]] * S)
    b.oc, b.bps = oc, BPS[sp["fmt"]]
    return b


def programme(m, S, n, seed0=100):
    """even streams hot, odd streams quiet"""
    return np.stack([synth.hot(seed0 + s, m, n) if s % 2 == 0 else synth.quiet(seed0 + s, m, n) for s in range(S)])


class Drive:
    """K batches on one device input; every step appends each member's emitted bytes per stream"""

    def __init__(self, element, specs, x, fs):
        self.S, self.m, total = x.shape
        self.fs, self.F = fs, total // fs
        self.xin = torch.from_numpy(G.to_frames(x, fs)).cuda()
        self.batches = [make_batch(element, sp, self.S, fs) for sp in specs]
        self.out = [[[] for _ in range(self.S)] for _ in specs]
        self.emitted = [[] for _ in specs]
        self.fused = []
        self.f0 = 0
        self.st = torch.cuda.current_stream().cuda_stream

    def _bufs(self, n_samples):
        caps = [(max(n_samples, 240) * b.oc * b.bps + 15) & ~15 for b in self.batches]
        return caps, [torch.zeros((self.S, c), dtype=torch.uint8, device="cuda") for c in caps]

    def _take(self, j, pcm, n):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        b = self.batches[j]
        for s in range(self.S):
            self.out[j][s].append(h[s][:n * b.oc * b.bps].copy())
        self.emitted[j].append(n)

    def _in(self):
        return self.xin.data_ptr() + 4 * self.f0 * self.m * self.fs, self.F * self.m * self.fs, self.m * self.fs

    def fan(self, nf):
        caps, pcms = self._bufs(nf * self.fs)
        d_in, ss, fstr = self._in()
        ns, fused = A.render_fanout(self.batches, d_in, ss, fstr, nf, [p.data_ptr() for p in pcms], caps, self.st)
        for j, n in enumerate(ns):
            self._take(j, pcms[j], n)
        self.fused.append(fused)
        self.f0 += nf
        return fused

    def single(self, nf):
        caps, pcms = self._bufs(nf * self.fs)
        d_in, ss, fstr = self._in()
        for j, b in enumerate(self.batches):
            self._take(j, pcms[j], b.render(d_in, ss, fstr, nf, pcms[j].data_ptr(), caps[j], self.st))
        self.f0 += nf

    def flush(self):
        caps, pcms = self._bufs(240)
        for j, b in enumerate(self.batches):
            self._take(j, pcms[j], b.flush(pcms[j].data_ptr(), caps[j], self.st))

    def close(self):
        for b in self.batches:
            b.close()

    def bytes_of(self, j, s):
        return np.concatenate(self.out[j][s])


def assert_same(got, want, what=""):
    assert got.emitted == want.emitted, what
    for j in range(len(got.batches)):
        for s in range(got.S):
            for i, (a, b) in enumerate(zip(got.out[j][s], want.out[j][s])):
                assert np.array_equal(a, b), "%s member %d stream %d step %d differs from the twin" % (what, j, s, i)


def assert_oracle(d, element, specs, x, fs):
    """s16 members against the oracle, stream by stream"""
    for j, sp in enumerate(specs):
        if sp["fmt"] != A.FMT_S16:
            continue
        oc = d.batches[j].oc
        omx = ELEMENTS[element][2](sp["layout"])
        for s in range(d.S):
            want = O.stream_run(omx, oc, x[s], fs, element_gain=sp["eg"], output_gain=sp["og"], loudness_on=int(sp["lg"] is not None),
                                loudness_gain=sp["lg"] if sp["lg"] is not None else 1.0, limiter_on=int(sp["limiter"]), thr_db=sp["thr_db"])
            assert np.array_equal(d.bytes_of(j, s).view(np.int16).reshape(-1, oc), want), "member %d stream %d differs from the oracle" % (j, s)


def assert_condition(element, specs, x):
    """every hot stream exceeds every member's threshold and no quiet stream does: the hypothesis path and the recurrence
    both run in every member, and a limiter state that leaked from one member into another would show"""
    for sp in specs:
        oc = A.layout_channels(A.SS[sp["layout"]])
        omx = ELEMENTS[element][2](sp["layout"])
        thr = 10.0 ** (sp["thr_db"] / 20.0)
        g = gain_product(sp)
        assert 0.7 <= g <= 1.25
        for s in range(x.shape[0]):
            peak = float(np.abs(O.render(omx, x[s], oc)).max()) * g
            print("condition %s -> %s stream %d (%s): peak %.3f against %.3f" % (element, sp["layout"], s, "hot" if s % 2 == 0 else "quiet", peak, thr))
            if s % 2 == 0:
                assert peak > thr, (element, sp["layout"], s, peak, thr)
            else:
                assert peak < thr, (element, sp["layout"], s, peak, thr)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("element", ["foa", "soa", "toa", "L51", "L71", "L714"])
def test_shared_kernel_parity(element, K):
    S, fs, calls = 8, 1024, [1, 3, 2, 5]
    specs = MEMBERS[:K]
    x = programme(ELEMENTS[element][0], S, sum(calls) * fs)
    assert_condition(element, specs, x)
    got, twin = Drive(element, specs, x, fs), Drive(element, specs, x, fs)
    m = ELEMENTS[element][0]
    A.route_reset()
    for nf in calls:
        assert got.fan(nf) == K
    got.flush()
    # one launch of render_fanout_kernel<m, K> per call and nothing beside it; each member's flush on the generic kernel
    assert A.route_tally() == {("FANOUT", 0, m, 0, K): len(calls), ("GENERIC", 0, m, 0, 0): K}
    for nf in calls:
        twin.single(nf)
    twin.flush()
    single = A.route_tally()
    assert single.pop(("GENERIC", 0, m, 0, 0)) == K and sum(single.values()) == K * len(calls)
    assert all(k[0] == "FAST" and k[1] == 0 and k[2] == m for k in single), single   # the twin: render_fast_kernel<m, OC> per member
    assert_same(got, twin)
    assert_oracle(got, element, specs, x, fs)
    got.close()
    twin.close()


def test_state_is_the_batches_own():
    """fan-out call -> single calls on each member -> fan-out call -> flush: the persisted state has one format"""
    S, fs = 8, 1024
    specs = [A_S16, A_GAINS_S24, MONO_S32_M3, member("A", fmt=A.FMT_F32, eg=1.2)]   # (f32: the fourth store format)
    x = programme(16, S, 7 * fs)
    got, twin = Drive("toa", specs, x, fs), Drive("toa", specs, x, fs)
    assert got.fan(2) == 4
    got.single(1)
    got.single(1)
    assert got.fan(3) == 4
    for nf in (2, 1, 1, 3):
        twin.single(nf)
    got.flush()
    twin.flush()
    assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_mixed_families():
    S, fs, calls = 8, 1024, [2, 1, 3]
    specs = [A_S16, MONO_S16, member("B"), member("J", fmt=A.FMT_S24)]
    x = programme(16, S, sum(calls) * fs)
    got, twin = Drive("toa", specs, x, fs), Drive("toa", specs, x, fs)
    for nf in calls:
        assert got.fan(nf) == 2
        twin.single(nf)
    got.flush()
    twin.flush()
    assert_same(got, twin, "wide members beside the shared pair:")
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()

    specs = [A_S16, member("A", limiter=False)]
    got, twin = Drive("toa", specs, x, fs), Drive("toa", specs, x, fs)
    for nf in calls:
        assert got.fan(nf) == 0
        twin.single(nf)
    got.flush()
    twin.flush()
    assert_same(got, twin, "limiter on / off:")
    assert got.emitted[0][0] == 2 * fs - 240 and got.emitted[1][0] == 2 * fs   # 240 withheld by the limiter's look-ahead
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()


def test_off_the_fast_path():
    S, K = 8, 3
    specs = MEMBERS[:K]
    fs = 1000   # call totals that are no multiple of 64: the general kernel, member by member
    x = programme(16, S, 4 * fs)
    got, twin = Drive("toa", specs, x, fs), Drive("toa", specs, x, fs)
    for nf in (1, 3):
        assert got.fan(nf) == 0
        twin.single(nf)
    got.flush()
    twin.flush()
    assert_same(got, twin)
    assert_oracle(got, "toa", specs, x, fs)
    got.close()
    twin.close()
    fs = 1024   # ... and the same members at 1024 on fresh batches share the input
    x = programme(16, S, 2 * fs)
    got = Drive("toa", specs, x, fs)
    assert got.fan(2) == K
    got.close()


def test_refusals_change_nothing():
    S, fs = 8, 1024
    specs = [member("A"), member("MONO")]
    x = programme(8, S, 4 * fs)
    got, twin = Drive("L71", specs, x, fs), Drive("L71", specs, x, fs)
    got.fan(1)
    twin.single(1)
    caps, pcms = got._bufs(fs)
    d_in, ss, fstr = got._in()
    ptrs = [p.data_ptr() for p in pcms]

    def refused(batches, code, caps_=None, ptrs_=None):
        """every buffer and stride of the call is valid for its member unless the case says otherwise: the one thing wrong
        with the call is what the case names"""
        pp, cc = ptrs_ or ptrs, caps_ or caps
        assert len(pp) == len(cc) == len(batches) and all(pp)
        with pytest.raises(A.IamfHipError) as e:
            A.render_fanout(batches, d_in, ss, fstr, 1, pp, cc, got.st)
        assert e.value.code == code, (e.value.code, code)

    a, b = got.batches
    other_streams = make_batch("L71", specs[1], S + 1, fs)
    other_m = make_batch("L51", specs[1], S, fs)
    other_fs = make_batch("L71", specs[1], S, 960)
    ahead = make_batch("L71", specs[1], S, fs)
    big = torch.zeros((S, 2 * caps[1]), dtype=torch.uint8, device="cuda")
    ahead.render(got.xin.data_ptr(), ss, fstr, 2, big.data_ptr(), 2 * caps[1], got.st)    # stands at 2 frames, `a` at 1
    flushed = make_batch("L71", specs[1], S, fs)
    flushed.render(got.xin.data_ptr(), ss, fstr, 1, big.data_ptr(), 2 * caps[1], got.st)
    flushed.flush(big.data_ptr(), 2 * caps[1], got.st)                                    # at 1 frame like `a`, but flushed
    dmx = A.Batch(S, A.dmx_matrix(5, 1), 2, frame_size=fs, out_format=A.FMT_S16, limiter=True)   # 7.1 -> stereo down-mixer
    torch.cuda.synchronize()
    refused([a, other_streams], BAD_ARG)
    refused([a, other_m], BAD_ARG)
    refused([a, other_fs], BAD_ARG)
    refused([a, ahead], INVALID_STATE)
    refused([a, flushed], INVALID_STATE)
    third = torch.zeros((S, caps[0]), dtype=torch.uint8, device="cuda")   # a buffer of its own for the repeated member
    refused([a, b, a], BAD_ARG, caps + [caps[0]], ptrs + [third.data_ptr()])
    refused([a, a], BAD_ARG, [caps[0], caps[0]], [ptrs[0], third.data_ptr()])
    refused([b, a, b], BAD_ARG, [caps[1], caps[0], caps[0]], [ptrs[1], ptrs[0], third.data_ptr()])
    refused([a, dmx], BAD_ARG)
    refused([a, b], TOO_SMALL, [caps[0], fs * 2 - 16])
    refused([a, b], TOO_SMALL, [fs * 4 - 16, caps[1]])
    for extra in (other_streams, other_m, other_fs, ahead, flushed, dmx):
        extra.close()
    # nothing moved: the rest of the programme still equals the twins'
    assert got.fan(3) == 2
    twin.single(3)
    got.flush()
    twin.flush()
    assert_same(got, twin)
    assert_oracle(got, "L71", specs, x, fs)
    got.close()
    twin.close()


def test_at_the_size_that_is_timed():
    S, F, fs = 512, 8, 1024
    specs = [A_S16, MONO_S16]
    x = np.stack([synth.hot(1000 + s, 16, F * fs) for s in range(S)])   # the hot programme on every stream
    got, twin = Drive("toa", specs, x, fs), Drive("toa", specs, x, fs)
    assert got.fan(F) == 2
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
