"""-m gpu: the pipelined decoder group (iamf_hip_decoder_group_submit / _poll / _complete): two rounds in flight, the host
parsing round k + 1 while the device renders round k.  Every handle must still get exactly what the reference decoder
returned for its stream (the same goldens as tests/test_gpu_group.py), the buffers of an outstanding round belong to
the library, and the protocol errors change nothing."""
import ctypes as C
import time

import numpy as np
import pytest

import e2e_cases
import e2e_fuzz as F
from decoder_driver import last_metadata
from test_gpu_group import group_decode_all, lib, open_handle  # noqa: F401  (lib: the fixture that declares the entry points)

pytestmark = pytest.mark.gpu

ERR_INVALID_STATE = -5
SENTINEL = 0xA5


def _declare(L):
    L.iamf_hip_decoder_group_submit.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                                C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    L.iamf_hip_decoder_group_poll.argtypes = [C.c_void_p, C.c_uint64]
    L.iamf_hip_decoder_group_complete.argtypes = [C.c_void_p, C.c_uint64]
    L.iamf_hip_decoder_group_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    return L


class Pipe:
    """N handles of one group fed round by round; rounds go through _submit and are completed one round later (two in
    flight), or through _decode (sync=True).  The next round's data come from the rsizes _submit returned, before the
    previous round is complete.  Each round's data is a private copy that is overwritten with garbage once submitted; the
    pcm buffers (two sets, rotated) hold a sentinel until the round's _complete."""

    def __init__(self, L, case, streams, threads, starve, block=0):
        self.L, self.case, self.starve, self.block = _declare(L), case, starve, block
        self.n = n = len(streams)
        self.streams = streams
        self.bps = case.get("bit_depth", 16) // 8
        self.hs, self.used = [], []
        for i in range(n):
            d, self.ch, u = open_handle(L, case, streams[i])
            self.hs.append(d)
            self.used.append(u)
        self.win = [block + 97 * i for i in range(n)]
        harr = (C.c_void_p * n)(*self.hs)
        self.g = C.c_void_p()
        self.rc = L.iamf_hip_decoder_group_create(harr, n, threads, C.byref(self.g))
        self.cap = self.bps * 6144 * 6 * self.ch
        self.pcms = [[C.create_string_buffer(self.cap) for _ in range(n)] for _ in range(2)]
        self.parr = [(C.c_void_p * n)(*[C.addressof(p) for p in self.pcms[k]]) for k in range(2)]
        self.res = [(C.c_int32 * n)() for _ in range(2)]
        self.copies = [[None] * n for _ in range(2)]
        self.kinds = [None, None]
        self.tickets = [0, 0]
        self.chunks, self.rets, self.done = [[] for _ in range(n)], [[] for _ in range(n)], [False] * n
        self.rnd = 0
        self.outstanding = []   # set indices in submit order
        self.submits = 0
        self.violations = 0

    def _prepare(self, k):
        n = self.n
        data, sizes = (C.c_void_p * n)(), (C.c_int32 * n)()
        kind = []
        for i in range(n):
            st = self.streams[i]
            if self.done[i]:
                buf, kd = st[:1], "idle"
            elif self.used[i] >= len(st):
                buf, kd = None, "flush"
            elif self.starve(self.rnd, i):
                buf, kd = st[self.used[i]:self.used[i] + 1], "starved"
            else:
                w = len(st) - self.used[i]
                if self.block and w > self.win[i]:
                    w = self.win[i]
                buf, kd = st[self.used[i]:self.used[i] + w], "feed"
            kind.append(kd)
            if buf is None:
                self.copies[k][i] = None
                data[i], sizes[i] = None, 0
            else:
                self.copies[k][i] = C.create_string_buffer(bytes(buf), len(buf))
                data[i], sizes[i] = C.addressof(self.copies[k][i]), len(buf)
            C.memset(self.pcms[k][i], SENTINEL, self.cap)
        return data, sizes, kind

    def _advance(self, kind, rsz, res):
        for i in range(self.n):
            if kind[i] == "flush":
                self.done[i] = True
            elif kind[i] == "feed":
                assert res[i] >= 0, (i, res[i])
                if self.block and not rsz[i] and len(self.streams[i]) - self.used[i] > self.win[i]:
                    self.win[i] += self.block + 97 * i     # no complete OBU in the window: the player reads on
                    continue
                self.win[i] = self.block + 97 * i
                self.used[i] += rsz[i]
                if not rsz[i]:
                    self.used[i] = len(self.streams[i])
            else:
                assert res[i] == 0 and rsz[i] == 0, (i, kind[i], res[i], rsz[i])

    def _collect(self, k):
        kind, res = self.kinds[k], self.res[k]
        for i in range(self.n):
            r = res[i]
            if kind[i] in ("flush", "feed") and (r > 0 or kind[i] == "flush"):
                if r > 0:
                    self.chunks[i].append(self.pcms[k][i].raw[:r * self.ch * self.bps])
                self.rets[i].append(r)

    def submit(self):
        k = self.rnd & 1
        data, sizes, kind = self._prepare(k)
        rsz, t = (C.c_uint32 * self.n)(), C.c_uint64(0)
        assert self.L.iamf_hip_decoder_group_submit(self.g, data, sizes, rsz, self.parr[k], self.res[k], C.byref(t)) == 0
        for i in range(self.n):   # the caller's data buffers are the caller's again
            if self.copies[k][i] is not None:
                C.memset(self.copies[k][i], 0x5A ^ (self.rnd & 0xFF), sizes[i])
        self.kinds[k], self.tickets[k] = kind, t.value
        self._advance(kind, rsz, self.res[k])
        self.outstanding.append(k)
        self.submits += 1
        self.rnd += 1
        return t.value

    def complete_oldest(self):
        k = self.outstanding.pop(0)
        assert self.L.iamf_hip_decoder_group_complete(self.g, self.tickets[k]) == 0
        for o in self.outstanding:   # a round still out: nothing has touched its pcm buffers
            for i in range(self.n):
                if self.pcms[o][i].raw != bytes([SENTINEL]) * self.cap:
                    self.violations += 1
        self._collect(k)

    def decode(self):
        k = self.rnd & 1
        data, sizes, kind = self._prepare(k)
        rsz = (C.c_uint32 * self.n)()
        assert self.L.iamf_hip_decoder_group_decode(self.g, data, sizes, rsz, self.parr[k], self.res[k]) == 0
        self.kinds[k] = kind
        self._advance(kind, rsz, self.res[k])
        self._collect(k)
        self.submits += 1
        self.rnd += 1

    def run(self, sync_rounds=()):
        """until every handle has flushed; rounds whose index is in sync_rounds go through _decode (after draining)"""
        while not all(self.done):
            if self.rnd in sync_rounds:
                while self.outstanding:
                    self.complete_oldest()
                self.decode()
                continue
            self.submit()
            if len(self.outstanding) == 2:
                self.complete_oldest()
            assert self.rnd < 20000
        while self.outstanding:
            self.complete_oldest()
        assert self.violations == 0

    def times(self):
        sec, rounds = (C.c_double * 4)(), C.c_int64(0)
        assert self.L.iamf_hip_decoder_group_times(self.g, sec, C.byref(rounds)) == 0
        return list(sec), rounds.value

    def close(self):
        self.L.iamf_hip_decoder_group_destroy(self.g)
        for d in self.hs:
            assert self.L.IAMF_decoder_close(d) == 0

    def outputs(self):
        bits = self.bps * 8
        outs = []
        for i in range(self.n):
            raw = np.frombuffer(b"".join(self.chunks[i]), dtype=np.uint8)
            out = raw.view(np.int16).reshape(-1, self.ch) if bits == 16 else (
                raw.view(np.int32).reshape(-1, self.ch) if bits == 32 else raw.reshape(-1, self.ch, 3))
            outs.append((out.copy(), self.rets[i]))
        return outs


def pipe_decode_all(L, case, stream, n, threads, starve, block=0):
    streams = list(stream) if isinstance(stream, (list, tuple)) else [stream] * n
    p = Pipe(L, case, streams, threads, starve, block)
    if p.rc != 0:
        for d in p.hs:
            L.IAMF_decoder_close(d)
        return p.rc, None
    p.run()
    _, rounds = p.times()
    assert rounds == p.submits
    p.close()
    return 0, p.outputs()


def _out_of_step(r, i):
    return (r + 2 * i) % 5 == 0 and i % 2 == 1


@pytest.mark.parametrize("name", sorted(e2e_cases.CASES))
def test_pipelined_group_matches_reference_decoder(lib, golden, name):
    case = e2e_cases.CASES[name]
    stream, _ = e2e_cases.build(name)
    want, want_rets = golden.npz("e2e")[name], list(golden.npz("e2e")[name + "_rets"])
    if -5 in want_rets:
        pytest.skip("a stream that reconfigures mid-way is a single-handle protocol (the group refuses new sequences)")
    rc, outs = pipe_decode_all(lib, case, stream, 7, 3, _out_of_step)
    assert rc == 0, rc
    for i, (pcm, rets) in enumerate(outs):
        assert rets == want_rets, (name, i, rets, want_rets)
        assert pcm.shape == want.shape and np.array_equal(pcm, want), (name, i)


def _lfe_names():
    import lfe_cases as LC
    return sorted(LC.E2E)


@pytest.mark.parametrize("name", _lfe_names())
def test_pipelined_group_with_the_hoa_lfe_generator(lib, golden, name):
    import lfe_cases as LC
    c = LC.E2E[name]
    stream, _ = LC.build(name)
    case = dict(layout=("ss", LC.SS_ENUM[c["ss"]]), bit_depth=c["bit_depth"], lfe_hoa=True)
    want, want_rets = golden.npz("lfe")["e2e_" + name], list(golden.npz("lfe")["e2e_" + name + "_rets"])
    rc, outs = pipe_decode_all(lib, case, stream, 7, 3, lambda r, i: (r + i) % 4 == 0 and i % 3 != 0)
    assert rc == 0, rc
    for i, (pcm, rets) in enumerate(outs):
        assert rets == want_rets, (name, i, rets, want_rets)
        assert pcm.shape == want.shape and np.array_equal(pcm, want), (name, i)


@pytest.mark.parametrize("name", sorted(n for n, c in e2e_cases.CASES.items() if c.get("out_rate")))
def test_pipelined_group_of_resampling_handles(lib, golden, name):
    case = e2e_cases.CASES[name]
    stream, _ = e2e_cases.build(name)
    want, want_rets = golden.npz("e2e")[name], list(golden.npz("e2e")[name + "_rets"])
    rc, outs = pipe_decode_all(lib, case, stream, 9, 2, lambda r, i: (r * (i + 1)) % 3 == 1)
    assert rc == 0, rc
    for i, (pcm, rets) in enumerate(outs):
        assert rets == want_rets, (name, i, rets, want_rets)
        assert np.array_equal(pcm, want), (name, i)


GOLD_G = __import__("test_gpu_fuzz_facade")._gold("gmix")


@pytest.mark.parametrize("seed", range(F.N_GMIX))
def test_pipelined_group_whose_handles_decode_different_streams(lib, seed):
    want = GOLD_G[str(seed)]
    if "handles" not in want:
        pytest.skip("the reference dies on one of these streams")
    variant, cases, streams = F.gmix_build(seed)
    rc, outs = pipe_decode_all(lib, dict(cases[0]), streams, len(streams), 2, _out_of_step)
    if "toa_projection" in cases[0]["pair"]:   # every stream brings a de-mapping matrix of its own: not one topology
        assert rc == -1
        return
    assert rc == 0, (seed, rc)
    for i, (pcm, rets) in enumerate(outs):
        assert [int(r) for r in rets] == want["handles"][i]["rets"], (seed, variant, i)
        assert F.digest(pcm) == want["handles"][i]["sha256"], (seed, variant, i)


@pytest.mark.parametrize("name", ["toa_binaural_s16", "scalable_plus_scalable_J_ramps", "l714dmx_plus_l714dmx_C_trim",
                                  "stereo_441_to_48k", "stereo_plus_scalable_C_ramps"])
def test_pipelined_group_fed_in_blocks(lib, golden, name):
    """the player's block loop: handle i reads 777 + 97 i bytes at a time, so the sub-stream packets of a temporal unit
    arrive over several rounds — the earlier ones staged in the other slot's row: they must move along"""
    case = e2e_cases.CASES[name]
    stream, _ = e2e_cases.build(name)
    want = golden.npz("e2e")[name]
    rc, outs = pipe_decode_all(lib, case, stream, 6, 3, lambda r, i: (r + i) % 7 == 3, block=777)
    assert rc == 0, rc
    for i, (pcm, _) in enumerate(outs):
        assert pcm.shape == want.shape and np.array_equal(pcm, want), (name, i)


def _protocol_pipe(L, name="stereo_plus_scalable_C_ramps", n=5):
    case = e2e_cases.CASES[name]
    stream, _ = e2e_cases.build(name)
    return Pipe(L, case, [stream] * n, 2, _out_of_step), case, stream


def test_protocol_errors_change_nothing(lib, golden):
    name = "stereo_plus_scalable_C_ramps"
    want, want_rets = golden.npz("e2e")[name], list(golden.npz("e2e")[name + "_rets"])
    p, _, _ = _protocol_pipe(lib)
    assert p.rc == 0
    L, n = p.L, p.n
    dummy = (C.c_void_p * n)(*[C.addressof(x) for x in p.pcms[0]])
    data, sizes, rsz, res, t = (C.c_void_p * n)(), (C.c_int32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)(), C.c_uint64(0)
    for i in range(n):
        data[i], sizes[i] = None, 0   # would flush every handle if it were taken
    assert L.iamf_hip_decoder_group_complete(p.g, 1) == ERR_INVALID_STATE        # never issued
    assert L.iamf_hip_decoder_group_poll(p.g, 1) == ERR_INVALID_STATE
    checked = 0
    while not all(p.done):
        p.submit()
        if len(p.outstanding) == 2:
            older, newer = p.tickets[p.outstanding[0]], p.tickets[p.outstanding[1]]
            assert L.iamf_hip_decoder_group_submit(p.g, data, sizes, rsz, dummy, res, C.byref(t)) == ERR_INVALID_STATE
            assert L.iamf_hip_decoder_group_complete(p.g, newer) == ERR_INVALID_STATE    # out of order
            assert L.iamf_hip_decoder_group_complete(p.g, newer + 5) == ERR_INVALID_STATE  # unknown
            assert L.iamf_hip_decoder_group_decode(p.g, data, sizes, rsz, dummy, res) == ERR_INVALID_STATE
            t0 = time.monotonic()
            while True:   # bounded: the round's device work is a fraction of a millisecond
                r = L.iamf_hip_decoder_group_poll(p.g, older)
                assert r in (0, 1), r
                if r == 1 or time.monotonic() - t0 > 5.0:
                    break
            assert r == 1, "poll did not report the round ready within 5 s"
            checked += 1
            p.complete_oldest()
    while p.outstanding:
        p.complete_oldest()
    assert checked > 3
    assert L.iamf_hip_decoder_group_complete(p.g, p.tickets[0]) == ERR_INVALID_STATE   # already completed
    p.close()
    for i, (pcm, rets) in enumerate(p.outputs()):
        assert rets == want_rets, (i, rets, want_rets)
        assert np.array_equal(pcm, want), i


def test_destroy_with_two_rounds_outstanding(lib):
    p, _, _ = _protocol_pipe(lib)
    assert p.rc == 0
    for _ in range(4):
        p.submit()
        if len(p.outstanding) == 2:
            p.complete_oldest()
    p.submit()   # (4 handles of 5 are fed: a unit is in flight in both slots)
    assert len(p.outstanding) == 2
    p.L.iamf_hip_decoder_group_destroy(p.g)
    for k in range(2):
        for i in range(p.n):
            assert p.pcms[k][i].raw == bytes([SENTINEL]) * p.cap, (k, i)
    for d in p.hs:
        assert p.L.IAMF_decoder_close(d) == 0


def test_data_buffers_are_the_callers_once_submitted_and_blocks_carry_over(lib, golden):
    """every round's data is overwritten right after _submit (Pipe does it always); here also with units split over calls"""
    name = "toa_binaural_s16"
    case = e2e_cases.CASES[name]
    stream, _ = e2e_cases.build(name)
    want = golden.npz("e2e")[name]
    rc, outs = pipe_decode_all(lib, case, stream, 4, 2, lambda r, i: False, block=4096)
    assert rc == 0
    for i, (pcm, _) in enumerate(outs):
        assert np.array_equal(pcm, want), i


@pytest.mark.parametrize("name", ["l714_J_ramps", "stereo_loudness_info", "scalable_plus_scalable_J_ramps", "stereo_trim"])
def test_metadata_and_mixed_sync_rounds(lib, name):
    """the same rounds through _decode and through the pipeline (with synchronous rounds mixed in): identical PCM, return
    values and IAMF_decoder_get_last_metadata rows per handle once drained; _times counts every submit"""
    case = e2e_cases.CASES[name]
    stream, _ = e2e_cases.build(name)
    runs = []
    for mode in ("sync", "pipe", "mixed"):
        p = Pipe(lib, case, [stream] * 5, 2, _out_of_step)
        assert p.rc == 0
        if mode == "sync":
            p.run(sync_rounds=range(100000))
        elif mode == "pipe":
            p.run()
        else:
            p.run(sync_rounds=set(range(0, 3)) | set(range(9, 12)) | set(range(20, 100000)))
        _, rounds = p.times()
        assert rounds == p.submits, (mode, rounds, p.submits)
        meta = [last_metadata(lib, d, True) for d in p.hs]
        p.close()
        runs.append((p.outputs(), meta))
    (o0, m0) = runs[0]
    for outs, meta in runs[1:]:
        for i in range(5):
            assert outs[i][1] == o0[i][1], i
            assert np.array_equal(outs[i][0], o0[i][0]), i
            assert meta[i] == m0[i], (i, meta[i], m0[i])
