"""-m gpu: per-stream lifecycle of the resampler — iamf_hip_resampler_restart_range, _export_range, _import_range.

Stereo, 4 streams, an interpolated rate pair (44.1 -> 48 kHz, resample_block_kernel) and a direct one (96 -> 48 kHz).  A
stream restarted next to running neighbours, and a stream moved to a second resampler in the middle of its life, must
give, bit for bit, what oracle_lib.resample_run gives for that programme alone — the flush tail included."""
import numpy as np
import pytest

import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

S, CH, NS = 4, 2, 1024
RATES = [(44100, 48000), (96000, 48000)]


class Rig:
    def __init__(self, rates):
        import torch
        import iac_amd as A
        self.torch = torch
        self.r = A.Resampler(S, CH, rates[0], rates[1])
        self.st = torch.cuda.current_stream().cuda_stream
        self.cap = self.r.out_capacity(NS)
        self.out = [[] for _ in range(S)]

    def upload(self, rows):
        """rows: {stream: x [ch][ns]} -> the interleaved input tensor [S][NS][ch] of one call"""
        t = self.torch.zeros((S, NS, CH), dtype=self.torch.float32, device="cuda")
        for s, x in rows.items():
            t[s, :x.shape[1]] = self.torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
        return t

    def process(self, inter, ns, ranges):
        o = self.torch.zeros((S, self.cap, CH), dtype=self.torch.float32, device="cuda")
        n = {}
        for s0, cnt in ranges:
            n[s0] = self.r.process_range(inter.data_ptr(), NS * CH, ns, o.data_ptr(), self.cap * CH, s0, cnt, self.st)
            assert n[s0] >= 0, (s0, cnt, n[s0])
        self._collect(o, n, ranges)

    def flush(self, ranges):
        cap = max(self.r.flush_capacity(), 1)
        o = self.torch.zeros((S, cap, CH), dtype=self.torch.float32, device="cuda")
        n = {}
        for s0, cnt in ranges:
            n[s0] = self.r.flush_range(o.data_ptr(), cap * CH, s0, cnt, self.st)
            assert n[s0] >= 0, (s0, cnt, n[s0])
        self._collect(o, n, ranges)

    def _collect(self, o, n, ranges):
        self.torch.cuda.synchronize()
        h = o.cpu().numpy()
        served = set()
        for s0, cnt in ranges:
            for s in range(s0, s0 + cnt):
                self.out[s].append(h[s, :n[s0]].T.copy())
                served.add(s)
        for s in range(S):
            assert s in served or not h[s].any(), "a stream outside the ranges was written"

    def take(self, s):
        got, self.out[s] = np.concatenate(self.out[s], axis=1), []
        return got


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


@pytest.mark.parametrize("rates", RATES)
def test_restart_of_one_stream_after_two_calls(rates):
    sizes = [1024, 700, 1024, 700]
    x = [synth.uniform(2100 + s, CH, sum(sizes), amp=0.9) for s in range(S)]
    y = synth.uniform(2150, CH, sizes[2] + sizes[3], amp=0.9)      # stream 1's second programme
    rig = Rig(rates)
    ins = [rig.upload({s: x[s][:, 0:1024] for s in range(S)}), rig.upload({s: x[s][:, 1024:1724] for s in range(S)})]
    rows = {s: x[s][:, 1724:2748] for s in range(S)}
    rows[1] = y[:, :1024]
    ins.append(rig.upload(rows))
    rows = {s: x[s][:, 2748:] for s in range(S)}
    rows[1] = y[:, 1024:]
    ins.append(rig.upload(rows))
    rig.torch.cuda.synchronize()

    rig.process(ins[0], sizes[0], [(0, S)])
    rig.process(ins[1], sizes[1], [(0, S)])
    first = rig.take(1)
    rig.r.restart_range(1, 1, rig.st)
    assert rig.r.same_state(0, 2) and rig.r.same_state(2, 3) and not rig.r.same_state(0, 1)
    groups = [(1, 1), (0, 1), (2, 2)]
    rig.process(ins[2], sizes[2], groups)
    rig.process(ins[3], sizes[3], groups)
    rig.flush(groups)

    same(first, O.resample_run(x[1][:, :1724], rates[0], rates[1], sizes[:2], flush=False)[0], "first life")
    same(rig.take(1), O.resample_run(y, rates[0], rates[1], sizes[2:])[0], "second life")
    for s in (0, 2, 3):
        same(rig.take(s), O.resample_run(x[s], rates[0], rates[1], sizes)[0], ("neighbour", s))
    rig.r.close()


@pytest.mark.parametrize("rates", RATES)
def test_export_to_a_second_resampler_mid_stream(rates):
    import iac_amd as A
    before, after = [1024, 700, 333], [1024, 512]      # three calls: the streams' past then lies in the second buffer
    sizes = before + after
    x = [synth.uniform(2200 + s, CH, sum(sizes), amp=0.9) for s in range(S)]
    a, b = Rig(rates), Rig(rates)
    ins, pos = [], 0
    for i, ns in enumerate(sizes):
        rig = a if i < len(before) else b
        ins.append(rig.upload({(s if rig is a else s - 1): x[s][:, pos:pos + ns] for s in (range(S) if rig is a else (1, 2))}))
        pos += ns
    a.torch.cuda.synchronize()

    for i, ns in enumerate(before):
        a.process(ins[i], ns, [(0, S)])
    nbytes = a.r.stream_state_bytes()
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes == b.r.stream_state_bytes()
    stride = nbytes + 16
    blob = a.torch.zeros((2, stride), dtype=a.torch.uint8, device="cuda")
    tickets = a.r.export_range(1, 2, blob.data_ptr(), stride, a.st)
    assert [t.kind for t in tickets] == [2, 2] and all(t.bytes == nbytes for t in tickets)
    b.r.import_range(0, 2, blob.data_ptr(), stride, tickets, b.st)
    assert b.r.same_state(0, 1) and not b.r.same_state(1, 2)
    for i, ns in enumerate(after):
        b.process(ins[len(before) + i], ns, [(0, 2)])
    b.flush([(0, 2)])
    for s in (1, 2):
        want = O.resample_run(x[s], rates[0], rates[1], sizes)[0]
        same(np.concatenate([a.take(s), b.take(s - 1)], axis=1), want, ("migrated", s))
    # refusals write nothing and change nothing: a ticket of another rate pair, a stride below the blob, a range past the end
    other = A.Resampler(1, CH, 48000, 44100)
    big = max(other.stream_state_bytes(), nbytes)
    blob2 = a.torch.zeros(big, dtype=a.torch.uint8, device="cuda")
    foreign = other.export_range(0, 1, blob2.data_ptr(), big, a.st)
    assert foreign[0].signature != tickets[0].signature
    for call in (lambda: b.r.import_range(0, 1, blob2.data_ptr(), big, foreign, b.st),
                 lambda: b.r.import_range(0, 2, blob.data_ptr(), nbytes - 16, tickets, b.st),
                 lambda: b.r.import_range(3, 2, blob.data_ptr(), stride, tickets, b.st)):
        with pytest.raises(A.IamfHipError) as e:
            call()
        assert e.value.code == -1
    other.close()
    a.r.close()
    b.r.close()
