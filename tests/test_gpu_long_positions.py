"""-m gpu: streams that have been running for a long time — positions across 2^31 and 2^32 samples and at 2^40.

A 48 kHz stream passes 2^31 samples after 12.4 hours and 2^32 after 24.9.  Every kernel family derives ring places, emit
decisions and output offsets from RenderParams::pos0 (int64) next to 32-bit quantities, and the host routes on pos0 & 15
and pos0 < kDelay.  Nobody renders twelve hours here: iamf_hip_batch_import_range takes the stream's position from the
ticket (iamf_hip_stream_state::cursor[0]), so a stream exported at P and imported with cursor[0] = P + D stands at P + D.
The edited ticket is a test device, no promise of the ABI.

Per family (tests/long_positions.py holds the table, the shifts and the programmes): two frames on a source batch, export
of the whole batch, import into a fresh batch of the same configuration with D added to every ticket, calls of one, two
and one frames, the flush.  Asserted for D = 0 (the control) and for every shift: the source's PCM followed by the
target's equals the oracle's output for the whole programme bit for bit (the MFMA projections within 1 LSB); every
shifted run equals the control bit for bit, the MFMA ones included; the launch tallies of all three tables equal the
control's and name the family's instance for every whole-frame call — a launch that falls back to the generic kernel at a
large position fails; the ticket exported behind the last render stands at Q + 4096 and, behind the flush, is flushed.
0xA5 canaries behind every emitted run must survive.

Out of scope: FIR batches (their export is UNIMPLEMENTED), the resampler (its cursor is a phase, not a running position)
and the positions the decoder façade and the groups keep internally, which cannot be set from outside."""
import numpy as np
import pytest

import long_positions as LPOS
import route_cases as R
from lifecycle_util import Rig, same

pytestmark = pytest.mark.gpu

S = LPOS.S
FILL = 0xA5
INVALID_STATE = -5
SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_PROJECTION", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY",
            "IAMF_HIP_LPCM_UNFUSED")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _mods():
    import torch
    import gpu_util as G
    import iac_amd as A
    return A, G, torch


class Device:
    """a family's inputs in device memory, uploaded once for the control and every shift"""

    def __init__(self, fam):
        A, G, torch = _mods()
        import lpcm_util as LP
        self.fam = fam
        self.st = torch.cuda.current_stream().cuda_stream
        self.fmt = {16: A.FMT_S16, 24: A.FMT_S24, -32: A.FMT_F32}[fam.bd]
        self.bps = {16: 2, 24: 3, -32: 4}[fam.bd]
        self.xin = self.xin2 = self.ramp = self.raw = self.records = None
        if fam.bytes:
            ints = fam.frames_of(fam.ints, np.zeros((fam.m, 0), dtype=np.int64))      # [S][F][m][fs], in decoded order
            coded = np.empty_like(ints)
            coded[:, :, fam.perm, :] = ints          # output channel c takes the decoded channel perm[c]
            raw, self.L, self.row = LP.rows(coded, fam.bytes, True, [1] * fam.m, fam.perm, head=16, pad=0, frame_size=fam.fs)
            self.raw = torch.from_numpy(raw).cuda()
        else:
            self.xin = torch.from_numpy(fam.frames_of(fam.x)).cuda()
        if fam.kind == "mix":
            self.xin2 = torch.from_numpy(fam.frames_of(fam.x2, np.zeros((1, 0), dtype=np.float32))).cuda()
            if fam.out_ramp is not None:
                self.ramp = torch.from_numpy(fam.out_ramp).cuda()
        if fam.kind in ("down", "demix"):
            self.records = fam.records

    def open(self):
        """fresh batches of the family's configuration, one per member"""
        A, G, torch = _mods()
        fam, out = self.fam, []
        for (mx, _), oc in zip(fam.mxs, fam.ocs):
            if fam.kind == "down":
                b = A.Batch(S, A.dmx_matrix(fam.il, fam.ol), oc, frame_size=fam.fs, out_format=self.fmt, limiter=True)
            else:
                b = A.Batch(S, mx, oc, frame_size=fam.fs, out_format=self.fmt, limiter=fam.limiter,
                            projection=A.PROJ_MFMA if fam.mfma else A.PROJ_EXACT, lfe_hoa=fam.lfe)
            if fam.kind == "mix":
                b.set_second_element(fam.mx2[0], [1.0] * S)
            if fam.kind == "demix":
                b.set_demixer(fam.dc["layout"], fam.dc["order"], fam.dc["gains"], fam.dc["offset"])
            out.append(b)
        return out

    def _pcms(self, n_samples):
        A, G, torch = _mods()
        caps = [G.r16(max(n_samples, 240) * oc * self.bps) + 16 for oc in self.fam.ocs]
        return caps, [torch.full((S, cap), FILL, dtype=torch.uint8, device="cuda") for cap in caps]

    def _take(self, out, pcms, ns):
        """the emitted runs, member by member and stream by stream; every byte behind them must still be the canary"""
        A, G, torch = _mods()
        torch.cuda.synchronize()
        for j, (pcm, n) in enumerate(zip(pcms, ns)):
            h = pcm.cpu().numpy()
            nb = n * self.fam.ocs[j] * self.bps
            assert (h[:, nb:] == FILL).all(), "bytes behind the emitted run were written"
            for s in range(S):
                out[j][s].append(h[s, :nb].copy())

    def _lpcm_input(self, f0):
        A, G, torch = _mods()
        inp = A.LpcmInput()
        inp.d_raw = self.raw.data_ptr() + f0 * self.row
        inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = self.fam.frames * self.row, self.row, self.L
        return inp

    def render(self, batches, out, f0, nf, trim=0):
        """frames [f0, f0 + nf) of every stream (trim: less that many samples at the start of the first one)"""
        A, G, torch = _mods()
        fam = self.fam
        m, fs, F = fam.m, fam.fs, fam.frames
        caps, pcms = self._pcms(nf * fs)
        keep = None
        if fam.kind == "fan":
            ns, fused = A.render_fanout(batches, self.xin.data_ptr() + 4 * f0 * m * fs, F * m * fs, m * fs, nf,
                                        [p.data_ptr() for p in pcms], caps, self.st)
            assert fused == 2, fused
        elif fam.kind == "fan_lpcm":
            ns, report = A.render_fanout_lpcm(batches, self._lpcm_input(f0), nf, [p.data_ptr() for p in pcms], caps, self.st)
            assert report == (2, 1, 0), report
        else:
            a = A.RenderArgs()
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcms[0].data_ptr(), caps[0], self.st
            if fam.kind == "lpcm":
                ns = [batches[0].render_lpcm(self._lpcm_input(f0), a)]
            else:
                a.d_in = self.xin.data_ptr() + 4 * (f0 * m * fs + trim)
                a.in_stream_stride, a.in_frame_stride = F * m * fs, m * fs
                a.n_samples = nf * fs - trim if trim else 0
                if self.xin2 is not None:
                    a.d_in2, a.in2_stream_stride, a.in2_frame_stride = self.xin2.data_ptr() + 4 * f0 * fs, F * fs, fs
                if self.ramp is not None:
                    a.d_output_ramp, a.ramp_stream_stride = self.ramp.data_ptr() + 4 * f0 * fs, fam.n
                if self.records is not None:
                    keep = torch.from_numpy(np.ascontiguousarray(self.records[:, f0:f0 + nf])).cuda()
                    setattr(a, "d_dmx_frames" if fam.kind == "down" else "d_demix_frames", keep.data_ptr())
                ns = [batches[0].render_ex(a)]
        self._take(out, pcms, ns)
        del keep

    def flush(self, batches, out):
        caps, pcms = self._pcms(240)
        self._take(out, pcms, [b.flush(p.data_ptr(), cap, self.st) for b, p, cap in zip(batches, pcms, caps)])

    def tickets(self, batches):
        """export of every member's whole batch -> [(blob, stride, tickets)]"""
        A, G, torch = _mods()
        got = []
        for b in batches:
            nbytes = b.stream_state_bytes()
            assert nbytes > 0 and nbytes % 16 == 0
            blob = torch.zeros((S, nbytes), dtype=torch.uint8, device="cuda")
            got.append((blob, nbytes, b.export_range(0, S, blob.data_ptr(), nbytes, self.st)))
        return got


def _reset_tallies(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)


def run(dev, D):
    """the recipe with the shift D -> ([member][stream] bytes of the source's PCM followed by the target's, the tallies of
    the base table, the extension and table 2)"""
    A, G, torch = _mods()
    fam = dev.fam
    out = [[[] for _ in range(S)] for _ in fam.ocs]
    src = tgt = None
    with R.environment(fam.env):
        _reset_tallies(A)
        try:
            src = dev.open()
            if fam.trim:      # a first frame trimmed at its start: the stream stands off the 16-sample grid for good
                dev.render(src, out, 0, 1, trim=fam.trim)
                dev.render(src, out, 1, fam.head_frames - 1)
            else:
                dev.render(src, out, 0, fam.head_frames)
            moved = dev.tickets(src)
            tgt = dev.open()
            Q = fam.pos + D
            for b, (blob, stride, tickets) in zip(tgt, moved):
                assert all(t.cursor[0] == fam.pos and t.cursor[1] == 0 for t in tickets), [tuple(t.cursor) for t in tickets]
                shifted = [A.StreamState.from_buffer_copy(bytes(t)) for t in tickets]
                for t in shifted:
                    t.cursor[0] += D
                b.import_range(0, S, blob.data_ptr(), stride, shifted, dev.st)
            f0 = fam.head_frames
            for nf in fam.calls:
                dev.render(tgt, out, f0, nf)
                f0 += nf
            for _, _, tickets in dev.tickets(tgt):
                assert all(t.cursor[0] == Q + 4 * 1024 - 96 * (fam.fs == 1000) and t.cursor[1] == 0 for t in tickets), \
                    (Q, [tuple(t.cursor) for t in tickets])
            dev.flush(tgt, out)
            for _, _, tickets in dev.tickets(tgt):   # (a batch without limiter has nothing to flush and stays open)
                assert all(t.cursor[1] == int(fam.limiter) for t in tickets), [tuple(t.cursor) for t in tickets]
        finally:
            for b in (src or []) + (tgt or []):
                b.close()
        tallies = (A.route_tally(), A.route_tally_ext(), A.route_table_tally(2, reset=True))
    return [[np.concatenate(o) for o in member] for member in out], tallies


def expected_tallies(fam):
    """the source's whole-frame call and the target's three take the family's instance; a trimmed first frame and every
    member's flush take the generic kernel"""
    K = len(fam.ocs)
    generic = [(R.gen(fam.m), (K if fam.limiter else 0) + (1 if fam.trim else 0))]
    inst = [(fam.inst, 4)]
    exp = [{}, {}, {}]
    for table, rows in ((0, generic), (fam.table, inst)):
        for k, v in rows:
            if v:
                exp[table][k] = exp[table].get(k, 0) + v
    return tuple(exp)


def view(dev, raw, oc):
    A, G, torch = _mods()
    n = raw.size // (oc * dev.bps)
    return G._view(raw, n, oc, dev.fmt)


@pytest.mark.parametrize("fam", LPOS.FAMILIES, ids=lambda f: f.id)
def test_family_across_the_boundaries(fam):
    fam.make()
    dev = Device(fam)
    control, tallies = run(dev, 0)
    assert tallies == expected_tallies(fam), (tallies, expected_tallies(fam))
    want = [[fam.want(s, j) for s in range(S)] for j in range(len(fam.ocs))]
    lsb = 1 if fam.mfma else 0

    def against_the_oracle(got, what):
        for j, oc in enumerate(fam.ocs):
            for s in range(S):
                g, w = view(dev, got[j][s], oc), want[j][s]
                if fam.bd == -32:
                    assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (fam.id, what, j, s)
                else:
                    R.compare(g, w, lsb, (fam.id, what, j, s))

    against_the_oracle(control, "control")
    for name, D, _ in fam.shifts:
        got, t = run(dev, D)
        for j in range(len(fam.ocs)):
            for s in range(S):
                assert np.array_equal(got[j][s], control[j][s]), "%s, %s: member %d stream %d differs from the control" % (
                    fam.id, name, j, s)
        against_the_oracle(got, name)
        assert t == tallies, "%s, %s: launched %s, the control %s" % (fam.id, name, t, tallies)


def test_mixed_positions_inside_one_batch():
    """the five-stream rig of tests/test_gpu_lifecycle.py: streams 1..2 are exported after two frames and imported into
    their own slots shifted to just below 2^31, streams 0, 3 and 4 stay where they are.  A range that spans both groups is
    refused with INVALID_STATE and writes nothing; rendered group by group, every stream matches the oracle, on the fast
    kernel throughout."""
    A, G, torch = _mods()
    W, n_streams = 6, 5
    rig = Rig("fast", n_streams, W)
    fs, m = rig.fs, rig.m
    import synth
    x = [synth.hot(5100 + s, m, W * fs, burst_phase=LPOS.BURST_PHASE - 30 + 15 * s, burst_period=LPOS.BURST_PERIOD)
         for s in range(n_streams)]
    for s in range(n_streams):
        rig.put(s, 0, x[s])
    A.route_reset()
    rig.render(0, 0, n_streams, 2)
    nbytes = rig.b.stream_state_bytes()
    blob = torch.zeros((2, nbytes), dtype=torch.uint8, device="cuda")
    tickets = rig.b.export_range(1, 2, blob.data_ptr(), nbytes, rig.st)
    D = LPOS.SHIFTS[0][1]
    for t in tickets:
        assert t.cursor[0] == 2 * fs
        t.cursor[0] += D
    rig.b.import_range(1, 2, blob.data_ptr(), nbytes, tickets, rig.st)
    groups = ((0, 1), (1, 2), (3, 2))
    for s0, cnt in ((0, 5), (0, 2), (2, 2), (1, 4)):
        cap = fs * rig.ch * 2
        pcm = torch.full((n_streams, cap), FILL, dtype=torch.uint8, device="cuda")
        a = A.RenderArgs()
        a.d_in, a.in_stream_stride, a.in_frame_stride = rig.xin.data_ptr() + 4 * 2 * m * fs, W * m * fs, m * fs
        a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = 1, pcm.data_ptr(), cap, rig.st
        with pytest.raises(A.IamfHipError) as e:
            rig.b.render_range(a, s0, cnt)
        assert e.value.code == INVALID_STATE, (s0, cnt, e.value.code)
        torch.cuda.synchronize()
        assert bool((pcm == FILL).all()), "a refused call wrote PCM"
    for wall, nf in ((2, 1), (3, 2), (5, 1)):
        for s0, cnt in groups:
            rig.render(wall, s0, cnt, nf)
    blob5 = torch.zeros((n_streams, nbytes), dtype=torch.uint8, device="cuda")
    moved = rig.b.export_range(0, n_streams, blob5.data_ptr(), nbytes, rig.st)
    assert [t.cursor[0] for t in moved] == [W * fs + (D if s in (1, 2) else 0) for s in range(n_streams)]
    for s0, cnt in groups:
        rig.flush(s0, cnt)
    tally = A.route_tally()
    R.check_tally(tally, {("FAST", 0, m, 2, 0): 1 + 3 * len(groups), R.gen(m): len(groups)})
    for s in range(n_streams):
        same(rig.take(s), rig.want(x[s]), ("mixed positions", s))
    rig.close()
