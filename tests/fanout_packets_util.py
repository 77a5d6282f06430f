"""Shared by tests/test_gpu_zz_fanout_packets.py, tests/test_fanout_packets_cpu.py and tools/fanout_packets_rate.py: the
packet forms, elements, members and the driver of iamf_hip_batch_render_fanout_packets and its twins, on top of
fanout_lpcm_util.py and lpcm_util.py.  Nothing here needs a GPU until a drive is made.

Run as a programme (`python fanout_packets_util.py child FORM`) it renders one small case through the entry and prints a
JSON line {family tally, report, sha256 of every member's bytes}: the fresh child process of the environment-switch test."""
import hashlib
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fanout_lpcm_util as U
import iac_amd as A
import lpcm_util as LP

FAM = "FANOUT_PACKETS"
FAMILY = 51
# form -> (bytes per packet sample, coupled pairs, variant of the family's rows, the family of the member's single call)
FORMS = {"s24": (3, False, 1, "LPCM24"), "s16c": (2, True, 2, "LPCM_COUPLED"), "s24c": (3, True, 3, "LPCM24_COUPLED")}
# the element of M channels: ambisonics of order 1..3 (mono-coded), 5.1 / 7.1 / 5.1.4 / 7.1.4 (coupled)
ELEMENT = {4: "foa", 9: "soa", 16: "toa", 6: "L51", 8: "L71", 10: "L514", 12: "L714"}
FORM_M = {"s24": [4, 9, 16], "s16c": [6, 8, 10, 12], "s24c": [6, 8, 10, 12]}
FAN_K = [2, 3, 4]


def instance_rows():
    """the rows of the three instance lists of render_route.hpp (FanPk24MK, FanPk16cMK, FanPk24cMK), in listing order"""
    return [(FAM, FORMS[f][2], m, 0, k) for f in ("s24", "s16c", "s24c") for m in FORM_M[f] for k in FAN_K]


def instance(form, m, k):
    return (FAM, FORMS[form][2], m, 0, k)


def mats(element, layout):
    """(product matrix, oracle matrix) of an element into a layout"""
    import oracle_lib as O
    if element in U.ORDER:
        return A.get_h2m_matrix(U.ORDER[element], A.SS[layout]), O.get_h2m(U.ORDER[element], O.SS[layout])
    return A.get_m2m_matrix(A.SS[element], A.SS[layout]), O.get_m2m(O.SS[element], O.SS[layout])


def coupled_order(m):
    """(widths, perm) of a coupled element of m channels whose sub-streams come in a permuted order: the pairs last to first,
    then LFE, then C.  perm[c] = the decoded channel the renderer's channel c (L R C LFE, then the pairs) takes"""
    npairs = (m - 2) // 2
    widths = [2] * npairs + [1, 1]
    pair_of = lambda i: [2 * (npairs - 1 - i), 2 * (npairs - 1 - i) + 1]   # the renderer's pair i <- decoded pair npairs-1-i
    perm = pair_of(0) + [2 * npairs + 1, 2 * npairs]
    for i in range(1, npairs):
        perm += pair_of(i)
    assert sorted(perm) == list(range(m))
    return widths, perm


def packet_rows(form, ints, fs, le=True):
    """packet rows with head 8 and pad 8 of a form's element: mono-coded forms in reversed channel order (no run offset
    ascends), coupled forms in coupled_order().  -> (raw [S][F][row], layout, row bytes, x [S][m][F * fs] f32)"""
    bps, coupled = FORMS[form][:2]
    m = ints.shape[2]
    if not coupled:
        return U.reversed_rows(ints, fs, bps, le)
    widths, perm = coupled_order(m)
    raw, L, row = LP.rows(ints, bps, le, widths, perm, head=8, pad=8, frame_size=fs)
    return raw, L, row, U.decoded(ints, perm, bps)


def chunk_peaks(element, sp, x, chunk=1024):
    """per stream the peaks of the member's rendered, gained element in every chunk: [S][chunks]"""
    import oracle_lib as O
    oc = A.layout_channels(A.SS[sp["layout"]])
    omx = mats(element, sp["layout"])[1]
    g = U.gain_product(sp)
    out = []
    for s in range(x.shape[0]):
        y = np.abs(O.render(omx, x[s], oc)).max(axis=0) * g
        out.append([float(y[c0:c0 + chunk].max()) for c0 in range(0, y.size, chunk)])
    return out


def members_for(element, x, base):
    """The members of `base` with their thresholds chosen on the CPU for this element and these samples: half-way (in dB,
    rounded down to half a dB, at most -1 dB) between the loudest chunk of a quiet stream and the quietest chunk of a loud one.
    assert_condition then proves the choice."""
    out = []
    for sp in base:
        if not sp["limiter"]:
            out.append(dict(sp))
            continue
        peaks = chunk_peaks(element, sp, x)
        loud = min(min(p) for s, p in enumerate(peaks) if s % 2 == 0)
        quiet = max(max(p) for s, p in enumerate(peaks) if s % 2 == 1)
        assert quiet < loud, (element, sp["layout"], quiet, loud)
        mid_db = 10.0 * np.log10(quiet * loud)
        sp2 = dict(sp)
        sp2["thr_db"] = float(min(-1.0, np.floor(2.0 * mid_db) / 2.0))
        out.append(sp2)
    return out


def assert_condition(element, specs, x, chunk=1024):
    """every loud (even) stream exceeds every member's threshold in every chunk, no quiet (odd) stream ever does"""
    for sp in specs:
        if not sp["limiter"]:
            continue
        thr = 10.0 ** (sp["thr_db"] / 20.0)
        assert 0.7 <= U.gain_product(sp) <= 1.25
        for s, peaks in enumerate(chunk_peaks(element, sp, x, chunk)):
            print("condition %s -> %s %.1f dB stream %d (%s): chunk peaks %.3f .. %.3f against %.3f"
                  % (element, sp["layout"], sp["thr_db"], s, "loud" if s % 2 == 0 else "quiet", min(peaks), max(peaks), thr))
            if s % 2 == 0:
                assert min(peaks) > thr, (element, sp["layout"], s, min(peaks), thr)
            else:
                assert max(peaks) < thr, (element, sp["layout"], s, max(peaks), thr)


def assert_oracle(d, element, specs, x, fs):
    """s16 members against the oracle, stream by stream; x: [S][m][samples] = what was rendered"""
    import oracle_lib as O
    for j, sp in enumerate(specs):
        if sp["fmt"] != A.FMT_S16:
            continue
        oc = d.batches[j].oc
        omx = mats(element, sp["layout"])[1]
        for s in range(d.S):
            want = O.stream_run(omx, oc, x[s], fs, element_gain=sp["eg"], output_gain=sp["og"], loudness_on=int(sp["lg"] is not None),
                                loudness_gain=sp["lg"] if sp["lg"] is not None else 1.0, limiter_on=int(sp["limiter"]), thr_db=sp["thr_db"])
            assert np.array_equal(d.bytes_of(j, s).view(np.int16).reshape(-1, oc), want), "member %d stream %d differs from the oracle" % (j, s)


class Drive(U.Drive):
    """fanout_lpcm_util.Drive with the entry under test (fan), the old entry (fan_lpcm) and the twin's single calls
    (iamf_hip_batch_render_packets per member, in member order)"""

    def fan_lpcm(self, *a, **k):
        return U.Drive.fan(self, *a, **k)

    def fan(self, nf, first=0, n_samples=0, s0=0, cnt=None, before_call=None):
        cnt, f0 = self._range(s0, cnt)
        caps, pcms = self.bufs(n_samples or nf * self.fs)
        inp = self.lpcm_input(f0, first)
        after_call = before_call(self.st) if before_call else None     # (queued right in front of the call, on its stream)
        ns, rep = A.render_fanout_packets(self.batches, inp, nf, [p.rows.d_pcm for p in pcms], caps, self.st,
                                          n_samples=n_samples, stream0=s0, n_streams=cnt)
        if after_call:
            self.notes = getattr(self, "notes", []) + [after_call()]
        for j, n in enumerate(ns):
            self._take(j, pcms[j], n, s0, cnt)
        self.reports.append(rep)
        self._advance(s0, cnt, nf)
        return rep

    def single(self, nf, first=0, n_samples=0, s0=0, cnt=None):
        cnt, f0 = self._range(s0, cnt)
        caps, pcms = self.bufs(n_samples or nf * self.fs)
        inp = self.lpcm_input(f0, first)
        for j, b in enumerate(self.batches):
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, n_samples, pcms[j].rows.d_pcm, caps[j], self.st
            self._take(j, pcms[j], b.render_packets(inp, a, s0, cnt), s0, cnt)
        self._advance(s0, cnt, nf)

    def export(self):
        """every member's iamf_hip_batch_export_range blob of all streams: [K] numpy uint8 [S][bytes]"""
        out = []
        for b in self.batches:
            sb = b.stream_state_bytes()
            d_state = self.torch.zeros((self.S, sb), dtype=self.torch.uint8, device="cuda")
            b.export_range(0, self.S, d_state.data_ptr(), sb, self.st)
            self.torch.cuda.synchronize()
            out.append(d_state.cpu().numpy())
        return out


def case(form, m, base, S, F, fs, le=True, seed0=500, condition=True):
    """-> (element, specs, raw, L, row, x) of a form's element of m channels into the members `base` with thresholds chosen for
    it; the condition is asserted on the CPU here, before any GPU call"""
    element = ELEMENT[m]
    ints = U.ints16(S, F, m, fs, seed0=seed0, bps=FORMS[form][0])
    raw, L, row, x = packet_rows(form, ints, fs, le)
    narrow = [sp for sp in base if A.layout_channels(A.SS[sp["layout"]]) <= 2]
    chosen = {id(sp): sp2 for sp, sp2 in zip(narrow, members_for(element, x, narrow))}
    specs = [chosen.get(id(sp), sp) for sp in base]
    if condition:
        assert_condition(element, [chosen[id(sp)] for sp in narrow], x, chunk=1024)
    return element, specs, raw, L, row, x


def pair(form, m, base, S, F, fs, **kw):
    """(got, twin, element, specs, x): two drives on the same packets"""
    element, specs, raw, L, row, x = case(form, m, base, S, F, fs)
    mxs = [mats(element, sp["layout"])[0] for sp in specs]
    return Drive(mxs, specs, raw, L, row, x, fs, **kw), Drive(mxs, specs, raw, L, row, x, fs, **kw), element, specs, x


def reset_tallies():
    A.route_reset()
    A.route_tally_ext(reset=True)
    for t in range(2, A.lib().iamf_hip_route_tables()):
        A.route_table_tally(t, reset=True)
    for fam in all_family_names():
        A.route_family_tally(fam, reset=True)


def all_family_names():
    names = list(A.ROUTE_BY_FAMILY_ONLY)
    for d in (A.ROUTE_FAMILY_MORE, A.ROUTE_FAMILY_LATER, A.ROUTE_FAMILY_NEWER, A.ROUTE_FAMILY_OPEN, A.ROUTE_FAMILY_FANOUT):
        names += list(d)
    return names + ["LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED", "LPCM24"]


def tallies():
    """every tally there is, read and reset: {'base': .., 'ext': .., family name: ..} without the empty ones"""
    out = {"base": A.route_tally(), "ext": A.route_tally_ext()}
    for fam in all_family_names():
        out[fam] = A.route_family_tally(fam, reset=True)
    return {k: v for k, v in out.items() if v}


def _child(form):
    import torch
    torch.cuda.set_device(0)
    m = FORM_M[form][-1]
    got, twin, element, specs, x = pair(form, m, [U.A_S16, U.MONO_S16_M6], 4, 2, 1024)
    reset_tallies()
    rep = got.fan(2)
    got.flush()
    h = hashlib.sha256()
    for j in range(2):
        for s in range(4):
            h.update(got.bytes_of(j, s).tobytes())
    print(json.dumps({"fam": {repr(k): v for k, v in A.route_family_tally(FAM).items()}, "report": list(rep), "sha": h.hexdigest()}))
    got.close()
    twin.close()


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    _child(sys.argv[2])
