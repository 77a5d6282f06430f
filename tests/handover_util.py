"""State hand-over between every pair of render kernel families that can meet on one batch (tests/test_gpu_handover.py,
tests/test_handover_cpu.py): the table of families per batch class, the boundaries, the programmes, the case list, the oracle
and the driver.  Importing this module needs numpy only.

render_route.hpp: "all share the persisted per-stream state, so consecutive calls of one stream may take different ones".
A case is (class, A, B, b): family A renders call 1 of b samples, family B call 2, iamf_hip_batch_flush ends the stream.

The table (ROWS): one row per (class, family) — the entry point, the environment switches and the rule (`kind`) that says
which call lengths and stream positions make pick_route() choose the family.  Classes:

  N    16 channels into stereo s16: FAST(0), GENERIC, FAST_RAGGED, LPCM early / late, LPCM24, FANOUT and FANOUT_LPCM (K = 2,
       the sibling a mono batch; in a case that names a fan-out family every call is made on both members — the other
       family's call on each in turn — and both members are checked)
  NC   5.1 into stereo: LPCM_COUPLED early / late, LPCM_MONO (the element as mono sub-streams: 6 is no LpcmM, the path is
       unfused by design — the unpacker, then FAST), FAST, GENERIC, FAST_RAGGED
  N2   16 channels and a mono second element: FAST(1), LPCM_MIX (LP2 = 1), GENERIC
  N2P  the same with a stereo second element, whose packets are one coupled pair: FAST(1), LPCM_MIX (LP2 = 2), GENERIC (a
       batch has ONE second element, so the two LP2 variants of the listing need a class each)
  ND   7.1 through the parametric down-mixer into stereo: FAST_DOWN, GENERIC
  NI   frame_size == 1, stereo: FAST_INTERLEAVED, GENERIC
  W    7.1.4 into Sound System J, exact projection: WIDE4(0), WIDE(0), GENERIC
  WM   the same with MFMA projection: WIDE4(1), WIDE(1), GENERIC; +-1 LSB, no state comparison
  WX   W with a mono second element: WIDE4_MIX, GENERIC
  WD   7.1.4 through the down-mixer into 5.1.4: WIDE4_DOWN, GENERIC
  WS   scalable 7.1.4 (layers stereo, 5.1.2, 7.1.4) through the demixer into Sound System J: WIDE4_DEMIX, GENERIC
  WL   3rd-order ambisonics into 5.1 with the LFE generator: WIDE4_LFE, GENERIC (d_lfe_state is part of the exported blob)

Out of scope (EXCLUDED): NOLIM keeps no state; FIR_SPLIT / FIR_FUSED have no bit-exact reference and d_fir_hist is not
exportable; the resampler's kernels are no render families; the façade's and the groups' internal batches are not reachable
call by call.

Boundaries b: 1024 (chunk-aligned), 1088 (total & 1023 = 64, below WIDE4's 256), 1280 (WIDE4's short last chunk), 1000 (off
the 16-grid, at or above 240: only GENERIC and FAST_RAGGED end there; WIDE and WIDE4_LFE must not start there — the tally says
GENERIC), 100 (below 240 and off the grid: every B falls to GENERIC, one case per class).  Call 2 has 2048 samples; 1000 for
FAST_RAGGED, and for GENERIC behind b = 1024, where the length and no switch picks it.

The frame size follows from the ABI: a call is whole frames or at most one trimmed frame, so no single frame size forms all
of 1024, 1088, 1280, 1000 and 2048.  frame_size(b, n2): 1024 for b in (1024, 1000, 100); for b in (1088, 1280) frames of 64
in front of a call of 2048 and ONE frame of b in front of a trimmed call of 1000.  Class NI always has frame_size 1.  Class
WS: the in-register demixer takes frames of 256 samples or more (iamf_render.hip: demix_w4), so b = 1280 has frames of 256, and
at b = 1088 — which shares no such frame with 2048 — WIDE4_DEMIX renders a call 2 of 1024 samples, one frame of 1088 trimmed.

The programmes: 6 streams per batch, one limiter phase per stream at the boundary (PHASES), placed relative to b, on the
16-bit grid (k / 32768), so f32, 16-bit packets and 24-bit packets (k * 256) carry the identical signal.  Peak amplitudes come
from the oracle alone: a probe of the class's chain in front of the limiter gives the response at each peak, and the peak is
scaled to its target (T1 = 0.95 or T2 = 1.08, the threshold being 0.891).  tests/test_handover_cpu.py proves every phase from
oracle_lib.limiter_trace.  At b = 100 no stream can be in its release (the look-ahead window alone is 240 samples): the
release and re-trigger streams put their first peak on sample 0 and are still limiting at the boundary.

Number of cases: 490 (N 185, NC 103, N2 31, N2P 31, ND 15, NI 17, W 28, WM 28, WX 13, WD 13, WS 13, WL 13), reported in 38 groups by
(class, A); tests/test_handover_cpu.py asserts the literals N_CASES / CASES_PER_CLASS against the list."""
from collections import namedtuple

import numpy as np

import route_cases as R

S = 6
EGS, OGS = [1.1, 1.25, 0.9], [1.0, 0.9, 1.3]      # three gain sets, products 1.1, 1.125, 1.17
PHASES = ("idle", "look-ahead", "mid-attack", "release", "re-trigger", "edge")
BOUNDARIES = (1024, 1088, 1280, 1000, 100)
N2 = 2048
T1, T2 = 0.95, 1.08
SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED",
            "IAMF_HIP_RAGGED_UNFUSED", "IAMF_HIP_INTERLEAVED_UNFUSED", "IAMF_HIP_PROJECTION", "IAMF_HIP_DENSE")
FORCE = {"IAMF_HIP_FORCE_GENERIC": "1"}
N_CASES = 490
CASES_PER_CLASS = {"N": 185, "NC": 103, "N2": 31, "N2P": 31, "ND": 15, "NI": 17, "W": 28, "WM": 28, "WX": 13, "WD": 13, "WS": 13,
                   "WL": 13}

# ------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------

# kind: the rule of pick_route() the row rests on —
#   aligned    whole 64-sample blocks, at a position that is a multiple of 16 or at least 240 (fast_shape_ok)
#   ragged     NO whole number of blocks, the same positions (ragged_shape_ok)
#   any        any length, the same positions (interleaved_shape_ok)
#   wide4      whole blocks whose rest of a 1024-chunk is 0 or at least 256, the same positions (wide4_shape_ok, pos_any)
#   wide4_16   the same at a multiple of 16 only (the LFE variant: pos16)
#   wide       whole blocks at a multiple of 16; IAMF_HIP_NO_WIDE4 where the length is wide4's
#   generic    everything; IAMF_HIP_FORCE_GENERIC where another family would take the length, nothing else
#   generic1   everything through iamf_hip_batch_render_range on a frame_size == 1 batch, no switch
# key: the tally row of one launch, "m" / "oc" standing for the batch's (a fan-out's member count is the k field)
Row = namedtuple("Row", "cls fam entry env kind key")


def _rows():
    def gen(cls, kind="generic"):
        return Row(cls, "GENERIC", "range", {}, kind, ("GENERIC", 0, "m", 0, 0))
    late = {"IAMF_HIP_LP_LATE": "1"}
    return [
        Row("N", "FAST", "range", {}, "aligned", ("FAST", 0, "m", "oc", 0)),
        gen("N"),
        Row("N", "FAST_RAGGED", "rag", {}, "ragged", ("FAST_RAGGED", 0, "m", "oc", 0)),
        Row("N", "LPCM_EARLY", "lpcm16", {}, "aligned", ("LPCM", 1, "m", "oc", 0)),
        Row("N", "LPCM_LATE", "lpcm16", late, "aligned", ("LPCM", 0, "m", "oc", 0)),
        Row("N", "LPCM24", "lpcm24", {}, "aligned", ("LPCM24", 1, "m", "oc", 0)),
        Row("N", "FANOUT", "fanout", {}, "aligned", ("FANOUT", 0, "m", 0, 2)),
        Row("N", "FANOUT_LPCM", "fanout_lpcm", {}, "aligned", ("FANOUT_LPCM", 0, "m", 0, 2)),
        Row("NC", "LPCM_COUPLED_EARLY", "lpcmc", {}, "aligned", ("LPCM_COUPLED", 1, "m", "oc", 0)),
        Row("NC", "LPCM_COUPLED_LATE", "lpcmc", late, "aligned", ("LPCM_COUPLED", 0, "m", "oc", 0)),
        Row("NC", "LPCM_MONO", "lpcm16", {}, "aligned", ("FAST", 0, "m", "oc", 0)),
        Row("NC", "FAST", "range", {}, "aligned", ("FAST", 0, "m", "oc", 0)),
        gen("NC"),
        Row("NC", "FAST_RAGGED", "rag", {}, "ragged", ("FAST_RAGGED", 0, "m", "oc", 0)),
        Row("N2", "FAST_MIX", "range", {}, "aligned", ("FAST", 1, "m", "oc", 0)),
        Row("N2", "LPCM_MIX", "lpcm_mix", {}, "aligned", ("LPCM_MIX", 0, "m", "oc", 1)),
        gen("N2"),
        Row("N2P", "FAST_MIX", "range", {}, "aligned", ("FAST", 1, "m", "oc", 0)),
        Row("N2P", "LPCM_MIX", "lpcm_mix", {}, "aligned", ("LPCM_MIX", 0, "m", "oc", 2)),
        gen("N2P"),
        Row("ND", "FAST_DOWN", "range", {}, "aligned", ("FAST_DOWN", 0, "m", "oc", 0)),
        gen("ND"),
        Row("NI", "FAST_INTERLEAVED", "il", {}, "any", ("FAST_INTERLEAVED", 0, "m", "oc", 0)),
        gen("NI", "generic1"),
        Row("W", "WIDE4", "range", {}, "wide4", ("WIDE4", 0, "m", "oc", 0)),
        Row("W", "WIDE", "range", {}, "wide", ("WIDE", 0, "m", 0, 0)),
        gen("W"),
        Row("WM", "WIDE4", "range", {}, "wide4", ("WIDE4", 1, "m", "oc", 0)),
        Row("WM", "WIDE", "range", {}, "wide", ("WIDE", 1, "m", 0, 0)),
        gen("WM"),
        Row("WX", "WIDE4_MIX", "range", {}, "wide4", ("WIDE4_MIX", 0, "m", "oc", 0)),
        gen("WX"),
        Row("WD", "WIDE4_DOWN", "range", {}, "wide4", ("WIDE4_DOWN", 0, "m", "oc", 0)),
        gen("WD"),
        Row("WS", "WIDE4_DEMIX", "range", {}, "wide4", ("WIDE4_DEMIX", 0, "m", "oc", 0)),
        gen("WS"),
        Row("WL", "WIDE4_LFE", "range", {}, "wide4_16", ("WIDE4_LFE", 0, "m", "oc", 0)),
        gen("WL"),
    ]


ROWS = _rows()
CLASS_NAMES = ["N", "NC", "N2", "N2P", "ND", "NI", "W", "WM", "WX", "WD", "WS", "WL"]

# the families of render_route.hpp's Family enum / of the listings that no row names, and why
EXCLUDED = {
    "NOLIM": "the limiter is off: the family keeps no state",
    "FIR_SPLIT": "no bit-exact reference, and d_fir_hist is not exportable",
    "FIR_FUSED": "no bit-exact reference, and d_fir_hist is not exportable",
    "RS_PLAIN": "the resampler: no render family, a state of its own",
    "RS_TILE": "the resampler: no render family, a state of its own",
    "RS_BLOCK": "the resampler: no render family, a state of its own",
    "RS_DIRECT": "the resampler: no render family, a state of its own",
}
# (and the façade's and the groups' internal batches: no call-by-call entry reaches them)

# the row family -> the family of the listings its key names
def listed_family(row):
    return row.key[0]


def rows_of(cls):
    return [r for r in ROWS if r.cls == cls]


def row(cls, fam):
    return [r for r in ROWS if r.cls == cls and r.fam == fam][0]


def _wide4_len(n):
    return n % 64 == 0 and ((n & 1023) == 0 or (n & 1023) >= 256)


def takes(r, n, pos):
    """the environment under which row r's entry, called for n samples at stream position `pos`, is routed to r's family by
    pick_route(); None where no switch makes it so"""
    pos_any = pos % 16 == 0 or pos >= 240
    k = r.kind
    if k == "aligned":
        return dict(r.env) if n % 64 == 0 and pos_any else None
    if k == "ragged":
        return dict(r.env) if n % 64 != 0 and pos_any else None
    if k == "any":
        return dict(r.env) if pos_any else None
    if k == "wide4":
        return dict(r.env) if _wide4_len(n) and pos_any else None
    if k == "wide4_16":
        return dict(r.env) if _wide4_len(n) and pos % 16 == 0 else None
    if k == "wide":
        if n % 64 or pos % 16:
            return None
        return {"IAMF_HIP_NO_WIDE4": "1"} if _wide4_len(n) else {}
    if k == "generic":
        return dict(FORCE) if n % 64 == 0 else {}
    if k == "generic1":
        return {}
    raise ValueError(k)


def frame_size(cls, b, n2):
    if cls == "NI":
        return 1
    if cls == "WS" and b == 1280 and n2 == N2:
        return 256          # the in-register demixer takes frames of 256 samples or more (iamf_render.hip: demix_w4)
    if b in (1024, 1000, 100):
        return 1024
    return 64 if n2 == N2 else b


Case = namedtuple("Case", "cls a b_row b n2 fs env_a env_b fam_a fam_b")
# a, b_row: the rows; fam_a, fam_b: the rows whose key the tally must show (b_row, or the class's GENERIC where b_row's family
# must not take the position)


def _second_length(r, b):
    if r.kind == "ragged":
        return 1000
    if r.cls == "WS" and r.kind == "wide4" and b == 1088:
        return 1024         # 1088 and 2048 share no frame of 256 samples or more: ONE frame of 1088, then that frame trimmed to 1024
    if r.kind == "generic" and b == 1024:
        return 1000
    return N2


def cases_of(cls):
    rows = rows_of(cls)
    gen = row(cls, "GENERIC")
    out = []
    for a in rows:
        for br in rows:
            for b in BOUNDARIES[:4]:
                n2 = _second_length(br, b)
                ea, eb = takes(a, b, 0), takes(br, n2, b)
                if ea is None:
                    continue
                if eb is None:
                    # the families that keep absolute ring positions must NOT start off the 16-grid: the tally says GENERIC
                    if b == 1000 and br.kind in ("wide", "wide4_16") and a is gen:
                        env = {"IAMF_HIP_NO_WIDE4": "1"} if br.kind == "wide" else {}
                        out.append(Case(cls, a, br, b, n2, frame_size(cls, b, n2), ea, env, a, gen))
                    continue
                out.append(Case(cls, a, br, b, n2, frame_size(cls, b, n2), ea, eb, a, br))
    # b = 100: below 240 and off the grid, every B falls to GENERIC; one case per class, B the class's first row
    a = [r for r in rows if r.kind in ("ragged", "any")] or [gen]
    br = rows[0]
    n2 = 1000 if br.kind == "ragged" else N2
    out.append(Case(cls, a[0], br, 100, n2, frame_size(cls, 100, n2), takes(a[0], 100, 0), dict(br.env), a[0], gen))
    return out


def all_cases():
    return [c for cls in CLASS_NAMES for c in cases_of(cls)]


def case_id(c):
    return "%s: %s -> %s at %d (+%d, frames of %d)" % (c.cls, c.a.fam, c.b_row.fam, c.b, c.n2, c.fs)


def groups():
    """the groups the cases are run and reported in: (class, A) -> its cases"""
    out = {}
    for c in all_cases():
        out.setdefault((c.cls, c.a.fam), []).append(c)
    return out


# ------------------------------------------------------------------------------------------
# the classes: shape, matrices, the chain in front of the limiter (oracle)
# ------------------------------------------------------------------------------------------

_DMX_MODES, _DMX_OFFS = (-1, 1, 2, 4, 5, 6, 0, 2), (0, 0, 37, 21, 0, -3, 4, 0)      # (an offset below 0: from the frame's end)


class Cls:
    """one batch class: m inputs, oc outputs; sib: the fan-out's sibling (a class of its own, mono)"""

    def __init__(self, name, m, oc, table=False, m2=0, down=None, lfe=False, mfma=False, like=None, demix=None):
        self.name, self.m, self.oc, self.table, self.m2, self.down, self.lfe, self.mfma, self.like = name, m, oc, table, m2, down, lfe, mfma, like
        self.demix = demix
        self._mats = None

    def mats(self):
        """((product, oracle) of element 0, the same of the second element or None)"""
        if self._mats is None:
            import iac_amd as A
            if self.down:
                first = (A.dmx_matrix(*self.down), None)
            elif self.like:       # the fan-out's sibling: output 0 of the class it stands beside, as a mono layout
                import oracle_lib as O
                w = CLASSES[self.like].mats()[0][0]._keep[:, :1].copy()
                first = R._custom(A, O, A.KIND_M2M, self.m, 1, w, 1)
            else:
                first = R.matrices(self.m, self.oc, table=self.table)
            second = R.matrices(self.m2, self.oc, table=False, salt=1) if self.m2 else None
            self._mats = (first, second)
        return self._mats

    def gains(self, s):
        return EGS[s % 3], OGS[s % 3]

    def eg2(self, s):
        return [0.6, 1.0, 0.9][s % 3]

    def dmx_schedule(self, n_frames, fs):
        return [(_DMX_MODES[f % 8], _DMX_OFFS[f % 8] % fs) for f in range(n_frames)]

    def demix_case(self, n_frames, fs):
        """demix_cases.make_case for the class's layer stack, its schedule of modes and recon gains repeated over n_frames"""
        import demix_cases as D
        dc = D.make_case(self.demix, default=(1, 3), offset=8, fs=fs, seed=782)
        dc["schedule"] = (dc["schedule"] * (n_frames // len(dc["schedule"]) + 1))[:n_frames]
        return dc

    def pre(self, s, x, x2, sizes, fs):
        """the oracle's chain in front of the limiter for stream s: x [m][total] (x2 [m2][total]) over calls of `sizes`
        -> [oc][total] f32.  As route_cases.run_matrix / run_down and test_gpu_programmes.run_second / run_down compose it."""
        import oracle_lib as O
        oc, n = self.oc, x.shape[1]
        (_, omx), second = self.mats()
        eg, og = self.gains(s)
        if self.down:
            d = O.Downmixer(*self.down)
            assert d.ok()
            d.set_mode_weight(1, 3)
            parts = []
            for (lo, hi), (mode, off) in zip(frames_of(sizes, fs), self.dmx_schedule(len(frames_of(sizes, fs)), fs)):
                xi = np.ascontiguousarray(x[:, lo:hi], dtype=np.float32)
                ns = hi - lo
                o = np.zeros((oc, ns), dtype=np.float32)
                off = min(off, ns)
                if off:
                    d.downmix(xi, o, 0, off)
                if mode > -1:
                    d.set_mode_weight(mode, -1)
                if ns > off:
                    d.downmix(xi, o, off, ns - off)
                parts.append(o)
            d.close()
            return np.ascontiguousarray(np.concatenate(parts, axis=1))
        if self.demix:      # sample by sample within a frame: a trimmed frame is the whole frame's first samples
            import demix_cases as D
            fr = frames_of(sizes, fs)
            xin = np.zeros((len(fr), self.m, fs), dtype=np.float32)
            for f, (lo, hi) in enumerate(fr):
                xin[f, :, :hi - lo] = x[:, lo:hi]
            dem = D.drive_demixer(O.lib(), "orc_demixer_", self.demix_case(len(fr), fs), xin)
            x = np.ascontiguousarray(np.concatenate([dem[f][:, :hi - lo] for f, (lo, hi) in enumerate(fr)], axis=1), dtype=np.float32)
        if self.lfe:
            y = np.ascontiguousarray(O.render_h2m_lfe(omx, x, oc, 48000, list(sizes)), dtype=np.float32)
        else:
            y = np.ascontiguousarray(O.render(omx, x, oc), dtype=np.float32)
        O.lib().orc_frame_gain_const(O.fp(y), oc, n, float(eg))
        z = np.zeros_like(y) + y
        if second:
            y1 = np.ascontiguousarray(O.render(second[1], x2, oc), dtype=np.float32)
            O.lib().orc_frame_gain_const(O.fp(y1), oc, n, float(self.eg2(s)))
            z = z + y1
        z = np.ascontiguousarray(z, dtype=np.float32)
        O.lib().orc_frame_gain_const(O.fp(z), oc, n, float(og))
        return z


CLASSES = {
    "N": Cls("N", 16, 2),
    "N.sib": Cls("N.sib", 16, 1, like="N"),
    "NC": Cls("NC", 6, 2),
    "N2": Cls("N2", 16, 2, m2=1),
    "N2P": Cls("N2P", 16, 2, m2=2),
    "ND": Cls("ND", 8, 2, down=(5, 1)),
    "NI": Cls("NI", 2, 2),
    "W": Cls("W", 12, 12, table=True),
    "WM": Cls("WM", 12, 12, table=True, mfma=True),
    "WX": Cls("WX", 12, 12, table=True, m2=1),
    "WD": Cls("WD", 12, 10, down=(7, 6)),
    "WS": Cls("WS", 12, 12, table=True, demix=[1, 3, 7]),
    "WL": Cls("WL", 16, 6, table=True, lfe=True),
}


def frames_of(sizes, fs):
    """[(lo, hi)] of every frame of calls of `sizes` samples: whole frames of fs, or one trimmed frame"""
    out, pos = [], 0
    for n in sizes:
        if n <= fs:
            out.append((pos, pos + n))
        else:
            assert n % fs == 0, (n, fs)
            out += [(pos + k * fs, pos + (k + 1) * fs) for k in range(n // fs)]
        pos += n
    return out


def call_frames(n, fs):
    """-> (n_frames, n_samples) of the ABI for a call of n samples"""
    if n < fs:
        return 1, n
    assert n % fs == 0, (n, fs)
    return n // fs, 0


# ------------------------------------------------------------------------------------------
# the programmes
# ------------------------------------------------------------------------------------------

def peaks(phase, b):
    """[(input sample, target level)] of the stream in `phase`"""
    first = max(b - 400, 0)
    return {"idle": [(b + 300, T1)],
            "look-ahead": [(b + 10, T1)],
            "mid-attack": [(b - 20, T1)],
            "release": [(first, T1)],
            "re-trigger": [(first, T1), (b + 5, T2)],
            "edge": [(b - 1, T1), (b, T1)]}[phase]


_PROG = {}


def _framed(cname):
    c = CLASSES[cname]
    return bool(c.down or c.demix)


def programme(cname, b, n2=N2, fs=None):
    """-> (ints [S][m][b + N2] int64 on the 16-bit grid, ints2 [S][m2][..] or None) of class cname at boundary b (where the
    chain in front of the limiter follows the frames — the down-mixers' and the demixer's coefficients —: [..][b + n2], for
    the frames of that case; everywhere else n2 and fs are not looked at).  Every peak is one sample on every channel at once,
    its sign per channel the sign of the channel's weight into output 0, its amplitude such that output 0 of the oracle's chain
    in front of the limiter reaches the target there."""
    if not _framed(cname) or fs is None:
        n2, fs = N2, frame_size(cname.split(".")[0], b, N2)
    key = (cname, b, n2, fs)
    if key in _PROG:
        return _PROG[key]
    if cname.endswith(".sib"):       # the fan-out's sibling renders the SAME element
        _PROG[key] = (programme(cname.split(".")[0], b)[0], None)
        return _PROG[key]
    c = CLASSES[cname]
    total = b + n2
    sizes = [b, n2]
    rng = np.random.default_rng(9100 + 7 * b + sum(ord(ch) for ch in cname.split(".")[0]))
    ints = rng.integers(-500, 501, size=(S, c.m, b + N2)).astype(np.int64)[:, :, :total]
    ints2 = rng.integers(-400, 401, size=(S, c.m2, b + N2)).astype(np.int64)[:, :, :total] if c.m2 else None
    for s in range(S):
        z2 = np.zeros((max(c.m2, 1), total), dtype=np.float32)
        # signs: an impulse per channel
        probe = np.zeros((c.m, total), dtype=np.float32)
        for ch in range(c.m):
            probe[ch, 8 + ch] = 0.5
        zp = c.pre(s, probe, z2[:c.m2], sizes, fs)
        sign = np.array([1.0 if zp[0, 8 + ch] >= 0 else -1.0 for ch in range(c.m)])
        # amplitudes: the response at each peak's place
        pk = peaks(PHASES[s], b)
        probe = np.zeros((c.m, total), dtype=np.float32)
        for p, _ in pk:
            probe[:, p] = 0.5 * sign
        zp = c.pre(s, probe, z2[:c.m2], sizes, fs)
        for p, level in pk:
            # output 0's: the least the peak reaches (the down-mixers, which take no gains here: the loudest output's)
            resp = float(np.abs(zp[:, p]).max() if c.down else abs(zp[0, p])) / 0.5
            assert resp > 0
            k = int(np.ceil(level / resp * 32768.0))
            assert k < 32768, (cname, b, s, p, "a peak of %.2f needs %.3f of full scale" % (level, k / 32768.0))
            ints[s, :, p] = (k * sign).astype(np.int64)
    _PROG[key] = (ints, ints2)
    return _PROG[key]


def floats(ints):
    return (ints.astype(np.float64) / 32768.0).astype(np.float32)


_PRE = {}


def limiter_input(cname, b, n2, fs):
    """[S][oc][b + n2]: what the limiter sees, per stream"""
    key = (cname, b, n2, fs)
    if key not in _PRE:
        c = CLASSES[cname]
        ints, ints2 = programme(cname, b, n2, fs)
        x = floats(ints)[:, :, :b + n2]
        x2 = floats(ints2)[:, :, :b + n2] if ints2 is not None else [None] * S
        _PRE[key] = np.stack([c.pre(s, np.ascontiguousarray(x[s]), None if x2[s] is None else np.ascontiguousarray(x2[s]), [b, n2], fs)
                              for s in range(S)])
    return _PRE[key]


_WANT = {}


def want(cname, b, n2, fs):
    """the oracle's PCM per stream, [S] of int16 [b + n2][oc] (240 samples of delay, then the flush's 240: the same count)"""
    import oracle_lib as O
    key = (cname, b, n2, fs)
    if key not in _WANT:
        z = limiter_input(cname, b, n2, fs)
        out = []
        for s in range(S):
            y, _ = O.limiter_run(np.ascontiguousarray(z[s]), [b, n2])
            out.append(O.pack(y, 16))
        _WANT[key] = out
    return _WANT[key]


def shapes(cls):
    """every (b, n2, fs) a case of the class renders"""
    return sorted({(c.b, c.n2, c.fs) for c in cases_of(cls)})


# ------------------------------------------------------------------------------------------
# the device side
# ------------------------------------------------------------------------------------------

def key_of(r, c):
    return tuple(c.m if v == "m" else (c.oc if v == "oc" else v) for v in r.key)


def reset_tallies(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)
    for fam in ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED"):
        A.route_family_tally(fam, reset=True)


def read_tallies(A):
    """every launch since reset_tallies: the base table, the extension table, table 2 and the by-family listings, as one dict"""
    out = dict(A.route_tally())
    for part in [A.route_tally_ext(), A.route_table_tally(2, reset=True)] + \
            [A.route_family_tally(fam, reset=True) for fam in ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED")]:
        for k, v in part.items():
            assert k not in out, k
            out[k] = v
    return out


class Rig:
    """the batches of one case (the class's, and its fan-out sibling where the case names a fan-out family), the programme
    and the calls.  call() renders one call through a row's entry and returns a record per member: the value returned, every
    stream's emitted bytes (every other byte of the PCM rows asserted 0xA5: gpu_util.rows_and_rest), the exported state."""

    def __init__(self, cls, b, n2, fs, sibling=False):
        import torch
        import iac_amd as A
        self.A, self.torch = A, torch
        self.cls, self.b, self.n2, self.fs = cls, b, n2, fs
        self.names = [cls] + ([cls + ".sib"] if sibling else [])
        self.cs = [CLASSES[n] for n in self.names]
        c = self.cs[0]
        self.ints, self.ints2 = programme(cls, b, n2, fs)
        self.x = floats(self.ints)
        self.x2 = floats(self.ints2) if self.ints2 is not None else None
        self.st = torch.cuda.current_stream().cuda_stream
        self.frame0 = 0          # frames rendered so far (the down-mixer's records are numbered through the stream)
        self.batches = []
        for k in self.cs:
            (mx, _), second = k.mats()
            bt = A.Batch(S, mx, k.oc, frame_size=fs, out_format=A.FMT_S16, limiter=True, lfe_hoa=k.lfe,
                         projection=A.PROJ_MFMA if k.mfma else A.PROJ_EXACT)
            self.batches.append(bt)
            if not k.down:
                bt.set_gains(element=[k.gains(s)[0] for s in range(S)], output=[k.gains(s)[1] for s in range(S)])
            if second:
                bt.set_second_element(second[0], [k.eg2(s) for s in range(S)])
        if c.down:
            self.dmx = self._dmx_records()
        if c.demix:
            F = len(frames_of([b, n2], fs))
            dc = c.demix_case(F, fs)
            self.batches[0].set_demixer(dc["layout"], dc["order"], dc["gains"], dc["offset"])
            self.demix = np.frombuffer(bytes(R.demix_frames(A, dc, S)), dtype=np.uint8).reshape(S, F, -1)
        self.sb = [bt.stream_state_bytes() for bt in self.batches]

    def close(self):
        for bt in self.batches:
            bt.close()

    def _dmx_records(self):
        import ctypes as C
        A, c = self.A, self.cs[0]
        L = A.lib()
        F = len(frames_of([self.b, self.n2], self.fs))
        sched = c.dmx_schedule(F, self.fs)
        frames = (A.DmxFrame * (S * F))()
        stt = A.DmxState()
        for s in range(S):
            L.iamf_hip_dmx_state_init(C.byref(stt))
            L.iamf_hip_dmx_set_mode_weight(C.byref(stt), 1, 3)
            for f, (mode, off) in enumerate(sched):
                fr = frames[s * F + f]
                fr.offset = off
                L.iamf_hip_dmx_coefficients(C.byref(stt), fr.prev)
                if mode > -1:
                    L.iamf_hip_dmx_set_mode_weight(C.byref(stt), mode, -1)
                L.iamf_hip_dmx_coefficients(C.byref(stt), fr.cur)
        return np.frombuffer(bytes(frames), dtype=np.uint8).reshape(S, F, -1)

    # ---- the inputs of one call ----
    def _planar(self, x, pos, n, nf, keep, second=False):
        import gpu_util as G
        import ragged_util as RU
        t, d_in, sst, fst = RU.place(np.ascontiguousarray(x[:, :, pos:pos + n]), nf, self.fs, G.second_layout(G.PAD16) if second else G.PAD16,
                                     np.nan)
        keep.append(t)
        return d_in, sst, fst

    def _interleaved(self, x, pos, n, keep):
        m = x.shape[1]
        ss = ((n * m + 3) & ~3) + 4
        h = np.full((S, ss), np.nan, dtype=np.float32)
        for s in range(S):
            h[s, :n * m].reshape(n, m)[:] = x[s, :, pos:pos + n].T
        t = self.torch.from_numpy(h).cuda()
        keep.append(t)
        return t.data_ptr(), ss, m

    def _packets(self, ints, pos, n, nf, bps, widths, perm, keep):
        """the call's samples as packet rows (lpcm_util.rows): frames [S][nf][ch][fs], what lies behind a trimmed frame's
        samples is zero -> the iamf_hip_lpcm_input of the call"""
        import lpcm_util as LP
        A = self.A
        m = ints.shape[1]
        fr = np.zeros((S, m, nf * self.fs), dtype=np.int64)
        fr[:, :, :n] = ints[:, :, pos:pos + n] * (256 if bps == 3 else 1)
        fr = fr.reshape(S, m, nf, self.fs).transpose(0, 2, 1, 3)
        dec = np.zeros_like(fr)
        dec[:, :, perm, :] = fr          # decoded channel perm[c] carries the element's channel c
        raw, L, row = LP.rows(dec, bps, True, widths, perm, head=16, pad=0, frame_size=self.fs)
        d_raw = self.torch.from_numpy(raw).cuda()
        keep.append(d_raw)
        inp = A.LpcmInput()
        inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
        inp.first_sample = 0
        return inp

    def _substreams(self, entry, m):
        import route_cases_lpcm_mix as LM
        if entry == "lpcmc" or (entry == "lpcm_mix" and m in LM.COUPLED_M):
            return LM.elem0_substreams(m, None)
        return [1] * m, list(range(m))[::-1]       # mono sub-streams, the element's channels in reverse order

    def call(self, r, pos, n):
        """row r's entry over n samples at position pos, on every member -> [record per member]"""
        import gpu_util as G
        A, torch, c = self.A, self.torch, self.cs[0]
        nf, ns = call_frames(n, self.fs)
        if self.fs == 1:
            nf, ns = n, 0
        keep = []
        rows = [G.pcm_rows(S, max(n, 240) * k.oc * 2, G.PAD16, 2) for k in self.cs]

        def args(j):
            a = A.RenderArgs()
            a.n_frames, a.n_samples, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, ns, rows[j][1], rows[j][2], self.st
            return a

        def f32(a):
            if self.fs == 1:
                a.d_in, a.in_stream_stride, a.in_frame_stride = self._interleaved(self.x, pos, n, keep)
            else:
                a.d_in, a.in_stream_stride, a.in_frame_stride = self._planar(self.x, pos, n, nf, keep)
            if c.m2:
                a.d_in2, a.in2_stream_stride, a.in2_frame_stride = self._planar(self.x2, pos, n, nf, keep, second=True)
            if c.down:
                d = torch.from_numpy(self.dmx[:, self.frame0:self.frame0 + nf].copy()).cuda()
                keep.append(d)
                a.d_dmx_frames = d.data_ptr()
            if c.demix:
                d = torch.from_numpy(self.demix[:, self.frame0:self.frame0 + nf].copy()).cuda()
                keep.append(d)
                a.d_demix_frames, a.demix_sample0 = d.data_ptr(), 0
            return a

        rets = []
        if r.entry in ("range", "rag", "il"):
            for j, bt in enumerate(self.batches):
                a = f32(args(j))
                rets.append({"range": bt.render_range, "rag": bt.render_ragged, "il": bt.render_interleaved}[r.entry](a, 0, S))
        elif r.entry in ("lpcm16", "lpcm24", "lpcmc"):
            bps = 3 if r.entry == "lpcm24" else 2
            widths, perm = self._substreams(r.entry, c.m)
            inp = self._packets(self.ints, pos, n, nf, bps, widths, perm, keep)
            for j, bt in enumerate(self.batches):
                rets.append(bt.render_lpcm(inp, args(j)))
        elif r.entry == "lpcm_mix":
            import route_cases_lpcm_mix as LM
            widths, perm = self._substreams(r.entry, c.m)
            in0 = self._packets(self.ints, pos, n, nf, 2, widths, perm, keep)
            w1, p1 = LM.elem1_substreams(c.m2, "pair" if c.m2 == 2 else "mono")
            in1 = self._packets(self.ints2, pos, n, nf, 2, w1, p1, keep)
            rets.append(self.batches[0].render_lpcm_mix(in0, in1, args(0)))
        elif r.entry == "fanout":
            assert len(self.batches) == 2 and ns == 0
            d_in, sst, fst = self._planar(self.x, pos, n, nf, keep)
            rets, fused = A.render_fanout(self.batches, d_in, sst, fst, nf, [p[1] for p in rows], [p[2] for p in rows], self.st)
            assert fused == 2, ("members in the shared launch", fused)
        elif r.entry == "fanout_lpcm":
            assert len(self.batches) == 2
            widths, perm = self._substreams(r.entry, c.m)
            inp = self._packets(self.ints, pos, n, nf, 2, widths, perm, keep)
            rets, report = A.render_fanout_lpcm(self.batches, inp, nf, [p[1] for p in rows], [p[2] for p in rows], self.st, n_samples=ns)
            assert report == (2, 1, 0), ("(members fused, input fused, unpacks)", report)
        else:
            raise ValueError(r.entry)
        self.frame0 += 1 if ns else nf
        torch.cuda.synchronize()
        return [self._record(j, rows[j][0], rets[j]) for j in range(len(self.batches))]

    def flush(self):
        import gpu_util as G
        rows = [G.pcm_rows(S, 240 * k.oc * 2, G.PAD16, 2) for k in self.cs]
        rets = [bt.flush(rows[j][1], rows[j][2], self.st) for j, bt in enumerate(self.batches)]
        self.torch.cuda.synchronize()
        return [self._record(j, rows[j][0], rets[j], export=False) for j in range(len(self.batches))]

    def _record(self, j, rows, ret, export=True):
        import gpu_util as G
        torch = self.torch
        pcm = G.rows_and_rest(rows, G.PAD16, ret * self.cs[j].oc * 2)
        state = None
        if export:
            d_state = torch.zeros((S, self.sb[j]), dtype=torch.uint8, device="cuda")
            tickets = self.batches[j].export_range(0, S, d_state.data_ptr(), self.sb[j], self.st)
            torch.cuda.synchronize()
            state = (d_state.cpu().numpy(), [(t.bytes, t.cursor[0], t.cursor[1]) for t in tickets])
        return dict(ret=ret, pcm=pcm, state=state)


def run(cls, steps, b, n2, fs, sibling=False):
    """steps: [(row, environment)] of call 1 and call 2; then the flush.  -> [(records per member, tally)] per step and for
    the flush"""
    import iac_amd as A
    rig = Rig(cls, b, n2, fs, sibling)
    out = []
    try:
        pos = 0
        for (r, env), n in zip(steps, (b, n2)):
            with R.environment(env):
                reset_tallies(A)
                recs = rig.call(r, pos, n)
                out.append((recs, read_tallies(A)))
            pos += n
        reset_tallies(A)
        recs = rig.flush()
        out.append((recs, read_tallies(A)))
    finally:
        rig.close()
    return out


_CONTROL = {}


def control(cls, b, n2, fs, sibling):
    """the same calls through iamf_hip_batch_render_range under IAMF_HIP_FORCE_GENERIC=1: once per (class, b, length)"""
    key = (cls, b, n2, fs, sibling)
    if key not in _CONTROL:
        gen = row(cls, "GENERIC")
        _CONTROL[key] = run(cls, [(gen, FORCE), (gen, FORCE)], b, n2, fs, sibling)
    return _CONTROL[key]


def expected_tally(r, cs, fanout_members=2):
    """the launches of one call through row r on the members cs"""
    out = {}
    if r.entry in ("fanout", "fanout_lpcm", "lpcm_mix"):
        out[key_of(r, cs[0])] = 1
        return out
    for c in cs:
        k = key_of(r, c)
        out[k] = out.get(k, 0) + 1
    return out


def state_mask(cname, nbytes):
    """the bytes of the exported blob that are compared (all of them: no entry is masked)"""
    return np.ones(nbytes, dtype=bool)


def check_case(case):
    """runs the case and asserts what tests/test_gpu_handover.py promises: every check is made, the case fails with the list"""
    import test_gpu_programmes as TP
    c0 = CLASSES[case.cls]
    sibling = "fanout" in (case.a.entry, case.b_row.entry) or "fanout_lpcm" in (case.a.entry, case.b_row.entry)
    names = [case.cls] + ([case.cls + ".sib"] if sibling else [])
    cs = [CLASSES[n] for n in names]
    got = run(case.cls, [(case.a, case.env_a), (case.b_row, case.env_b)], case.b, case.n2, case.fs, sibling)
    ref = control(case.cls, case.b, case.n2, case.fs, sibling)
    gen = row(case.cls, "GENERIC")
    bad = []

    def hold(ok, *what):
        if not ok:
            bad.append(" ".join(str(w) for w in what))

    # tallies: exactly the expected rows, one launch per call and member
    for k, fam in enumerate((case.fam_a, case.fam_b, gen)):
        exp = expected_tally(fam, cs)
        hold(got[k][1] == exp, "tally of %s:" % ("call 1", "call 2", "the flush")[k], sorted(got[k][1].items()), "expected", sorted(exp.items()))
        hold(ref[k][1] == expected_tally(gen, cs), "the control's tally, step %d:" % k, sorted(ref[k][1].items()))
    for j, name in enumerate(names):
        w = want(name, case.b, case.n2, case.fs)
        # shapes: the values returned
        rets = [got[k][0][j]["ret"] for k in range(3)]
        exp_rets = [max(case.b - 240, 0), case.n2 - max(240 - case.b, 0), 240]
        hold(rets == exp_rets and rets == [ref[k][0][j]["ret"] for k in range(3)], name, "returned", rets, "expected", exp_rets)
        # state: after call 1 and after call 2, bit for bit the control's (names the call that WROTE it)
        if not c0.mfma:
            for k in range(2):
                g, r = got[k][0][j]["state"], ref[k][0][j]["state"]
                hold(g[1] == r[1], name, "tickets after call %d:" % (k + 1), g[1], r[1])
                mask = state_mask(name, g[0].shape[1])
                for s in range(S):
                    d = np.flatnonzero((g[0][s] != r[0][s]) & mask)
                    hold(d.size == 0, name, "the state %s wrote in call %d, stream %d (%s): %d bytes differ from the control's, the first at "
                         "byte %d" % ((case.fam_a, case.fam_b)[k].fam, k + 1, s, PHASES[s], d.size, int(d[0]) if d.size else -1))
        # PCM: call 1, call 2 and the flush against the oracle's bytes
        for s in range(S):
            raw = np.concatenate([got[k][0][j]["pcm"][s] for k in range(3)])
            pcm = raw.view(np.int16).reshape(-1, cs[j].oc)
            d = TP.mismatch(pcm, w[s], 1 if c0.mfma else 0)
            hold(d is None, name, "PCM of stream %d (%s) against the oracle: %s" % (s, PHASES[s], d))
            if not c0.mfma:
                rraw = np.concatenate([ref[k][0][j]["pcm"][s] for k in range(3)])
                rd = TP.mismatch(rraw.view(np.int16).reshape(-1, cs[j].oc), w[s])
                hold(rd is None, name, "the control itself misses the oracle, stream %d: %s" % (s, rd))
    assert not bad, "\n    ".join(["%d checks failed" % len(bad)] + bad)
