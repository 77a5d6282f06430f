"""-m gpu: the packet-fed render kernels wherever a caller may put its packets.

render_fast_kernel<.., LP> (16-bit packets, family LPCM), its LPB = 3 form (24-bit, LPCM24) and render_fanout_kernel<M, K, LP>
(FANOUT_LPCM) read a stream's packet rows through one buffer resource with 32-bit offsets, from a base computed in 64 bits;
lpcm_form() (iac_amd/csrc/lpcm_form.hpp) and fast_shape_ok() (render_route.hpp) decide which calls they take, and every
other call is unpacked to f32 first (iamf_hip_lpcm_unpack_frames).  Their own tests place the rows in one way: dense, at the
start of a fresh allocation.  Here the same programme — 3 streams, four 1024-sample frames, calls of 1 and 3 frames and the
flush, channels in reversed order, samples that drive the limiter — runs under every packet layout of tests/gpu_util.py
(the PK_ table there; tests/test_packet_layouts_cpu.py tests the helper), and asserts

  the launch tally   the named instance once per fused call, the f32 kernel once per unfused call, the general kernel for the
                     flush: FUSED below, which tests/route_host pins row by row without a GPU;
  the PCM            every stream and every n_emitted bit for bit the oracle's (oracle_lib.stream_run on ints / 2^15 or
                     ints / 2^23) and a twin's that ran under IAMF_HIP_LPCM_UNFUSED=1 on PK_DENSE;
  no stray write     gpu_util.rows_and_rest after every call and the flush.

Every byte of a packet allocation outside the runs is 0x7F / 0x80, so a load that strays, steps by the dense stride or
narrows a stream's base to 32 bits reads samples near full scale.  The far layouts (streams 2^31 + 16 bytes apart; frames
426 MB apart, at and one step beyond the 32-bit rule) write only the rows and their guards.  The 24-bit and fan-out cases
run again with the PCM rows padded, offset and far apart, which tests/test_gpu_layouts.py does for the 16-bit family."""
import functools
import gc

import numpy as np
import pytest

import fanout_lpcm_util as U
import gpu_util as G
import lpcm_util as LP
import route_cases as R

pytestmark = pytest.mark.gpu

BAD_ARG = -1
S, FS, F, CALLS = 3, 1024, 4, [1, 3]
SWITCHES = ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PROJECTION",
            "IAMF_HIP_NO_WIDE4")

# which of CALLS the packet-fed kernel takes under each layout (tests/route_host/route_host_check.cpp and
# route_host_lpcm24_check.cpp, packet_layout_rows: the same geometry, asserted there without a GPU)
FUSED = {
    G.PK_DENSE: (1, 1),
    G.PK_PAD16: (1, 1),
    G.PK_GRID: (1, 0),           # the call from frame 1 has d_raw 8 (16 bit) or 4 (24 bit) bytes off 16
    G.PK_OFF_BASE: (0, 0),
    G.PK_OFF_STRIDE: (0, 0),
    G.PK_FAR_STREAMS: (1, 1),
    G.PK_BOUND: (1, 1),
    G.PK_BEYOND: (1, 0),         # (3 + 2) * (B(3) + 16) + 2^24 >= 2^31: the 3-frame call is unpacked, at far frame strides
}
assert set(FUSED) == set(G.PK_LAYOUTS)

# (family, m, out channels, early prefetch)
SINGLE = [("LPCM", 16, 2, 1), ("LPCM", 1, 1, 0), ("LPCM", 9, 2, 0), ("LPCM24", 16, 2, 1), ("LPCM24", 16, 2, 0), ("LPCM24", 4, 1, 1)]
SINGLE_IDS = ["%s_m%d_oc%d_%s" % (f.lower(), m, oc, "early" if e else "late") for f, m, oc, e in SINGLE]
# (element, members): {A, mono} of a 3rd-order element, four renditions of a 1st-order one
FAN = [("toa", (0, 1)), ("foa", (0, 1, 2, 3))]
FAN_IDS = ["fanout_lpcm_m16_k2", "fanout_lpcm_m4_k4"]
PCM_SIDE = [G.PAD16, G.OFF_PCM, G.FAR_PCM]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _mods():
    import iac_amd as A
    import oracle_lib as O
    return A, O


def _variant(early):
    return {"IAMF_HIP_LP_EARLY": "1"} if early else {"IAMF_HIP_LP_LATE": "1"}


def _reset(A):
    A.route_reset()
    A.route_tally_ext(reset=True)
    A.route_table_tally(2, reset=True)


def _tallies(A):
    return A.route_tally(), A.route_tally_ext(), A.route_table_tally(2, reset=True)


def _some(d):
    return {k: v for k, v in d.items() if v}


@functools.lru_cache(maxsize=None)
def _programme(sb, m):
    """-> (raw [S][F][row], layout, row bytes, x [S][m][F * FS] f32: what the decoder would hand the renderer).  Runs at
    head g, pad g on the form's grid g and in reversed channel order: every offset differs, none ascends, and they are no
    more aligned than the form asks"""
    rng = np.random.default_rng(7000 + 100 * sb + m)
    ints = LP.ints(rng, S, F, m, FS, sb)
    full = 1 << (8 * sb - 1)
    ints[:, :, :, ::97] = (int(0.946 * full) * (-1) ** np.arange(ints[0, 0, 0, ::97].size))[None, None, None, :]   # bursts on every channel at once
    perm = [m - 1 - c for c in range(m)]
    g = G.pk_grid(sb)
    raw, L, row = LP.rows(ints, sb, True, [1] * m, perm, head=g, pad=g, frame_size=FS)
    x = (ints[:, :, perm, :].astype(np.float64) / float(full)).astype(np.float32)      # exact
    return raw, L, row, np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * FS)


@functools.lru_cache(maxsize=None)
def _matrices(sb, m, oc):
    """a matrix through which the programme drives the limiter in every stream (judged by the oracle's rendering)"""
    A, O = _mods()
    x = _programme(sb, m)[3]
    for table in (True, False):
        mx, omx = R.matrices(m, oc, table=table)
        if min(float(np.abs(O.render(omx, x[s], oc)).max()) for s in range(S)) > 0.95:
            return mx, omx
    raise AssertionError("the programme does not drive the limiter")


# ------------------------------------------------------------------------------------------
# the single call: LPCM and LPCM24
# ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _single_reference(fam, m, oc):
    """-> (the oracle's PCM per stream, the unfused twin's bytes per stream, what the twin's calls emitted); computed once
    per case and shared by every layout"""
    A, O = _mods()
    sb = 3 if fam == "LPCM24" else 2
    raw, L, row, x = _programme(sb, m)
    mx, omx = _matrices(sb, m, oc)
    want = [O.stream_run(omx, oc, x[s], FS) for s in range(S)]
    emitted = []
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        _reset(A)
        twin = LP.render_lpcm(mx, oc, raw, L, row, FS, CALLS, packets=G.PK_DENSE, emitted=emitted)
        base, ext, t2 = _tallies(A)
    assert base == {("FAST", 0, m, oc, 0): len(CALLS), R.gen(m): 1} and ext == {} and t2 == {}, (base, ext, t2)
    for a in want + twin:
        a.setflags(write=False)
    return want, twin, tuple(emitted)


def single_tally(fam, m, oc, early, fused, generic=False):
    """-> (base, ext, table 2) for calls fused as `fused` says; generic: the PCM breaks the 16-byte rule, so every call is
    unpacked and rendered by the general kernel"""
    if generic:
        return {R.gen(m): len(fused) + 1}, {}, {}
    inst = {(fam, early, m, oc, 0): sum(fused)}
    f32 = {("FAST", 0, m, oc, 0): len(fused) - sum(fused), R.gen(m): 1}
    if fam == "LPCM24":
        return _some(f32), {}, _some(inst)
    return _some({**f32, **inst}), {}, {}


def run_single(case, pk, pcm=G.DENSE, generic=False, refused=None):
    A, O = _mods()
    fam, m, oc, early = case
    sb = 3 if fam == "LPCM24" else 2
    raw, L, row, x = _programme(sb, m)
    mx, omx = _matrices(sb, m, oc)
    want, twin, twin_emitted = _single_reference(fam, m, oc)
    emitted = []
    with R.environment(_variant(early)):
        _reset(A)
        got = LP.render_lpcm(mx, oc, raw, L, row, FS, CALLS, layout=pcm, packets=pk, emitted=emitted, refused=refused)
        tallies = _tallies(A)
    print("tally %s m%d oc%d %s, packets %s, PCM %s: base %s ext %s table2 %s"
          % (fam, m, oc, "early" if early else "late", pk.name, pcm.name, *tallies))
    assert tallies == single_tally(fam, m, oc, early, FUSED[pk], generic), (pk.name, pcm.name, tallies)
    assert tuple(emitted) == twin_emitted, (emitted, twin_emitted)
    for s in range(S):
        g = got[s].view(np.int16).reshape(-1, oc)
        assert g.shape == want[s].shape and np.array_equal(g, want[s]), "%s: stream %d against the oracle" % (pk.name, s)
        assert np.array_equal(got[s], twin[s]), "%s: stream %d against the unfused twin" % (pk.name, s)


def _far(fn, *a, **kw):
    """a test that holds gigabytes: freed whatever happens, and the largest allocation reported"""
    import torch
    torch.cuda.reset_peak_memory_stats()
    try:
        fn(*a, **kw)
    finally:
        gc.collect()
        print("largest allocation: %.2f GB in all at the peak" % (torch.cuda.max_memory_allocated() / 1e9))
        torch.cuda.empty_cache()


@pytest.mark.parametrize("pk", G.PK_SMALL, ids=lambda l: l.name)
@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_single_call_under_every_small_packet_layout(case, pk):
    run_single(case, pk)


@pytest.mark.parametrize("pk", G.PK_FAR, ids=lambda l: l.name)
@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_single_call_under_the_far_packet_layouts(case, pk):
    _far(run_single, case, pk)


@pytest.mark.parametrize("pcm", PCM_SIDE, ids=lambda l: l.name)
@pytest.mark.parametrize("case", [c for c in SINGLE if c[0] == "LPCM24"], ids=[i for i in SINGLE_IDS if i.startswith("lpcm24")])
def test_lpcm24_with_the_pcm_rows_padded_offset_and_far_apart(case, pcm):
    """as ROUTED["LPCM"] of tests/test_gpu_layouts.py: the same instance under PAD16 and FAR_PCM; an offset PCM: unpacked,
    then the general kernel"""
    _far(run_single, case, G.PK_PAD16, pcm=pcm, generic=pcm == G.OFF_PCM)


@pytest.mark.parametrize("case", [SINGLE[0], SINGLE[3]], ids=[SINGLE_IDS[0], SINGLE_IDS[3]])
def test_a_stream_major_placement_is_refused_and_changes_nothing(case):
    """[F][S][row]: raw_stream_stride < n_frames * raw_frame_stride is a bad argument (lpcm_form_check); no PCM byte is
    written, and the same batch then renders the whole programme under PK_PAD16"""
    run_single(case, G.PK_PAD16, refused=(G.PK_FRAME_MAJOR, BAD_ARG, 1))


# ------------------------------------------------------------------------------------------
# the fan-out
# ------------------------------------------------------------------------------------------

def _fan_matrices(element, specs):
    A, O = _mods()
    out = []
    for sp in specs:
        out.append((A.get_h2m_matrix(U.ORDER[element], A.SS[sp["layout"]]), O.get_h2m(U.ORDER[element], O.SS[sp["layout"]])))
    return out


def _fan_setup(element, members):
    specs = [U.MEMBERS[j] for j in members]
    m = U.CHANNELS[element]
    raw, L, row, x = _programme(2, m)
    return specs, m, raw, L, row, x, _fan_matrices(element, specs)


@functools.lru_cache(maxsize=None)
def _fan_reference(element, members):
    """-> ({(member, stream): the twin's bytes}, what the twin's steps emitted per member): single calls per member under
    IAMF_HIP_LPCM_UNFUSED=1 on PK_DENSE.  The members of integer formats are also held against the oracle here, once."""
    A, O = _mods()
    specs, m, raw, L, row, x, mxs = _fan_setup(element, members)
    with R.environment({"IAMF_HIP_LPCM_UNFUSED": "1"}):
        _reset(A)
        twin = U.Drive([mx for mx, _ in mxs], specs, raw, L, row, None, FS, packets=G.PK_DENSE)
        try:
            for nf in CALLS:
                twin.single(nf)
            twin.flush()
        finally:
            twin.close()
        base, ext, t2 = _tallies(A)
    assert ext == {} and t2 == {} and not [k for k in base if k[0] in ("LPCM", "FANOUT")], (base, ext, t2)
    out = {(j, s): twin.bytes_of(j, s) for j in range(len(specs)) for s in range(S)}
    bd = {A.FMT_S16: 16, A.FMT_S24: 24, A.FMT_S32: 32}
    for j, sp in enumerate(specs):
        oc = twin.batches[j].oc
        for s in range(S):
            want = O.stream_run(mxs[j][1], oc, x[s], FS, element_gain=sp["eg"], output_gain=sp["og"], loudness_on=int(sp["lg"] is not None),
                                loudness_gain=sp["lg"] if sp["lg"] is not None else 1.0, limiter_on=int(sp["limiter"]), thr_db=sp["thr_db"],
                                bit_depth=bd[sp["fmt"]])
            got = G._view(out[(j, s)], out[(j, s)].size // (oc * U.BPS[sp["fmt"]]), oc, sp["fmt"])
            assert got.shape == want.shape and np.array_equal(got, want), "the twin's member %d, stream %d against the oracle" % (j, s)
    return out, [list(e) for e in twin.emitted]


def run_fan(element, members, pk, pcm=G.DENSE, singly=False, refuse_first=False):
    """the report and the tallies that include/iamf_hip.h documents: members whose single call runs the packet-fed kernel
    share one launch (n_fused = K, input_fused = 1, no unpack); a call the packet-fed kernels do not take is unpacked once
    and goes through the f32 fan-out (K, 0, 1); singly: every member's PCM breaks the 16-byte rule, so the f32 fan-out
    renders each member on its own with the general kernel (0, 0, 1)"""
    import torch
    A, O = _mods()
    specs, m, raw, L, row, x, mxs = _fan_setup(element, members)
    K = len(specs)
    want, want_emitted = _fan_reference(element, members)
    fused = FUSED[pk]
    _reset(A)
    d = U.Drive([mx for mx, _ in mxs], specs, raw, L, row, None, FS, packets=pk, pcm_layout=pcm)
    try:
        if refuse_first:
            pl = G.place_packets(raw, L, G.PK_FRAME_MAJOR, 0, 1)
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = pl.d_raw, pl.stream_stride, pl.frame_stride, L
            strides, pcms = d.bufs(FS)
            sentinel = A.FanoutReport(-7, -7, -7, -7)
            with pytest.raises(A.IamfHipError) as e:
                A.render_fanout_lpcm(d.batches, inp, 1, [p.rows.d_pcm for p in pcms], strides, d.st, report=sentinel)
            assert e.value.code == BAD_ARG
            assert (sentinel.n_fused, sentinel.input_fused, sentinel.n_unpacks, sentinel.reserved) == (-7, -7, -7, -7)
            torch.cuda.synchronize()
            for p in pcms:
                G.rows_and_rest(p.rows, pcm, 0)
            assert _tallies(A) == ({}, {}, {})
        reports = [d.fan(nf) for nf in CALLS]
        d.flush()
    finally:
        d.close()
    tallies = _tallies(A)
    print("tally fan-out m%d K%d, packets %s, PCM %s: reports %s base %s ext %s table2 %s" % (m, K, pk.name, pcm.name, reports, *tallies))
    if singly:
        assert reports == [(0, 0, 1)] * len(CALLS), reports
        assert tallies == ({R.gen(m): K * (len(CALLS) + 1)}, {}, {}), tallies
    else:
        assert reports == [(K, 1, 0) if f else (K, 0, 1) for f in fused], (pk.name, reports)
        base = _some({("FANOUT", 0, m, 0, K): len(fused) - sum(fused), R.gen(m): K})
        assert tallies == (base, _some({("FANOUT_LPCM", 0, m, 0, K): sum(fused)}), {}), (pk.name, tallies)
    assert d.emitted == want_emitted, (d.emitted, want_emitted)
    for j in range(K):
        for s in range(S):
            assert np.array_equal(d.bytes_of(j, s), want[(j, s)]), "%s: member %d, stream %d against the twin and the oracle" % (pk.name, j, s)


@pytest.mark.parametrize("pk", G.PK_SMALL, ids=lambda l: l.name)
@pytest.mark.parametrize("element,members", FAN, ids=FAN_IDS)
def test_fanout_under_every_small_packet_layout(element, members, pk):
    run_fan(element, members, pk)


@pytest.mark.parametrize("pk", G.PK_FAR, ids=lambda l: l.name)
@pytest.mark.parametrize("element,members", FAN, ids=FAN_IDS)
def test_fanout_under_the_far_packet_layouts(element, members, pk):
    _far(run_fan, element, members, pk)


@pytest.mark.parametrize("pcm", PCM_SIDE, ids=lambda l: l.name)
@pytest.mark.parametrize("element,members", FAN, ids=FAN_IDS)
def test_fanout_with_the_pcm_rows_padded_offset_and_far_apart(element, members, pcm):
    _far(run_fan, element, members, G.PK_PAD16, pcm=pcm, singly=pcm == G.OFF_PCM)


def test_the_fanout_refuses_a_stream_major_placement_and_changes_nothing():
    run_fan("toa", (0, 1), G.PK_PAD16, refuse_first=True)
