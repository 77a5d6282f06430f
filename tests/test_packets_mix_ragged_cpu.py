"""No GPU: iamf_hip_batch_render_packets_mix_ragged is declared, exported and bound, and takes the call struct of
iamf_hip_batch_render_packets_mix; its family (PACKETS_MIX_RAGGED = 39) lists exactly the 72 instances — the whole-block mix
families' (bed, outputs, second element) in 16 and in 24 bit — named as the launchers walk them, which no numbered table and no
other family lists; the tables and the other families are as they were; every instance has a GPU case; the refusals that need no
device answer IAMF_HIP_ERR_BAD_ARG, as the twin entry's; the routes the GPU tests assert are what the length, position and trim
rules give; and the limiter cases of the GPU tests are proven, from the oracle's limiter trace, to reach their branch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import iac_amd as A
import packets_mix_ragged_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def _header():
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        return f.read()


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_packets_mix_ragged" in names and hasattr(A.lib(), "iamf_hip_batch_render_packets_mix_ragged")
    for hidden in ("iamf_hip_fast_packets_mix_ragged_launch", "iamf_hip_fast_packets_mix_ragged_coupled_launch",
                   "iamf_hip_fast_packets_mix_ragged24_launch", "iamf_hip_fast_packets_mix_ragged24_coupled_launch"):
        assert hidden not in names       # the launch entries stay hidden
    with open(os.path.join(ROOT, "iac_amd", "csrc", "exports.map")) as f:
        assert re.search(r"global:[^}]*\biamf_hip_\*;", f.read(), flags=re.S)      # the map exports the entry by its prefix
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    proto = re.search(r"\bint\s+iamf_hip_batch_render_packets_mix_ragged\s*\(([^)]*)\)\s*;", src)
    assert proto and re.sub(r"\s+", " ", proto.group(1)).strip() == \
        "iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0, int32_t n_streams"
    assert re.search(r"IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED\s*=\s*%d\b" % U.FAMILY, src)
    assert A.ROUTE_FAMILY_NEWER == {U.FAM: U.FAMILY} and A.hipabi._family_id(U.FAM) == U.FAMILY and A.hipabi._family_name(U.FAMILY) == U.FAM
    for pinned in (A.ROUTE, A.ROUTE_BY_FAMILY_ONLY, A.ROUTE_FAMILY_MORE, A.ROUTE_FAMILY_LATER):
        assert U.FAM not in pinned and U.FAMILY not in pinned.values()
    assert A.hipabi._family_name(37) == "PACKETS_RAGGED" and A.hipabi._family_id("PACKETS_RAGGED") == 37 and A.hipabi._family_name(33) == "LPCM24_MIX"
    assert callable(A.Batch.render_packets_mix_ragged)
    assert A.lib().iamf_hip_batch_render_packets_mix_ragged.argtypes == A.lib().iamf_hip_batch_render_packets_mix.argtypes
    assert A.lib().iamf_hip_batch_render_packets_mix_ragged.argtypes[1]._type_ is A.PacketMixCall


def test_the_family_lists_72_instances_as_the_launchers_walk_them():
    rows = A.route_family_instances(U.FAM)
    assert rows == [U.inst(*i) for i in U.INSTANCES] and len(rows) == len(set(rows)) == 72
    assert A.route_family_instances(U.FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(U.FAMILY, None, 0) == 72
    # the same (bed, outputs, second element) as the two whole-block mix families, once per sample size
    for bps, whole in U.WHOLE.items():
        theirs = A.route_family_instances(whole)
        assert [(m, c, k) for _, v, m, c, k in rows if v == bps] == [(m, c, k) for _, _, m, c, k in theirs], whole
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == U.FAM], t
    for other in U.OTHER_FAMILIES + ("FAST", "LPCM", "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == U.FAM], other
    row = (A.RouteRow * 5)()
    assert A.lib().iamf_hip_route_family_instances(U.FAMILY, row, 5) == 72       # cap rows filled, the count returned
    assert all(r.family == U.FAMILY and r.variant == 2 and r.k in (1, 2) and r.launches == 0 for r in row)
    assert A.route_family_tally(U.FAM) == {} and A.route_family_tally(U.FAM, reset=True) == {}


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    counts = {"LPCM_COUPLED": 20, "LPCM_MIX": 36, "FAST_INTERLEAVED": 4, "FAST_RAGGED": 18, "LPCM24_COUPLED": 20, "LPCM24_MIX": 36, "LPCM": 16,
              "LPCM24": 16, "PACKETS_RAGGED": 36}
    for fam, n in counts.items():
        assert len(A.route_family_instances(fam)) == n, fam
    for fam in (18, 19, 24, 26, 28, 30, 32, 34, 35, 36, 38, 40, 41):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def test_every_instance_has_a_gpu_case():
    import test_gpu_zz_packets_mix_ragged as TG
    marks = [m for m in TG.test_every_instance.pytestmark if m.name == "parametrize"]
    cases = [U.inst(*i) for i in marks[0].args[1]]
    assert len(cases) == len(set(cases)) and cases == A.route_family_instances(U.FAM)
    for bps, m, oc, k in U.SHAPES.values():      # the shapes of the length, trim, ramp and switch tests are instances
        assert (bps, m, oc, k) in U.INSTANCES
    assert {U.SHAPES[n][0] for n in U.SHAPES} == {2, 3}


def _call(reserved=None, d_in=None, d_in2=None):
    call = A.PacketMixCall()
    for i in range(2):
        call.in_[i].d_raw, call.in_[i].raw_stream_stride, call.in_[i].raw_frame_stride = 0x1000 * (i + 1), 4096, 4096
    call.args.d_pcm, call.args.n_frames = 0x3000, 1
    call.args.d_in, call.args.d_in2 = d_in, d_in2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_reserved_words_and_f32_inputs_are_refused_without_a_device():
    """what iamf_hip_batch_render_packets_mix refuses before it looks at the batch, with its code"""
    L = A.lib()
    for entry in (L.iamf_hip_batch_render_packets_mix_ragged, L.iamf_hip_batch_render_packets_mix):
        assert entry(None, C.byref(_call()), 0, 1) == BAD_ARG
        assert entry(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
        assert entry(None, None, 0, 1) == BAD_ARG
        for i in range(4):    # (nor here: the reserved words are looked at before the batch)
            assert entry(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i
        assert entry(0x4000, C.byref(_call(d_in=0x2000)), 0, 1) == BAD_ARG
        assert entry(0x4000, C.byref(_call(d_in2=0x2000)), 0, 1) == BAD_ARG


def test_the_default_routes():
    """what the GPU tests assert per call is what the length, position and trim rules give"""
    def routes(calls, fs):
        return U.default_routes(U.Mix(2, 4, 2, 1, calls, fs))
    assert routes([(1, 0), (1, 145)], 1024) == [U.WHOLE_ROW, U.RAG]
    assert routes([(3, 0)], 1000) == [U.RAG] and routes([(5, 0), (5, 0)], 120) == [U.RAG, U.RAG]
    assert routes([(1, 100), (1, 900), (1, 0), (1, 0)], 1000) == [U.RAG, U.GENERIC, U.RAG, U.RAG]
    assert routes([(1, 0), (1, 41, 3)], 1000) == [U.RAG, U.GENERIC] and routes([(1, 0), (1, 41, 951)], 1000) == [U.RAG, U.GENERIC]
    assert routes([(1, 0), (1, 354, 212)], 576) == [U.WHOLE_ROW, U.RAG]
    assert routes([(1, 1025)], 4100) == [U.RAG] and routes([(1, 2049)], 2052) == [U.RAG]


def test_the_oracle_of_trimmed_calls_takes_the_calls_samples():
    """Mix.kept() and want_any(): a call trimmed to n samples from first on takes exactly those samples of its frame"""
    mix = U.Mix(3, 6, 2, 1, [(1, 0), (1, 145, 4), (2, 0)], 512)
    kept = mix.kept()
    assert [len(k) for k in kept] == [512, 145, 1024] == mix.sizes()
    assert kept[1][0] == 512 + 4 and kept[1][-1] == 512 + 4 + 144 and kept[2][0] == 1024
    assert mix.want_any(0).shape == (512 + 145 + 1024, 2)
    z, y0, y1 = mix.pre_limiter(0)
    mix.assert_drives_the_limiter(0, z, y0, y1)


# ---- the limiter cases ----

@pytest.mark.parametrize("bps", [2, 3])
@pytest.mark.parametrize("name", sorted(U.LIM_CASES))
def test_the_limiter_cases_reach_their_branch(name, bps):
    """from oracle_lib.limiter_trace alone (step k is the one input sample k enters at; a peak on input p triggers at step
    p + 1): the first call stays idle; the case's first trigger falls where its name says; the limiter is in attack or release,
    with a gain below 1, at every call boundary behind it — the release runs across the ragged call, the whole-block call and
    the f32 call that follow"""
    import oracle_lib as O
    mix = U.lim_mix(name, bps=bps)
    sz = mix.sizes()
    ends = [int(e) for e in np.cumsum(sz)]
    assert sz == [1000, 1000, 1000, 1000, 960, 1000]
    for s in range(mix.S):
        z, _, _ = mix.pre_limiter(s)
        y, t = O.limiter_trace(z, sz)
        trig = np.flatnonzero(t & O.LIM_TRIGGER)
        p = mix.peak - s
        assert trig.size and int(trig[0]) == p + 1, (name, s, trig[:3])
        assert not (t[:p + 1] & 3).any(), (name, s, "idle up to the peak")
        if name == "trigger_in_the_last_partial_block":
            assert 1000 + 960 <= p + 1 < 2000          # samples 960 .. 999 of the second call: its sixteenth, partial block
        elif name == "peak_on_the_last_real_sample" and s == 0:
            assert p == 1999 and int(trig[0]) == 2000   # the second call's last sample; the trigger is the third call's first step
        elif name == "release_across_the_next_call":
            assert 1240 <= p < 1760
        for e in ends[:-1]:
            if e - 1 <= p + 1:      # (the trigger's own step still reports the phase it found)
                continue
            assert (t[e - 1] & 3) != O.LIM_IDLE and (t[e] & 3) != O.LIM_IDLE, (name, s, e)
        for e in ends[2:-1]:                          # the gain is below 1 on what leaves around the boundary
            j = e - 240
            c = int(np.argmax(np.abs(z[:, j])))
            assert z[c, j] != 0.0 and abs(y[c, j]) < abs(z[c, j]), (name, s, e)
        assert (t[ends[2]:ends[-1]] & 3 == O.LIM_RELEASE).all(), (name, s, "the release runs across the last three calls")


# ---- the façade and group cases ----

def test_the_stored_fuzz_sets_hold_streams_for_every_two_element_packet_form():
    """the streams tests/test_gpu_zz_packets_mix_facade.py decodes are selected by configuration from the stored fuzz sets, whose
    PCM hashes come from the real reference: at least one with a ragged mix frame, one whose whole-block frames are 16-bit and
    one whose are 24-bit, one with gain ramps; every selected instance is one the library lists"""
    import json
    import e2e_fuzz as F
    sel = U.facade_mix_streams()
    assert len(sel) >= 3, sel
    assert [s for s in sel if s[2]["ragged"]], "no stream with a frame for the ragged two-element form"
    assert [s for s in sel if s[2]["whole"] and s[2]["inst"][0] == 2] and [s for s in sel if s[2]["whole"] and s[2]["inst"][0] == 3], sel
    assert [s for s in sel if F.case(s[1], s[0]).get("pair_ramps")], "no stream with gain ramps"
    for v, seed, fr in sel:
        c = F.case(seed, v)
        assert len(c["pair"]) == 2 and c["fs"] % 4 == 0 and c["sample_size"] in (16, 24), (v, seed)
        assert U.inst(*fr["inst"]) in A.route_family_instances(U.FAM) and U.whole(*fr["inst"]) in A.route_family_instances(U.WHOLE[fr["inst"][0]])
        want = json.load(open(os.path.join(ROOT, "tests", "golden", "fuzz.json" if v == "default" else "fuzz_%s.json" % v)))[str(seed)]
        assert "sha256" in want and "rets" in want, (v, seed)      # (the reference decoded it: there is a hash to hold the PCM against)
        for f in fr["ragged"]:
            s0, te = c.get("trims", {}).get(f, (0, 0))
            assert s0 % 4 == 0 and (c["fs"] - s0 - te) % 64, (v, seed, f)


def test_the_facade_rule_leaves_out_what_the_handle_does_not_take():
    base = dict(pair=("toa", "stereo"), sample_size=16, layout=("ss", 0), fs=1000, frames=3, trims={2: (0, 855)})
    fr = U.facade_mix_frames(base)
    assert fr == dict(inst=(2, 16, 2, 2), ragged=[0, 1, 2], whole=[], f32=[])
    assert U.facade_mix_frames(dict(base, trims={0: (3, 0)}))["f32"] == [0]                   # a start off a multiple of 4: the f32 path
    assert U.facade_mix_frames(dict(base, fs=1024, trims={}))["whole"] == [0, 1, 2]
    for other in (dict(pair=("toa",)), dict(pair=("toa", "soa")), dict(pair=("toa_projection", "mono")), dict(pair=("l714dmx", "mono")),
                  dict(pair=("scalable", "mono")), dict(sample_size=32), dict(layout=("ss", 3)), dict(layout=("binaural",)), dict(limiter=False),
                  dict(rate=44100), dict(out_rate=96000), dict(big_endian=True), dict(fs=1002)):
        assert U.facade_mix_frames(dict(base, **other)) is None, other
    assert U.facade_mix_frames(dict(base, pair=("toa", "foa")), "lfe") is None               # (a batch of its own for element 1)
    assert U.facade_mix_frames(dict(base, pair=("toa", "foa")), "default") is not None
