"""No GPU: iamf_hip_batch_render_packets_mix_nolim is declared with the prototype of include/iamf_hip.h, exported and bound, and takes
the call struct of iamf_hip_batch_render_packets_mix; its family (NOLIM_PACKETS_MIX = 47) lists exactly the 36 instances — (the
four single-element packet forms x their channel counts) x the second element's two forms — which no numbered table and no other
family lists, ids 44, 45 and 46 empty; the other families' counts are as they were; every instance has a GPU case; the refusals
that need no device answer IAMF_HIP_ERR_BAD_ARG through both entries; and the stored fuzz streams the façade tests decode are
selected by configuration and hold the streams named below.  (The routing rule is pinned by
tests/test_route_host_nolim_packets_mix.py.)"""
import ctypes as C
import json
import os
import re
import subprocess

import iac_amd as A
import nolim_packets_mix_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_packets_mix_nolim" in names and hasattr(A.lib(), "iamf_hip_batch_render_packets_mix_nolim")
    for hidden in ("iamf_hip_nolim_packets_mix_launch", "iamf_hip_nolim_packets24_mix_launch", "iamf_hip_nolim_packets_launch",
                   "iamf_hip_nolim_packets24_launch"):
        assert hidden not in names       # the launch entries stay hidden
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_packets_mix_nolim\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_packet_mix_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX\s*=\s*%d\b" % U.FAMILY, src)
    assert A.hipabi._family_id(U.FAM) == U.FAMILY and A.hipabi._family_name(U.FAMILY) == U.FAM
    assert A.ROUTE_FAMILY_OPEN[U.FAM] == U.FAMILY and A.ROUTE_FAMILY_OPEN["NOLIM_PACKETS"] == 43
    for pinned in (A.ROUTE, A.ROUTE_BY_FAMILY_ONLY, A.ROUTE_FAMILY_MORE, A.ROUTE_FAMILY_LATER, A.ROUTE_FAMILY_NEWER):
        assert U.FAM not in pinned
    assert callable(A.Batch.render_packets_mix_nolim)
    fn = A.lib().iamf_hip_batch_render_packets_mix_nolim
    assert fn.argtypes == A.lib().iamf_hip_batch_render_packets_mix_ragged.argtypes == [C.c_void_p, C.POINTER(A.PacketMixCall), C.c_int32, C.c_int32]
    assert fn.argtypes[1]._type_ is A.PacketMixCall


def test_the_family_lists_exactly_the_36_rows():
    rows = A.route_family_instances(U.FAM)
    assert len(rows) == len(set(rows)) == 36 and rows == [U.inst(b, m, k) for b, m, k in U.INSTANCES]
    assert A.route_family_instances(U.FAMILY) == rows and A.lib().iamf_hip_route_family_instances(U.FAMILY, None, 0) == 36
    assert {(r[1], r[2], r[3], r[4]) for r in rows} == {(b, m, 0, k) for b in (2, 3) for m in (1, 4, 9, 16, 2, 6, 8, 10, 12) for k in (1, 2)}
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == U.FAM], t
    for other in ("NOLIM", "NOLIM_PACKETS", "PACKETS_RAGGED", "PACKETS_MIX_RAGGED", "LPCM_MIX", "LPCM24_MIX", "LPCM_COUPLED", "LPCM24_COUPLED", "LPCM",
                  "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == U.FAM], other
    for fam in (44, 45, 46, 48):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam
    assert A.route_family_tally(U.FAM) == {} and A.route_family_tally(U.FAM, reset=True) == {}


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3 and A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    counts = {"NOLIM": 12, "NOLIM_PACKETS": 18, "PACKETS_RAGGED": 36, "PACKETS_MIX_RAGGED": 72, "LPCM_COUPLED": 20, "LPCM24_COUPLED": 20,
              "FAST_INTERLEAVED": 4}
    for fam, n in counts.items():
        assert len(A.route_family_instances(fam)) == n, fam


def test_every_instance_has_a_gpu_case():
    import test_gpu_zz_nolim_packets_mix as TG
    assert [U.inst(b, m, k) for b, m, k in TG.EVERY_INSTANCE] == A.route_family_instances(U.FAM)


def _call(reserved=None, d_in=None, d_in2=None):
    call = A.PacketMixCall()
    for e in range(2):
        call.in_[e].d_raw, call.in_[e].raw_stream_stride, call.in_[e].raw_frame_stride = 0x1000 * (e + 1), 4096, 4096
    call.args.d_pcm, call.args.n_frames = 0x3000, 1
    call.args.d_in, call.args.d_in2 = d_in, d_in2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_reserved_words_and_f32_inputs_are_refused_without_a_device():
    """what iamf_hip_batch_render_packets_mix_ragged refuses before it looks at the batch, with its code"""
    L = A.lib()
    for entry in (L.iamf_hip_batch_render_packets_mix_nolim, L.iamf_hip_batch_render_packets_mix_ragged):
        assert entry(None, C.byref(_call()), 0, 1) == BAD_ARG
        assert entry(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
        for i in range(4):
            assert entry(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i
        assert entry(0x4000, C.byref(_call(d_in=0x2000)), 0, 1) == BAD_ARG
        assert entry(0x4000, C.byref(_call(d_in2=0x2000)), 0, 1) == BAD_ARG


def test_the_stored_fuzz_streams_of_the_facade_tests():
    """selected by configuration from the stored fuzz sets, whose PCM hashes come from the real reference: default 129 (7.1.2 +
    zeroth order, 16 bit, limiter off, frames of 1024, 8 channels of s16), default 163 (7.1.2 + first order, 24 bit, 32 -> 48 kHz,
    gain ramps, the last frame trimmed to 895 samples: the twin's; 11 channels) and default 209 (5.1.4 + zeroth order, 16 -> 48 kHz
    with the limiter off, the last frame trimmed to 737 samples: the twin's); and, of the params set — whose stream N is the
    default set's stream N with mix-gain parameter timelines on it (e2e_fuzz.build: case_params) — params 129 and params 163, the
    same two pairs with animated element and output gains.  (case(seed, "params") describes no stream of that set: the five
    configurations it yields — 12, 115, 135, 147, 194 — are not what fuzz_params.json holds hashes of.)"""
    import e2e_fuzz as F
    import e2e_model as M
    sel = U.facade_streams()
    assert {(v, s) for v, s, _ in sel} >= {("default", 129), ("default", 163), ("default", 209), ("params", 129), ("params", 163)}
    by = {(v, s): (U.facade_case(s, v), fr) for v, s, fr in sel}
    for v in ("default", "params"):
        c, fr = by[(v, 129)]
        assert c["pair"] == ("l712", "zoa") and c["sample_size"] == 16 and c["limiter"] is False and c["fs"] == 1024 and c["bit_depth"] == 16
        assert M.SS_CH[c["layout"][1]] == 8 and fr == list(range(c["frames"])) and ("gain_sched" in c) == (v == "params")
        c, fr = by[(v, 163)]
        assert c["pair"] == ("l712", "foa") and c["sample_size"] == 24 and (c["rate"], c["out_rate"]) == (32000, 48000) and c["trims"] == {7: (0, 1153)}
        assert M.SS_CH[c["layout"][1]] == 11 and fr == list(range(c["frames"] - 1)) and ("gain_sched" in c) == (v == "params")
    assert by[("default", 163)][0]["pair_ramps"]
    c, fr = by[("default", 209)]
    assert c["pair"] == ("l514", "zoa") and (c["rate"], c["out_rate"]) == (16000, 48000) and c["limiter"] is False
    assert c["trims"] == {6: (0, 287)} and c["fs"] - 287 == 737 and fr == list(range(6))
    for v, seed, _ in sel:
        want = json.load(open(os.path.join(ROOT, "tests", "golden", U.FACADE_GOLD[v])))[str(seed)]
        assert "sha256" in want, (v, seed)      # (the reference decoded it: there is a hash to hold the PCM against)
        assert A.route_family_instances(U.FAM).count(U.facade_instance(U.facade_case(seed, v))) == 1, (v, seed)
        stream_case = F.build(seed, v)[1]
        assert stream_case["pair"] == U.facade_case(seed, v)["pair"], (v, seed)      # (the description is the built stream's)
