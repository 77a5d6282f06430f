"""No GPU: iamf_hip_batch_render_packets_nolim is declared with the prototype of include/iamf_hip.h, exported and bound, and takes
the call struct of iamf_hip_batch_render_packets; its family (NOLIM_PACKETS = 43) lists exactly the 18 instances — the four
single-element packet forms x their channel counts — which no numbered table and no other family lists, ids 40, 41, 42 and 44 empty; every
instance has a GPU case; the refusals that need no device answer IAMF_HIP_ERR_BAD_ARG; and the stored fuzz streams the façade
tests decode are selected by configuration and hold the streams named below.  (The routing rule is pinned by
tests/test_route_host_nolim_packets.py.)"""
import ctypes as C
import json
import os
import re
import subprocess

import iac_amd as A
import nolim_packets_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_packets_nolim" in names and hasattr(A.lib(), "iamf_hip_batch_render_packets_nolim")
    for hidden in ("iamf_hip_nolim_packets_launch", "iamf_hip_nolim_packets24_launch"):
        assert hidden not in names       # the launch entries stay hidden
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_packets_nolim\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_packet_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"IAMF_HIP_ROUTE_NOLIM_PACKETS\s*=\s*%d\b" % U.FAMILY, src)
    assert A.hipabi._family_id(U.FAM) == U.FAMILY and A.hipabi._family_name(U.FAMILY) == U.FAM
    for pinned in (A.ROUTE, A.ROUTE_BY_FAMILY_ONLY, A.ROUTE_FAMILY_MORE, A.ROUTE_FAMILY_LATER, A.ROUTE_FAMILY_NEWER):
        assert U.FAM not in pinned
    assert callable(A.Batch.render_packets_nolim)
    fn = A.lib().iamf_hip_batch_render_packets_nolim
    assert fn.argtypes == A.lib().iamf_hip_batch_render_packets_ragged.argtypes == [C.c_void_p, C.POINTER(A.PacketCall), C.c_int32, C.c_int32]
    assert fn.argtypes[1]._type_ is A.PacketCall


def test_the_family_lists_exactly_the_18_rows():
    rows = A.route_family_instances(U.FAM)
    assert len(rows) == len(set(rows)) == 18 and rows == [U.inst(f, m) for f, m in U.INSTANCES]
    assert A.route_family_instances(U.FAMILY) == rows and A.lib().iamf_hip_route_family_instances(U.FAMILY, None, 0) == 18
    assert {(r[2], r[4]) for r in rows} == {(m, k) for k in (2, 3) for m in (1, 4, 9, 16, 2, 6, 8, 10, 12)}
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == U.FAM], t
    for other in ("NOLIM", "PACKETS_RAGGED", "PACKETS_MIX_RAGGED", "LPCM_COUPLED", "LPCM24_COUPLED", "LPCM", "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == U.FAM], other
    for fam in (40, 41, 42, 44):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam
    assert A.route_family_tally(U.FAM) == {} and A.route_family_tally(U.FAM, reset=True) == {}


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3 and A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    counts = {"NOLIM": 12, "PACKETS_RAGGED": 36, "PACKETS_MIX_RAGGED": 72, "LPCM_COUPLED": 20, "LPCM24_COUPLED": 20, "FAST_INTERLEAVED": 4}
    for fam, n in counts.items():
        assert len(A.route_family_instances(fam)) == n, fam


def test_every_instance_has_a_gpu_case():
    import test_gpu_zz_nolim_packets as TG
    assert [U.inst(f, m) for f, m in TG.EVERY_INSTANCE] == A.route_family_instances(U.FAM)


def _call(reserved=None, d_in=None, d_in2=None):
    call = A.PacketCall()
    call.in_.d_raw, call.in_.raw_stream_stride, call.in_.raw_frame_stride = 0x1000, 4096, 4096
    call.args.d_pcm, call.args.n_frames = 0x3000, 1
    call.args.d_in, call.args.d_in2 = d_in, d_in2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_reserved_words_and_f32_inputs_are_refused_without_a_device():
    """what iamf_hip_batch_render_packets_ragged refuses before it looks at the batch, with its code"""
    L = A.lib()
    for entry in (L.iamf_hip_batch_render_packets_nolim, L.iamf_hip_batch_render_packets_ragged):
        assert entry(None, C.byref(_call()), 0, 1) == BAD_ARG
        assert entry(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
        for i in range(4):
            assert entry(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i
        assert entry(0x4000, C.byref(_call(d_in=0x2000)), 0, 1) == BAD_ARG
        assert entry(0x4000, C.byref(_call(d_in2=0x2000)), 0, 1) == BAD_ARG


def test_the_stored_fuzz_streams_of_the_facade_tests():
    """selected by configuration from the stored fuzz sets, whose PCM hashes come from the real reference: the resampling ones
    hold default 71 (5.1 24-bit coupled, 48 -> 44.1 kHz, mono out, trimmed), default 205 (3rd order 16 bit, 44.1 -> 48 kHz, mono
    out) and wide 105 (7.1.4 16-bit coupled, 96 -> 44.1 kHz, stereo out, frames of 1000); the limiter-off ones default 1 and
    default 224 (7.1 and 1st order, 16 bit, into stereo)"""
    import e2e_fuzz as F
    sel = U.facade_streams()
    assert sel and {(v, s) for v, s, _ in sel} >= {("default", 71), ("default", 205), ("wide", 105)}
    assert {(v, s) for v, s, _ in U.facade_streams(limiter_off=True)} >= {("default", 1), ("default", 224)}
    by = {(v, s): F.case(s, v) for v, s, _ in sel}
    c = by[("default", 71)]
    assert c["pair"] == ("l51",) and c["sample_size"] == 24 and (c["rate"], c["out_rate"]) == (48000, 44100) and c["layout"] == ("ss", 12) and c["trims"]
    c = by[("default", 205)]
    assert c["pair"] == ("toa",) and c["sample_size"] == 16 and (c["rate"], c["out_rate"]) == (44100, 48000) and c["layout"] == ("ss", 12)
    c = by[("wide", 105)]
    assert c["pair"] == ("l714",) and c["sample_size"] == 16 and (c["rate"], c["out_rate"]) == (96000, 44100) and c["layout"] == ("ss", 0) and c["fs"] == 1000
    for key, kind in ((("default", 1), "l71"), (("default", 224), "foa")):
        c = by[key]
        assert c["pair"] == (kind,) and c["sample_size"] == 16 and c["layout"] == ("ss", 0) and c["limiter"] is False
    gold = {"default": "fuzz.json", "wide": "fuzz_wide.json"}
    for v, seed, _ in sel:
        want = json.load(open(os.path.join(ROOT, "tests", "golden", gold[v])))[str(seed)]
        assert "sha256" in want, (v, seed)      # (the reference decoded it: there is a hash to hold the PCM against)
