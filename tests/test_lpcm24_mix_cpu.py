"""No GPU: iamf_hip_batch_render_packets_mix is declared, exported and bound, and its ctypes mirror has the C struct's size and
offsets (a compiled probe says them); the launch entries of the two new units stay hidden; its family (LPCM24_MIX = 33, named in
a dict of its own beside A.ROUTE and A.ROUTE_BY_FAMILY_ONLY, which are pinned) lists exactly the 36 instances, which no numbered
table and no other family lists; every pinned count of the other listings is unchanged; the refusals that need no device answer
IAMF_HIP_ERR_BAD_ARG; and the cases of tests/test_gpu_zz_lpcm24_mix.py are the listing's rows."""
import ctypes as C
import os
import re
import subprocess

import iac_amd as A
import route_cases_lpcm_mix as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
FAM, FAMILY = "LPCM24_MIX", 33
ROUTE_KEYS = {"NONE", "GENERIC", "NOLIM", "FAST", "FAST_DOWN", "WIDE", "WIDE4", "WIDE4_DEMIX", "WIDE4_DOWN", "WIDE4_MIX", "WIDE4_LFE",
              "LPCM", "FANOUT", "FIR_SPLIT", "FIR_FUSED", "FANOUT_LPCM", "LPCM24", "LPCM_COUPLED", "RS_PLAIN", "RS_TILE", "RS_BLOCK",
              "RS_DIRECT", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED"}


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_packets_mix" in names and hasattr(A.lib(), "iamf_hip_batch_render_packets_mix")
    assert "iamf_hip_fast_lpcm24_mix_launch" not in names and "iamf_hip_fast_lpcm24_mix_coupled_launch" not in names   # hidden
    assert "iamf_hip_batch_render_lpcm_mix" in names and "iamf_hip_batch_render_packets" in names
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_packets_mix\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_packet_mix_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*iamf_hip_lpcm_input in\[2\];\s*iamf_hip_render_args args;\s*int32_t reserved\[4\];\s*\}\s*"
                     r"iamf_hip_packet_mix_call;", src)
    assert re.search(r"IAMF_HIP_ROUTE_LPCM24_MIX\s*=\s*%d\b" % FAMILY, src)
    assert A.ROUTE_FAMILY_MORE == {FAM: FAMILY} and A.hipabi._family_id(FAM) == FAMILY and A.hipabi._family_name(FAMILY) == FAM
    assert A.hipabi._family_id("LPCM24_COUPLED") == 31 and A.hipabi._family_id("LPCM_MIX") == 25 and A.hipabi._family_id(7) == 7
    assert A.hipabi._family_name(31) == "LPCM24_COUPLED" and A.hipabi._family_name(25) == "LPCM_MIX"
    assert callable(A.Batch.render_packets_mix)
    assert A.lib().iamf_hip_batch_render_packets_mix.argtypes[1]._type_ is A.PacketMixCall


def test_the_pinned_dicts_are_as_they_were():
    assert set(A.ROUTE) == ROUTE_KEYS and FAM not in A.ROUTE and FAMILY not in A.ROUTE.values()
    assert A.ROUTE_BY_FAMILY_ONLY == {"LPCM24_COUPLED": 31}
    assert len(A.hipabi.ROUTE_NAME) == len(A.ROUTE) + 1 and FAMILY not in A.hipabi.ROUTE_NAME


def test_the_mirror_has_the_c_structs_size_and_offsets(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "iamf_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(iamf_hip_packet_mix_call), offsetof(iamf_hip_packet_mix_call, in),\n'
                '                        offsetof(iamf_hip_packet_mix_call, args), offsetof(iamf_hip_packet_mix_call, reserved),\n'
                '                        sizeof(iamf_hip_lpcm_input), sizeof(iamf_hip_render_args), sizeof(iamf_hip_lpcm_mix_call)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    size, o_in, o_args, o_res, in_size, args_size, old_size = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    P = A.PacketMixCall
    assert (C.sizeof(P), P.in_.offset, P.args.offset, P.reserved.offset) == (size, o_in, o_args, o_res)
    assert C.sizeof(A.LpcmInput) == in_size and C.sizeof(A.RenderArgs) == args_size and C.sizeof(A.LpcmMixCall) == old_size
    assert o_in == 0 and o_args == 2 * in_size and o_res == 2 * in_size + args_size and size == old_size + 16


def test_the_family_has_36_rows_and_shares_none_with_a_table_or_a_family():
    rows = A.route_family_instances(FAM)
    want = {(FAM, 0, m, oc, k) for m in RM.LPCM_M + RM.COUPLED_M for oc in RM.MIX_OC for k in RM.MIX_K}
    assert len(rows) == len(set(rows)) == 36 and set(rows) == want
    assert A.route_family_instances(FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(FAMILY, None, 0) == 36
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == FAM], t
    for other in ("LPCM_COUPLED", "LPCM_MIX", "LPCM24_COUPLED", "FAST_INTERLEAVED", "FAST_RAGGED", "FAST", "LPCM", "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == FAM], other
    assert {r[1:] for r in A.route_family_instances("LPCM_MIX")} == {r[1:] for r in rows}     # the 16-bit mix's (variant, m, c, k), another family
    row = (A.RouteRow * 5)()
    assert A.lib().iamf_hip_route_family_instances(FAMILY, row, 5) == 36       # cap rows filled, the count returned
    assert all(r.family == FAMILY and r.variant == 0 and r.k in (1, 2) and r.launches == 0 for r in row)


def test_the_gpu_cases_are_the_listings_rows():
    import test_gpu_zz_lpcm24_mix as T
    assert sorted(T.inst(*i) for i in T.INSTANCES) == sorted(A.route_family_instances(FAM))
    for m, oc, k in T.INSTANCES:
        m2, form2 = T.second(m, k)
        assert (m2, form2) in ((1, "mono"), (4, "mono"), (2, "pair")) and (form2 == "pair") == (k == 2)


def test_the_tally_is_empty_without_a_device():
    assert A.route_family_tally(FAM) == {} and A.route_family_tally(FAM, reset=True) == {}
    assert A.lib().iamf_hip_route_family_tally(FAMILY, None, 0, 0) == 0


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_instances()) == len(set(A.route_instances()))
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    assert len(A.route_family_instances("LPCM_COUPLED")) == 20 and len(A.route_family_instances("LPCM_MIX")) == 36
    assert len(A.route_family_instances("FAST_INTERLEAVED")) == 4 and len(A.route_family_instances("FAST_RAGGED")) == 18
    assert len(A.route_family_instances("LPCM24_COUPLED")) == 20
    assert [r for t in range(3) for r in A.route_table_instances(t) if r[0] == FAM] == []
    for fam in (18, 19, 24, 26, 28, 30, 32, 34, 35):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def _call(reserved=None, d_in=None, d_in2=None):
    call = A.PacketMixCall()
    for i in (0, 1):
        call.in_[i].d_raw, call.in_[i].raw_stream_stride, call.in_[i].raw_frame_stride = 0x5000 + 0x10000 * i, 1 << 16, 1 << 14
    call.args.d_pcm, call.args.n_frames = 0x3000, 1
    call.args.d_in, call.args.d_in2 = d_in, d_in2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_and_reserved_words_are_refused_without_a_device():
    L = A.lib()
    assert L.iamf_hip_batch_render_packets_mix(None, C.byref(_call()), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_packets_mix(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
    assert L.iamf_hip_batch_render_packets_mix(None, None, 0, 1) == BAD_ARG
    for i in range(4):    # (nor here: the reserved words are looked at before the batch)
        assert L.iamf_hip_batch_render_packets_mix(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i
    # (nor here: d_in and d_in2 are the call's own words)
    assert L.iamf_hip_batch_render_packets_mix(0x4000, C.byref(_call(d_in=0x1000)), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_packets_mix(0x4000, C.byref(_call(d_in2=0x1000)), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_lpcm_mix(None, None, 0, 1) == BAD_ARG            # the old entry's own, as it was
