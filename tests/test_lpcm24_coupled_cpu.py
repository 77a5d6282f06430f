"""No GPU: iamf_hip_batch_render_packets is declared, exported and bound, and its ctypes mirror has the C struct's size and
offsets (a compiled probe says them); its family (LPCM24_COUPLED = 31, named beside A.ROUTE, whose keys are pinned) lists exactly
the 20 instances, which no numbered table and no other family lists; every pinned count of the other listings is unchanged; the
refusals that need no device answer IAMF_HIP_ERR_BAD_ARG; and the packet rows the GPU tests build (lpcm_util.rows with 24-bit
samples and the coupled widths) hold, read back by a numpy restatement of the unpacker, the ints they were built from — L in
front of R."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import iac_amd as A
import lpcm_util as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
FAM, FAMILY = "LPCM24_COUPLED", 31
COUPLED_M = [2, 6, 8, 10, 12]
ROUTE_KEYS = {"NONE", "GENERIC", "NOLIM", "FAST", "FAST_DOWN", "WIDE", "WIDE4", "WIDE4_DEMIX", "WIDE4_DOWN", "WIDE4_MIX", "WIDE4_LFE",
              "LPCM", "FANOUT", "FIR_SPLIT", "FIR_FUSED", "FANOUT_LPCM", "LPCM24", "LPCM_COUPLED", "RS_PLAIN", "RS_TILE", "RS_BLOCK",
              "RS_DIRECT", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED"}


def coupled(m):
    """(widths, perm) of lpcm_util.rows for a loudspeaker layout of m channels, as tests/test_gpu_lpcm_coupled.py has them"""
    if m <= 2:
        return [m], list(range(m))
    return [2] * ((m - 2) // 2) + [1, 1], [0, 1, m - 2, m - 1] + list(range(2, m - 2))


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_packets" in names and hasattr(A.lib(), "iamf_hip_batch_render_packets")
    assert "iamf_hip_fast_lpcm24_coupled_launch" not in names       # the launch entry stays hidden
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_packets\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_packet_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*iamf_hip_lpcm_input in;\s*iamf_hip_render_args args;\s*int32_t reserved\[4\];\s*\}\s*"
                     r"iamf_hip_packet_call;", src)
    assert re.search(r"IAMF_HIP_ROUTE_LPCM24_COUPLED\s*=\s*%d\b" % FAMILY, src)
    assert A.ROUTE_BY_FAMILY_ONLY == {FAM: FAMILY} and A.hipabi.ROUTE_NAME[FAMILY] == FAM
    assert A.hipabi.ROUTE_NAME[29] == "FAST_RAGGED" and A.hipabi.ROUTE_NAME[17] == "LPCM_COUPLED"      # the numbers in use keep their names
    assert callable(A.Batch.render_packets)
    assert A.lib().iamf_hip_batch_render_packets.argtypes[1]._type_ is A.PacketCall


def test_the_names_of_route_are_as_they_were():
    assert set(A.ROUTE) == ROUTE_KEYS and FAM not in A.ROUTE and FAMILY not in A.ROUTE.values()
    assert len(A.hipabi.ROUTE_NAME) == len(A.ROUTE) + 1


def test_the_mirror_has_the_c_structs_size_and_offsets(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "iamf_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(iamf_hip_packet_call), offsetof(iamf_hip_packet_call, in),\n'
                '                        offsetof(iamf_hip_packet_call, args), offsetof(iamf_hip_packet_call, reserved),\n'
                '                        sizeof(iamf_hip_lpcm_input), sizeof(iamf_hip_render_args)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    size, o_in, o_args, o_res, in_size, args_size = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    P = A.PacketCall
    assert (C.sizeof(P), P.in_.offset, P.args.offset, P.reserved.offset) == (size, o_in, o_args, o_res)
    assert C.sizeof(A.LpcmInput) == in_size and C.sizeof(A.RenderArgs) == args_size
    assert o_in == 0 and o_args == in_size and o_res == in_size + args_size and size == in_size + args_size + 16


def test_the_family_has_20_rows_and_shares_none_with_a_table_or_a_family():
    rows = A.route_family_instances(FAM)
    want = {(FAM, early, m, oc, 0) for m in COUPLED_M for oc in (1, 2) for early in (0, 1)}
    assert len(rows) == len(set(rows)) == 20 and set(rows) == want
    assert A.route_family_instances(FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(FAMILY, None, 0) == 20
    keys = {r[1:] for r in rows}
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == FAM], t
    for other in ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED", "FAST", "LPCM", "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == FAM], other
    assert {r[1:] for r in A.route_family_instances("LPCM_COUPLED")} == keys     # the 16-bit form's (variant, m, c, k), another family
    row = (A.RouteRow * 5)()
    assert A.lib().iamf_hip_route_family_instances(FAMILY, row, 5) == 20       # cap rows filled, the count returned
    assert all(r.family == FAMILY and r.k == 0 and r.launches == 0 for r in row)


def test_the_tally_is_empty_without_a_device():
    assert A.route_family_tally(FAM) == {} and A.route_family_tally(FAM, reset=True) == {}
    assert A.lib().iamf_hip_route_family_tally(FAMILY, None, 0, 0) == 0


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    assert len(A.route_family_instances("LPCM_COUPLED")) == 20 and len(A.route_family_instances("LPCM_MIX")) == 36
    assert len(A.route_family_instances("FAST_INTERLEAVED")) == 4 and len(A.route_family_instances("FAST_RAGGED")) == 18
    assert [r for t in range(3) for r in A.route_table_instances(t) if r[0] == FAM] == []
    for fam in (18, 19, 24, 26, 28, 30, 32):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def _call(reserved=None, d_in=None, d_in2=None):
    call = A.PacketCall()
    call.in_.d_raw, call.in_.raw_stream_stride, call.in_.raw_frame_stride = 0x5000, 1 << 16, 1 << 14
    call.args.d_pcm, call.args.n_frames = 0x3000, 1
    call.args.d_in, call.args.d_in2 = d_in, d_in2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_and_reserved_words_are_refused_without_a_device():
    L = A.lib()
    assert L.iamf_hip_batch_render_packets(None, C.byref(_call()), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_packets(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
    assert L.iamf_hip_batch_render_packets(None, None, 0, 1) == BAD_ARG
    for i in range(4):    # (nor here: the reserved words are looked at before the batch)
        assert L.iamf_hip_batch_render_packets(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i
    # (nor here: d_in and d_in2 are the call's own words)
    assert L.iamf_hip_batch_render_packets(0x4000, C.byref(_call(d_in=0x1000)), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_packets(0x4000, C.byref(_call(d_in2=0x1000)), 0, 1) == BAD_ARG


def _unpack(raw, L, fs):
    """iamf_hip_lpcm_unpack restated: sample i of channel c = the sample_bytes little-endian bytes at src_offset[c] +
    src_step[c] * i of the row, sign-extended -> [S][F][ch][fs] ints"""
    S, F, _ = raw.shape
    out = np.zeros((S, F, L.channels, fs), dtype=np.int64)
    i = np.arange(fs)
    for c in range(L.channels):
        at = L.src_offset[c] + L.src_step[c] * i
        u = sum(raw[:, :, at + k].astype(np.int64) << (8 * k) for k in range(L.sample_bytes))
        bits = 8 * L.sample_bytes
        out[:, :, c, :] = (u ^ (1 << (bits - 1))) - (1 << (bits - 1))
    return out


def test_the_packet_rows_hold_the_ints_with_left_in_front_of_right():
    fs = 64
    for m in COUPLED_M:
        widths, perm = coupled(m)
        ints = LP.ints(np.random.default_rng(3100 + m), 2, 2, m, fs, 3)
        ints[0, 0, :, 0] = -(1 << 23)
        ints[0, 0, :, 1] = (1 << 23) - 1
        raw, L, row = LP.rows(ints, 3, True, widths, perm, head=4, pad=4, frame_size=fs)
        assert L.sample_bytes == 3 and L.little_endian == 1 and row % 16 == 0 and raw.shape == (2, 2, row)
        got = _unpack(raw, L, fs)
        assert np.array_equal(got, ints[:, :, perm, :]), m       # playback channel p holds decoded channel perm[p]
        for c in range(m):
            paired = m == 2 or c < 2 or c >= 4
            assert L.src_step[c] == (6 if paired else 3), (m, c)
            if paired and c % 2 == 0:      # L in front: the partner (R) 3 bytes behind, both decoded channels of ONE sub-stream
                assert L.src_offset[c + 1] == L.src_offset[c] + 3 and perm[c + 1] == perm[c] + 1, (m, c)
                assert L.src_offset[c] % 4 == 0, (m, c)
                assert not np.array_equal(got[:, :, c], got[:, :, c + 1])
            if not paired:
                assert L.src_offset[c] % 4 == 0, (m, c)
