"""No GPU: iamf_hip_batch_render_packets_ragged is declared, exported and bound, and takes the call struct of
iamf_hip_batch_render_packets; its family (PACKETS_RAGGED = 37) lists exactly the 36 instances — the four single-element packet
forms x their channel counts x one or two outputs — which no numbered table and no other family lists; the tables and the other
families are as they were, ids 36 and 38 empty; tests/route_host/route_host_packets_ragged_check.cpp, compiled with the host
compiler, pins every clause of packets_ragged_shape_ok (render_route.hpp); every instance has a GPU case; the refusals that need
no device answer IAMF_HIP_ERR_BAD_ARG; the programme of the GPU tests lies on the packets' grid and packets_of() places it as
the layout says; and every programme the limiter-on GPU tests render (packets_ragged_util.proofs) is proven, from the oracle's
limiter trace, to keep the limiter attenuating across the end of every call and into the next one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import iac_amd as A
import packets_ragged_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
BAD_ARG = -1
FAMILY = 37


def _header():
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        return f.read()


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_packets_ragged" in names and hasattr(A.lib(), "iamf_hip_batch_render_packets_ragged")
    for hidden in ("iamf_hip_fast_packets_ragged_launch", "iamf_hip_fast_packets_ragged_coupled_launch", "iamf_hip_fast_packets_ragged24_launch",
                   "iamf_hip_fast_packets_ragged24_coupled_launch"):
        assert hidden not in names       # the launch entries stay hidden
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_packets_ragged\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_packet_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"IAMF_HIP_ROUTE_PACKETS_RAGGED\s*=\s*%d\b" % FAMILY, src)
    assert A.ROUTE_FAMILY_LATER == {PU.FAM: FAMILY} and A.hipabi._family_id(PU.FAM) == FAMILY and A.hipabi._family_name(FAMILY) == PU.FAM
    assert PU.FAM not in A.ROUTE and PU.FAM not in A.ROUTE_BY_FAMILY_ONLY and PU.FAM not in A.ROUTE_FAMILY_MORE
    assert A.hipabi._family_name(33) == "LPCM24_MIX" and A.hipabi.ROUTE_NAME[31] == "LPCM24_COUPLED" and A.hipabi.ROUTE_NAME[29] == "FAST_RAGGED"
    assert callable(A.Batch.render_packets_ragged)
    assert A.lib().iamf_hip_batch_render_packets_ragged.argtypes == A.lib().iamf_hip_batch_render_packets.argtypes
    assert A.lib().iamf_hip_batch_render_packets_ragged.argtypes[1]._type_ is A.PacketCall


def test_the_mirror_has_the_c_structs_size_and_offsets(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "iamf_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(iamf_hip_packet_call), offsetof(iamf_hip_packet_call, in),\n'
                '                        offsetof(iamf_hip_packet_call, args), offsetof(iamf_hip_packet_call, reserved),\n'
                '                        sizeof(iamf_hip_lpcm_input), offsetof(iamf_hip_lpcm_input, first_sample)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    size, o_in, o_args, o_res, in_size, o_first = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert (C.sizeof(A.PacketCall), A.PacketCall.in_.offset, A.PacketCall.args.offset, A.PacketCall.reserved.offset) == (size, o_in, o_args, o_res)
    assert C.sizeof(A.LpcmInput) == in_size and A.LpcmInput.first_sample.offset == o_first


def test_the_family_has_36_rows_and_shares_none_with_a_table_or_a_family():
    rows = A.route_family_instances(PU.FAM)
    assert len(rows) == len(set(rows)) == 36 and set(rows) == {PU.inst(f, m, oc) for f, m, oc in PU.INSTANCES}
    assert A.route_family_instances(FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(FAMILY, None, 0) == 36
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == PU.FAM], t
    for other in ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST_RAGGED", "LPCM24_COUPLED", "LPCM24_MIX", "FAST", "LPCM", "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == PU.FAM], other
    row = (A.RouteRow * 5)()
    assert A.lib().iamf_hip_route_family_instances(FAMILY, row, 5) == 36       # cap rows filled, the count returned
    assert all(r.family == FAMILY and r.variant == 0 and r.k in (2, 3) and r.launches == 0 for r in row)
    assert A.route_family_tally(PU.FAM) == {} and A.route_family_tally(PU.FAM, reset=True) == {}


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    counts = {"LPCM_COUPLED": 20, "LPCM_MIX": 36, "FAST_INTERLEAVED": 4, "FAST_RAGGED": 18, "LPCM24_COUPLED": 20, "LPCM24_MIX": 36, "LPCM": 16,
              "LPCM24": 16}
    for fam, n in counts.items():
        assert len(A.route_family_instances(fam)) == n, fam
    for fam in (18, 19, 24, 26, 28, 30, 32, 34, 35, 36, 38):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def test_the_routing_rule_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_packets_ragged_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_packets_ragged_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 250 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out


def test_every_instance_has_a_gpu_case():
    import test_gpu_zz_packets_ragged as TG
    cases = [PU.inst(f, m, oc) for f, m, oc in TG.EVERY_INSTANCE]       # what test_every_instance walks
    assert len(cases) == len(set(cases)) and set(cases) == set(A.route_family_instances(PU.FAM))
    assert [PU.inst(f, m, oc) for f, m, oc in PU.INSTANCES] == A.route_family_instances(PU.FAM)     # the listing's order


def _call(reserved=None, d_in=None, d_in2=None):
    call = A.PacketCall()
    call.in_.d_raw, call.in_.raw_stream_stride, call.in_.raw_frame_stride = 0x1000, 4096, 4096
    call.args.d_pcm, call.args.n_frames = 0x3000, 1
    call.args.d_in, call.args.d_in2 = d_in, d_in2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_reserved_words_and_f32_inputs_are_refused_without_a_device():
    """what iamf_hip_batch_render_packets refuses before it looks at the batch, with its code"""
    L = A.lib()
    for entry in (L.iamf_hip_batch_render_packets_ragged, L.iamf_hip_batch_render_packets):
        assert entry(None, C.byref(_call()), 0, 1) == BAD_ARG
        assert entry(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
        assert entry(None, None, 0, 1) == BAD_ARG
        for i in range(4):    # (nor here: the reserved words are looked at before the batch)
            assert entry(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i
        assert entry(0x4000, C.byref(_call(d_in=0x2000)), 0, 1) == BAD_ARG
        assert entry(0x4000, C.byref(_call(d_in2=0x2000)), 0, 1) == BAD_ARG


# ---- the programme and its packets ----

@pytest.mark.parametrize("form", sorted(PU.FORMS))
def test_the_programme_lies_on_the_packets_grid_and_is_placed_as_the_layout_says(form):
    """ints / 2^15 (2^23) is exact in f32, and unpacking packets_of()'s rows by the layout gives the call's samples back at
    first_sample on, with the fill in every other byte"""
    import gpu_util as G
    bps, cpl = PU.FORMS[form]
    m, fs, first, n = (6 if cpl else 4), 100, 4, 90
    ints = PU.hot_ints(form, m, 300)
    x = PU.as_f32(ints, bps)
    assert np.array_equal((x.astype(np.float64) * (1 << (8 * bps - 1))).astype(np.int64), ints) and np.abs(ints).max() > (1 << (8 * bps - 3))
    raw, L, row = PU.packets_of(form, ints[:, :, 10:10 + n], 1, fs, first, fill=0xA5, head=4, pad=4)
    assert raw.shape == (PU.S, 1, row) and L.sample_bytes == bps and L.channels == m and L.frame_size == fs
    used = np.zeros(row, dtype=bool)
    for c in range(m):
        at = L.src_offset[c] + L.src_step[c] * (first + np.arange(n))
        v = sum(raw[:, 0, at + k].astype(np.int64) << (8 * k) for k in range(bps))
        v = (v ^ (1 << (8 * bps - 1))) - (1 << (8 * bps - 1))
        assert np.array_equal(v, ints[:, c, 10:10 + n]), (form, c)
        for k in range(bps):
            used[at + k] = True
    assert bool((raw[:, 0, ~used] == 0xA5).all()) and used.sum() == m * n * bps
    assert (used & ~G.packet_run_mask(L, row)).sum() == 0      # (the runs hold frame_size samples: the call's are among them)


def test_the_default_routes_of_the_cases():
    """what the GPU tests assert per call is what the length and position rules give"""
    for name, (form, m, oc, fs, calls) in PU.CASES.items():
        got = PU.default_routes(fs, calls)
        assert got == [PU.PRAG] * len(calls), (name, got)
        assert (form, m, oc) in PU.INSTANCES and fs % 4 == 0
        for nf, ns in calls:
            assert nf >= 1 and 0 <= ns <= fs and (ns == 0 or nf == 1)
    assert PU.default_routes(1000, [(1, 0), (8, 0), (1, 0)]) == [PU.PRAG, PU.WHOLE_ROW, PU.PRAG]
    assert PU.default_routes(1000, [(1, 100), (1, 0)]) == [PU.PRAG, "GENERIC"]


PROOFS = PU.proofs()


def test_the_proofs_cover_every_case_and_every_instance():
    labels = [p[0] for p in PROOFS]
    assert len(labels) == len(set(labels)) and set(PU.CASES) <= set(labels)
    assert {(p[1], p[2], p[3]) for p in PROOFS if p[0].startswith("instance ")} == set(PU.INSTANCES)


@pytest.mark.parametrize("proof", PROOFS, ids=[p[0] for p in PROOFS])
def test_the_limiter_attenuates_across_every_call_boundary(proof):
    """for every programme a limiter-on GPU test renders (packets_ragged_util.proofs): the first call triggers, and at every
    call boundary the limiter is in attack or release with a gain below 1"""
    import oracle_lib as O
    name, form, m, oc, fs, calls, streams = proof
    sz = PU.sizes(fs, calls)
    ints = PU.hot_ints(form, m, sum(sz), streams=streams)
    _, omx = PU.IU.dense_matrices(m, oc)
    for s in range(streams):
        _, z = PU.want(omx, oc, ints[s], PU.FORMS[form][0], sz, 16, PU.EG[s % len(PU.EG)], PU.OG[s % len(PU.OG)])
        y, t = O.limiter_trace(z, sz)
        trig = np.flatnonzero(t & O.LIM_TRIGGER)
        assert trig.size and trig[0] < sz[0], (name, s, "the first call triggers")
        for e in np.cumsum(sz)[:-1]:
            e = int(e)
            what = (name, s, e)
            assert (t[e - 1] & 3) != O.LIM_IDLE and (t[e] & 3) != O.LIM_IDLE, what
            for k in (e - 1, e):
                j = k - 240
                if j < 0:
                    continue
                c = int(np.argmax(np.abs(z[:, j])))
                assert z[c, j] != 0.0 and abs(y[c, j]) < abs(z[c, j]), what


# ---- the façade and group cases ----

def test_at_least_one_stored_fuzz_stream_reaches_the_family_through_the_facade():
    """the streams tests/test_gpu_zz_packets_ragged_facade.py decodes are selected by configuration from the stored fuzz sets,
    whose PCM hashes come from the real reference: at least one is selected, in 16 and in 24 bits, into stereo and into mono.
    (The stored sets hold no stream with frames of 1000 or 2000 that the façade's packet path takes — those are big-endian,
    resampled, two-element or into wide layouts — so the selected streams reach the family through their trimmed frames.)"""
    import json
    import e2e_fuzz as F
    sel = PU.facade_streams()
    assert len(sel) >= 2, sel
    cases = [F.case(seed, v) for v, seed, _ in sel]
    assert {c["sample_size"] for c in cases} >= {16, 24} and {c["layout"] for c in cases} == set(PU.FACADE_LAYOUTS), cases
    gold = {"default": "fuzz.json", "wide": "fuzz_wide.json"}
    for v, seed, frames in sel:
        want = json.load(open(os.path.join(ROOT, "tests", "golden", gold[v])))[str(seed)]
        assert "sha256" in want and frames, (v, seed)      # (the reference decoded it: there is a hash to hold the PCM against)
