"""No GPU: iamf_hip_batch_render_ragged is declared, exported and bound, and its ctypes mirror has the C struct's size and
offsets (a compiled probe says them); its family (FAST_RAGGED = 29) lists exactly the 18 instances, which no numbered table
and no other family lists; the tables are as they were; every instance has a GPU case; the refusals that need no device
answer IAMF_HIP_ERR_BAD_ARG; and every programme the limiter-on GPU tests render (ragged_util.proofs: the cases, every instance,
the sequences, the lifecycle, the range and the fall-backs) is proven, from the oracle's limiter trace, to keep the limiter
attenuating across the end of every call and into the next one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import iac_amd as A
import ragged_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
FAMILY = 29


def _header():
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        return f.read()


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_ragged" in names and hasattr(A.lib(), "iamf_hip_batch_render_ragged")
    assert "iamf_hip_fast_ragged_launch" not in names       # the launch entry stays hidden
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_ragged\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_ragged_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*iamf_hip_render_args args;\s*int32_t reserved\[4\];\s*\}\s*iamf_hip_ragged_call;", src)
    assert re.search(r"IAMF_HIP_ROUTE_FAST_RAGGED\s*=\s*%d\b" % FAMILY, src)
    assert A.ROUTE["FAST_RAGGED"] == FAMILY and A.hipabi.ROUTE_NAME[FAMILY] == "FAST_RAGGED"
    assert A.hipabi.ROUTE_NAME[27] == "FAST_INTERLEAVED" and A.hipabi.ROUTE_NAME[25] == "LPCM_MIX"      # the numbers in use keep their names
    assert callable(A.Batch.render_ragged)
    assert A.lib().iamf_hip_batch_render_ragged.argtypes[1]._type_ is A.RaggedCall


def test_the_mirror_has_the_c_structs_size_and_offsets(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "iamf_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(iamf_hip_ragged_call), offsetof(iamf_hip_ragged_call, args),\n'
                '                        offsetof(iamf_hip_ragged_call, reserved), sizeof(iamf_hip_render_args)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    size, o_args, o_res, args_size = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert (C.sizeof(A.RaggedCall), A.RaggedCall.args.offset, A.RaggedCall.reserved.offset) == (size, o_args, o_res)
    assert C.sizeof(A.RenderArgs) == args_size and o_args == 0 and o_res == args_size and size == args_size + 16


def test_the_family_has_18_rows_and_shares_none_with_a_table_or_a_family():
    rows = A.route_family_instances("FAST_RAGGED")
    assert len(rows) == len(set(rows)) == 18 and set(rows) == {RU.inst(m, oc) for m in (1, 2, 4, 6, 8, 9, 10, 12, 16) for oc in (1, 2)}
    assert A.route_family_instances(FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(FAMILY, None, 0) == 18
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == "FAST_RAGGED"], t
    for other in ("LPCM_COUPLED", "LPCM_MIX", "FAST_INTERLEAVED", "FAST", "LPCM", "LPCM24", "GENERIC"):
        theirs = A.route_family_instances(other)
        assert not set(rows) & set(theirs) and not [r for r in theirs if r[0] == "FAST_RAGGED"], other
    row = (A.RouteRow * 5)()
    assert A.lib().iamf_hip_route_family_instances(FAMILY, row, 5) == 18       # cap rows filled, the count returned
    assert all(r.family == FAMILY and r.variant == 0 and r.k == 0 and r.launches == 0 for r in row)
    assert A.route_family_tally("FAST_RAGGED") == {} and A.route_family_tally("FAST_RAGGED", reset=True) == {}


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    assert len(A.route_family_instances("LPCM_COUPLED")) == 20 and len(A.route_family_instances("LPCM_MIX")) == 36
    assert len(A.route_family_instances("FAST_INTERLEAVED")) == 4
    for fam in (18, 19, 24, 26, 28, 30):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def test_every_instance_has_a_gpu_case():
    import test_gpu_ragged as TG
    cases = [RU.inst(m, oc) for m, oc in TG.EVERY_INSTANCE]       # what test_every_instance walks
    assert len(cases) == len(set(cases)) and set(cases) == set(A.route_family_instances("FAST_RAGGED"))
    assert RU.INSTANCES == [(r[2], r[3]) for r in A.route_family_instances("FAST_RAGGED")]


def _call(reserved=None, d_in=0x1000, d_pcm=0x3000, n_frames=1):
    call = A.RaggedCall()
    call.args.d_in, call.args.d_pcm, call.args.n_frames, call.args.in_frame_stride = d_in, d_pcm, n_frames, 2000
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_and_reserved_words_are_refused_without_a_device():
    L = A.lib()
    assert L.iamf_hip_batch_render_ragged(None, C.byref(_call()), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_ragged(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
    assert L.iamf_hip_batch_render_ragged(None, None, 0, 1) == BAD_ARG
    for i in range(4):    # (nor here: the reserved words are looked at before the batch)
        assert L.iamf_hip_batch_render_ragged(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i


# ---- the cases of the GPU tests: the limiter works across every call boundary ----

def test_the_default_routes_of_the_cases():
    """what the GPU tests assert per call is what the length and position rules give"""
    want = {"frame_1000": "RR", "lengths": "R" * 8, "frames_100": "RRRR", "frames_1000": "RR", "mod4": "RRR", "first_100": "RGR",
            "mixed": "RFRFR"}
    for name, (m, oc, fs, calls) in RU.CASES.items():
        got = "".join({RU.RAG: "R", "FAST": "F", "GENERIC": "G"}[r] for r in RU.default_routes(fs, calls))
        assert got == want[name], (name, got)
        assert (m, oc) in RU.INSTANCES and fs % 4 == 0
        for nf, ns in calls:
            assert nf >= 1 and 0 <= ns <= fs and (ns == 0 or nf == 1)


PROOFS = RU.proofs()


def test_the_proofs_cover_every_case_and_every_instance():
    labels = [p[0] for p in PROOFS]
    assert len(labels) == len(set(labels)) and set(RU.CASES) <= set(labels)
    assert {(p[1], p[2]) for p in PROOFS if p[0].startswith("instance ")} == set(RU.INSTANCES)


@pytest.mark.parametrize("proof", PROOFS, ids=[p[0] for p in PROOFS])
def test_the_limiter_attenuates_across_every_call_boundary(proof):
    """for every programme a limiter-on GPU test renders (ragged_util.proofs): the first call triggers, and at every call
    boundary the limiter is in attack or release with a gain below 1"""
    import oracle_lib as O
    name, m, oc, fs, calls, streams, egs, ogs = proof
    sz = RU.sizes(fs, calls)
    x = RU.hot(m, sum(sz), streams=streams)
    _, omx = RU.IU.dense_matrices(m, oc)
    for s in range(streams):
        _, z = RU.want(omx, oc, x[s], sz, 16, egs[s % len(egs)], ogs[s % len(ogs)])
        y, t = O.limiter_trace(z, sz)
        trig = np.flatnonzero(t & O.LIM_TRIGGER)
        assert trig.size and trig[0] < sz[0], (name, s, "the first call triggers")
        for e in np.cumsum(sz)[:-1]:
            e = int(e)
            what = (name, s, e)
            # the last step of the call and the first of the next are in attack or release, and the gain is below 1 there:
            # the output sample each of them emits (240 behind) is smaller than its input
            assert (t[e - 1] & 3) != O.LIM_IDLE and (t[e] & 3) != O.LIM_IDLE, what
            for k in (e - 1, e):
                j = k - 240
                if j < 0:
                    continue
                c = int(np.argmax(np.abs(z[:, j])))
                assert z[c, j] != 0.0 and abs(y[c, j]) < abs(z[c, j]), what
