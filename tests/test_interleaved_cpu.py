"""No GPU: iamf_hip_batch_render_interleaved is declared, exported and bound, and its ctypes mirror has the C struct's size and
offsets (a compiled probe says them); its family (FAST_INTERLEAVED = 27) lists exactly the 4 instances, which no numbered
table lists; every instance has a GPU case; the refusals that need no device answer IAMF_HIP_ERR_BAD_ARG; and the programmes
of the seam tests (tests/test_gpu_interleaved.py) are proven, from the oracle's limiter trace, to put their triggers where
the tests say: on the last sample of a ragged call, on the first sample of the next, inside the partial last block, with a
release that runs across three calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import iac_amd as A
import interleaved_util as IU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
FAMILY = 27


def _header():
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        return f.read()


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_interleaved" in names and hasattr(A.lib(), "iamf_hip_batch_render_interleaved")
    assert "iamf_hip_fast_interleaved_launch" not in names       # the launch entry stays hidden
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_interleaved\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_interleaved_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*iamf_hip_render_args args;\s*int32_t reserved\[4\];\s*\}\s*iamf_hip_interleaved_call;", src)
    assert re.search(r"IAMF_HIP_ROUTE_FAST_INTERLEAVED\s*=\s*%d\b" % FAMILY, src)
    assert A.ROUTE["FAST_INTERLEAVED"] == FAMILY and A.hipabi.ROUTE_NAME[FAMILY] == "FAST_INTERLEAVED"
    assert A.hipabi.ROUTE_NAME[25] == "LPCM_MIX" and A.hipabi.ROUTE_NAME[20] == "RS_PLAIN"      # the numbers in use keep their names
    assert callable(A.Batch.render_interleaved)
    assert A.lib().iamf_hip_batch_render_interleaved.argtypes[1]._type_ is A.InterleavedCall


def test_the_mirror_has_the_c_structs_size_and_offsets(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "iamf_hip.h"\n'
                'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(iamf_hip_interleaved_call), offsetof(iamf_hip_interleaved_call, args),\n'
                '                        offsetof(iamf_hip_interleaved_call, reserved), sizeof(iamf_hip_render_args)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    size, o_args, o_res, args_size = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert (C.sizeof(A.InterleavedCall), A.InterleavedCall.args.offset, A.InterleavedCall.reserved.offset) == (size, o_args, o_res)
    assert C.sizeof(A.RenderArgs) == args_size and o_args == 0 and o_res == args_size and size == args_size + 16


def test_the_family_has_4_rows_and_shares_none_with_a_table():
    rows = A.route_family_instances("FAST_INTERLEAVED")
    assert len(rows) == len(set(rows)) == 4 and set(rows) == {IU.inst(m, oc) for m in (1, 2) for oc in (1, 2)}
    assert A.route_family_instances(FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(FAMILY, None, 0) == 4
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == "FAST_INTERLEAVED"], t
    for other in ("LPCM_COUPLED", "LPCM_MIX", "FAST"):
        assert not set(rows) & set(A.route_family_instances(other))
    row = (A.RouteRow * 3)()
    assert A.lib().iamf_hip_route_family_instances(FAMILY, row, 3) == 4       # cap rows filled, the count returned
    assert all(r.family == FAMILY and r.variant == 0 and r.k == 0 and r.launches == 0 for r in row)
    assert A.route_family_tally("FAST_INTERLEAVED") == {} and A.route_family_tally("FAST_INTERLEAVED", reset=True) == {}


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    assert len(A.route_family_instances("LPCM_COUPLED")) == 20 and len(A.route_family_instances("LPCM_MIX")) == 36
    for fam in (18, 19, 24, 26, 28):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def test_every_instance_has_a_gpu_case():
    import test_gpu_interleaved as TG
    marks = [m for m in TG.test_every_instance.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "m,oc"
    cases = [IU.inst(m, oc) for m, oc in marks[0].args[1]]
    assert len(cases) == len(set(cases)) and set(cases) == set(A.route_family_instances("FAST_INTERLEAVED"))
    assert IU.INSTANCES == [(r[2], r[3]) for r in A.route_family_instances("FAST_INTERLEAVED")]


def _call(reserved=None, d_in=0x1000, d_pcm=0x3000, n_frames=1115):
    call = A.InterleavedCall()
    call.args.d_in, call.args.d_pcm, call.args.n_frames, call.args.in_frame_stride = d_in, d_pcm, n_frames, 2
    if reserved is not None:
        call.reserved[reserved] = 1
    return call


def test_null_arguments_and_reserved_words_are_refused_without_a_device():
    L = A.lib()
    assert L.iamf_hip_batch_render_interleaved(None, C.byref(_call()), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_interleaved(0x4000, None, 0, 1) == BAD_ARG       # (the fake handle is never read: `call` is looked at first)
    assert L.iamf_hip_batch_render_interleaved(None, None, 0, 1) == BAD_ARG
    for i in range(4):    # (nor here: the reserved words are looked at before the batch)
        assert L.iamf_hip_batch_render_interleaved(0x4000, C.byref(_call(reserved=i)), 0, 1) == BAD_ARG, i


# ---- the seam programmes: where the oracle's limiter triggers ----

def test_the_plateau_triggers_on_the_seam():
    import oracle_lib as O
    x, lengths, onsets = IU.seam_plateau()
    assert lengths == [1115, 1114, 1115] and lengths[0] % 4 and lengths[0] % 64 == 27       # a ragged call, a partial last block of 27
    first = []
    for s in range(3):
        t, tr = IU.first_trigger(x[s], lengths)
        first.append(t)
        assert not (tr[:t] & O.LIM_TRIGGER).any() and (tr[t:t + 240] & O.LIM_TRIGGER).all(), s      # held by the plateau from there on
        assert float(np.abs(x[s][:, :onsets[s]]).max(initial=0.0)) == 0.0
    assert first == IU.SEAM_TRIGGERS == [lengths[0] - 1, lengths[0], 1100]
    assert 64 * (lengths[0] // 64) <= first[2] < lengths[0] - 1       # inside the partial last block, not its last sample


def test_the_retrigger_programme_releases_across_three_calls():
    import oracle_lib as O
    import programmes as P
    x, lengths, ks = IU.seam_retrigger()
    starts = np.concatenate([[0], np.cumsum(lengths)])
    assert lengths[0] == P.LAST_TRIGGER + 1 and all(n % 4 for n in lengths)
    for s, k in enumerate(ks):
        _, tr = IU.first_trigger(x[s], lengths)
        hits = np.flatnonzero(tr & O.LIM_TRIGGER)
        run1 = hits[hits <= P.LAST_TRIGGER]
        assert run1[-1] == lengths[0] - 1 == P.LAST_TRIGGER       # the first run's last trigger: the last sample of the ragged call 0
        again = int(hits[hits > P.LAST_TRIGGER][0])
        assert again > starts[1] and not (tr[starts[1]:again] & O.LIM_TRIGGER).any()
        phase = tr & 3
        if k == 5:    # one step before idle: the release has run across calls 1, 2 and 3
            assert starts[3] < again < starts[4]
            for c in (1, 2):
                assert (phase[starts[c] + 48:starts[c + 1]] == O.LIM_RELEASE).all(), (k, c)
            assert (phase[starts[3]:again] == O.LIM_RELEASE).all()
        else:         # in the attack / the early release of call 1
            assert starts[1] < again < starts[2]
