"""No GPU: iamf_hip_batch_render_lpcm_mix is declared, exported and bound; its family (LPCM_MIX) lists exactly the 36
instances of the two-element packet form, which no numbered table lists; every instance has a case in
tests/route_cases_lpcm_mix.py; and the refusals that need no device answer IAMF_HIP_ERR_BAD_ARG (the others need a batch,
which needs a device: tests/test_gpu_lpcm_mix.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import iac_amd as A
import route_cases_lpcm_mix as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
FAMILY = 25      # 20 .. 23 are the resampler's families; 18, 19 and 24 stay "no such family" (tests/test_lpcm_coupled_cpu.py)


def _header():
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        return f.read()


def test_the_entry_is_declared_exported_and_mirrored():
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "iamf_hip_batch_render_lpcm_mix" in names and hasattr(A.lib(), "iamf_hip_batch_render_lpcm_mix")
    assert "iamf_hip_fast_lpcm_mix_launch" not in names and "iamf_hip_fast_lpcm_mix_coupled_launch" not in names   # internal entries
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_lpcm_mix\s*\(\s*iamf_hip_batch \*b,\s*const iamf_hip_lpcm_mix_call \*call,\s*"
                     r"int32_t stream0,\s*int32_t n_streams\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s*\{\s*iamf_hip_lpcm_input in\[2\];\s*iamf_hip_render_args args;\s*\}\s*iamf_hip_lpcm_mix_call;", src)
    assert re.search(r"IAMF_HIP_ROUTE_LPCM_MIX\s*=\s*%d\b" % FAMILY, src)
    assert A.ROUTE["LPCM_MIX"] == FAMILY and A.hipabi.ROUTE_NAME[FAMILY] == "LPCM_MIX"
    assert A.hipabi.ROUTE_NAME[20] == "RS_PLAIN"                       # the numbers in use keep their names
    assert C.sizeof(A.LpcmMixCall) == 2 * C.sizeof(A.LpcmInput) + C.sizeof(A.RenderArgs)
    assert A.LpcmMixCall.args.offset == 2 * C.sizeof(A.LpcmInput)
    assert callable(A.Batch.render_lpcm_mix)
    assert A.lib().iamf_hip_batch_render_lpcm_mix.argtypes[1]._type_ is A.LpcmMixCall


def test_the_family_has_36_rows_and_shares_none_with_a_table():
    rows = A.route_family_instances("LPCM_MIX")
    want = {("LPCM_MIX", 0, m, oc, k) for m in RM.LPCM_M + RM.COUPLED_M for oc in RM.MIX_OC for k in RM.MIX_K}
    assert len(rows) == len(set(rows)) == 36 and set(rows) == want
    assert A.route_family_instances(FAMILY) == rows
    assert A.lib().iamf_hip_route_family_instances(FAMILY, None, 0) == 36
    for t in range(A.route_tables()):
        listed = A.route_table_instances(t)
        assert not set(rows) & set(listed) and not [r for r in listed if r[0] == "LPCM_MIX"], t
    assert not set(rows) & set(A.route_family_instances("LPCM_COUPLED"))
    row = (A.RouteRow * 3)()
    assert A.lib().iamf_hip_route_family_instances(FAMILY, row, 3) == 36     # cap rows filled, the count returned
    assert all(r.family == FAMILY and r.variant == 0 and r.launches == 0 for r in row)
    assert A.route_family_tally("LPCM_MIX") == {} and A.route_family_tally("LPCM_MIX", reset=True) == {}
    assert A.lib().iamf_hip_route_family_tally(FAMILY, None, 0, 0) == 0


def test_the_tables_and_the_other_families_are_as_they_were():
    assert A.route_tables() == 3
    assert A.lib().iamf_hip_route_table_instances(3, None, 0) == -1
    assert len(A.route_table_instances(2)) == 16 and len(A.route_instances_ext()) == 9
    assert len(A.route_family_instances("LPCM_COUPLED")) == 20
    assert A.route_family_instances("RS_PLAIN") == [("RS_PLAIN", 0, 0, 0, 0)]
    for fam in (18, 19, 24, 26):
        assert A.lib().iamf_hip_route_family_instances(fam, None, 0) == -1, fam


def test_every_instance_has_a_case():
    rows = A.route_family_instances("LPCM_MIX")
    insts = [c.inst for c in RM.CASES]
    assert len(insts) == len(set(insts)) and set(insts) == set(rows)
    assert len({c.id for c in RM.CASES}) == len(RM.CASES)
    for c in RM.CASES:
        assert c.build is RM.run_mix and c.inst == RM.inst(c.kw["m"], c.kw["oc"], c.kw["k"])


def _call(d_raw0=0x1000, d_raw1=0x2000, d_in=None, d_in2=None, d_pcm=0x3000, n_frames=1, first=(0, 0)):
    call = A.LpcmMixCall()
    call.in_[0].d_raw, call.in_[1].d_raw = d_raw0, d_raw1
    call.in_[0].first_sample, call.in_[1].first_sample = first
    call.args.d_in, call.args.d_in2, call.args.d_pcm, call.args.n_frames = d_in, d_in2, d_pcm, n_frames
    return call


def test_null_arguments_are_refused_without_a_device():
    L = A.lib()
    assert L.iamf_hip_batch_render_lpcm_mix(None, C.byref(_call()), 0, 1) == BAD_ARG
    assert L.iamf_hip_batch_render_lpcm_mix(0x4000, None, 0, 1) == BAD_ARG        # (the fake handle is never read: `call` is looked at first)
    assert L.iamf_hip_batch_render_lpcm_mix(None, None, 0, 1) == BAD_ARG
