"""-m gpu: the render kernels on padded, offset and far-apart buffer layouts.

include/iamf_hip.h lets a caller place its input, second element, ramps and PCM rows freely; pick_route()
(iac_amd/csrc/render_route.hpp) sends a call to a vector kernel only if pointers and strides keep the 16-byte rules and a
call's input fits 32-bit byte offsets, and tests/test_route_host.py pins those rules.  Every other GPU test uses one
layout: dense frames of a fresh allocation and PCM rows back to back.  Here cases of tests/route_cases.py run again, as
they are (three streams, calls of 1 to 3 frames with the state carried over, the flush, the builders' own comparison with
the oracle), under each layout of tests/gpu_util.py (the table there; tests/test_layouts_cpu.py tests the helper):

  DENSE, PAD16, FRAME_MAJOR   the launch tally is the case's own: the named instance ran on every call
  OFF_IN, OFF_PCM             the tally is what the rules say (ROUTED below); FIR calls are refused, change nothing, and the
                              same batch then renders the programme under PAD16
  FAR_IN, FAR_PCM             frames 2^31 + 16 bytes apart / PCM rows 2^31 + 16 bytes apart, two calls of 1 and 3 frames

Under every layout gpu_util.rows_and_rest holds after every call and the flush: no byte outside the emitted runs is
written.  Every float between the samples is a NaN and the programmes are finite, so a kernel that steps by the dense
stride, narrows an offset to 32 bits or reads a gap differs from the oracle."""
import pytest

import gpu_util as G
import route_cases as R

pytestmark = pytest.mark.gpu

UNIMPLEMENTED, BAD_ARG = -6, -1      # IAMF_HIP_ERR_*

IDS = """generic_m2 generic_m24 nolim_m2 nolim_m24
fast_m1_oc1 fast_m16_oc2 fast_m24_oc2 fast_m4_oc2_mix fast_m16_oc1_mix fast_down_8_2 fast_down_2_1
wide_m12_c11 wide_m16_c11_mfma wide_m12_c11_s24 wide_m12_c12_s32 wide_m24_c24
wide4_m4_c6 wide4_m12_c12 wide4_m16_c24 wide4_m16_c14_mfma
wide4_demix_m12_c12 wide4_demix_m6_c24 wide4_down_12_6 wide4_down_8_6 wide4_mix_m16_c12 wide4_mix_m4_c6_mfma
wide4_lfe_m16_c6 wide4_lfe_m4_c24 wide4_lfe_m4_c6_511_streams
lpcm_m16_oc2_early lpcm_m1_oc1_late
fanout_m16_k2 fanout_m4_k4
fir_split_m16 fir_split_m12 fir_fused3_m4 fir_fused2_m16 fir_fused1_m6
rs_plain rs_tile_interpolated rs_tile_direct rs_block_c2_r1 rs_block_c8_r2 rs_direct_c2_n64 rs_direct_c2_n128
rs_direct_c6_n192""".split()
FAR_IDS = """generic_m2 nolim_m24 wide_m12_c11_s24 wide4_m12_c12 wide4_mix_m16_c12 wide4_demix_m12_c12 wide4_down_12_6
wide4_lfe_m16_c6 fast_m16_oc2 fanout_m16_k2 fir_split_m16""".split()
FAR_CALLS = [1, 3]                    # one call spans both 32-bit crossings

BY_ID = {c.id: c for c in R.CASES}
assert all(i in BY_ID for i in IDS + FAR_IDS)

GENERIC, SAME, REFUSED, SINGLY = "generic", "same", "refused", "singly"
# What a family's calls take once a layout breaks the 16-byte rules, as tests/route_host/route_host_check.cpp pins them
# (the rows of its address rules).  OFF_IN breaks them for the input, the second element and the ramps, OFF_PCM for the PCM.
ROUTED = {
    #               OFF_IN    OFF_PCM
    "GENERIC":     (SAME,     SAME),
    "NOLIM":       (GENERIC,  GENERIC),
    "FAST":        (GENERIC,  GENERIC),
    "FAST_DOWN":   (GENERIC,  GENERIC),
    "WIDE":        (SAME,     GENERIC),    # render_wide_kernel loads scalars: wide_shape_ok looks at the PCM only
    "WIDE4":       ("WIDE",   GENERIC),
    "WIDE4_DEMIX": (GENERIC,  GENERIC),    # the 256-sample kernel has no stage in front of the projection
    "WIDE4_DOWN":  (GENERIC,  GENERIC),
    "WIDE4_MIX":   (GENERIC,  GENERIC),
    "WIDE4_LFE":   (GENERIC,  GENERIC),
    "LPCM":        (SAME,     GENERIC),    # where the packets lie: tests/test_gpu_packet_layouts.py; an offset PCM: unpacked, then the f32 path
    "FANOUT":      (SINGLY,   SINGLY),     # no member is a call of the fast kernel: each is rendered on its own
    "FIR_SPLIT":   (REFUSED,  REFUSED),
    "FIR_FUSED":   (REFUSED,  REFUSED),
    "RS_PLAIN":    (SAME,     SAME),       # the resampler's kernels load scalars
    "RS_TILE":     (SAME,     SAME),
    "RS_BLOCK":    (SAME,     SAME),
    "RS_DIRECT":   (SAME,     SAME),
}
# FAR_IN: render_fast_kernel addresses a stream's input of one call with 32-bit byte offsets (fast_shape_ok:
# (frames + 2) * in_frame_stride * 4 + 100 * frame_size < 2^31, so neither call of FAR_CALLS is its), the FIR stage keeps
# 32-bit float offsets (BAD_ARG from (frames + 1) * in_frame_stride >= 2^31: the 3-frame call).  The other kernels
# compute 64-bit addresses and keep their calls.  FAR_PCM: every kernel computes a row's address in 64 bits.
FAR_ROUTED = {"FAST": GENERIC, "FANOUT": SINGLY, "FIR_SPLIT": REFUSED}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available()


def _under(case, layout, how, **kw):
    """the case under a layout, with the instance its calls are expected to take"""
    m = case.inst[2]
    kw = dict(case.kw, layout=layout, **kw)
    inst = case.inst
    if how == GENERIC:
        inst = R.gen(m)
    elif how == "WIDE":
        inst = ("WIDE", case.inst[1], m, 0, 0)
    elif how == SINGLY:
        inst, kw["fused"] = R.gen(m), 0
    elif how == REFUSED:
        raise AssertionError("a refused call has no instance")
    else:
        assert how == SAME
    return case._replace(inst=inst, kw=kw)


def _clean_env(case, monkeypatch):
    for k in ("IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_PROJECTION", "IAMF_HIP_LP_LATE", "IAMF_HIP_LPCM_UNFUSED",
              "IAMF_HIP_FIR_FUSED", "IAMF_HIP_FIR_F16", "IAMF_HIP_FIR_F32", "IAMF_HIP_RESAMPLE_TILE", "IAMF_HIP_RESAMPLE_PLAIN"):
        if k not in case.kw.get("env", {}):
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("layout", [G.DENSE, G.PAD16, G.FRAME_MAJOR], ids=lambda l: l.name)
@pytest.mark.parametrize("cid", IDS)
def test_aligned_layouts_keep_the_instance(cid, layout, monkeypatch):
    case = BY_ID[cid]
    _clean_env(case, monkeypatch)
    c = _under(case, layout, SAME)
    c.build(c)


@pytest.mark.parametrize("layout", [G.OFF_IN, G.OFF_PCM], ids=lambda l: l.name)
@pytest.mark.parametrize("cid", IDS)
def test_offset_layouts_take_the_route_the_rules_say(cid, layout, monkeypatch):
    case = BY_ID[cid]
    _clean_env(case, monkeypatch)
    how = ROUTED[case.inst[0]][0 if layout == G.OFF_IN else 1]
    if how == REFUSED:
        # refused before anything is launched or changed: the batch then renders the whole programme under PAD16
        c = _under(case, G.PAD16, SAME, refused=(layout, UNIMPLEMENTED, 1))
    else:
        c = _under(case, layout, how)
    c.build(c)


@pytest.mark.parametrize("layout", G.FAR_LAYOUTS, ids=lambda l: l.name)
@pytest.mark.parametrize("cid", FAR_IDS)
def test_far_layouts(cid, layout, monkeypatch):
    import torch
    case = BY_ID[cid]
    _clean_env(case, monkeypatch)
    how = FAR_ROUTED.get(case.inst[0], SAME) if layout == G.FAR_IN else SAME
    try:
        if how == REFUSED:
            c = _under(case, G.PAD16, SAME, calls=FAR_CALLS, refused=(layout, BAD_ARG, 3))
        else:
            c = _under(case, layout, how, calls=FAR_CALLS)
        c.build(c)
    finally:
        torch.cuda.empty_cache()     # gigabytes: not kept for the tests behind this one
