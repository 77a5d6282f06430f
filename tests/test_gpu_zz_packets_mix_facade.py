"""-m gpu: the decoder façade and the decoder groups hand BOTH elements' packets of a two-element presentation to
iamf_hip_batch_render_packets_mix_ragged (render_launch of iamf_decoder_facade.c, group_run_lpcm_mix of iamf_decoder_group.inc):
whole 64-sample blocks take the whole-block mix kernels (LPCM_MIX, LPCM24_MIX), a trimmed end or a frame of 1000 the ragged
two-element form (PACKETS_MIX_RAGGED), with or without gain ramps.

The streams are stored fuzz streams (tests/e2e_fuzz.py, PCM hashes of the real reference in tests/golden/), selected by
configuration (packets_mix_ragged_util.facade_mix_streams; tests/test_packets_mix_ragged_cpu.py asserts what is selected): each
through a single handle and through a group of four.  Each asserts the families' tallies, that the PCM hash and the values
returned are the stored reference's, and that the PCM is byte-equal under IAMF_HIP_FACADE_UNPACK=1 / IAMF_HIP_GROUP_UNPACK=1,
where the mix families' tallies stay empty."""
import json
import os

import numpy as np
import pytest

import e2e_fuzz as F
import packets_mix_ragged_util as U
import route_cases as R
from decoder_driver import decode_stream
from test_gpu_fuzz_facade import _Variant
from test_gpu_group import group_decode_all, lib  # noqa: F401  (the fixture that declares the group entry points)

pytestmark = pytest.mark.gpu

_G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = {"default": json.load(open(os.path.join(_G, "fuzz.json"))), "lfe": json.load(open(os.path.join(_G, "fuzz_lfe.json")))}
STREAMS = U.facade_mix_streams()
IDS = ["%s_%d" % (v, s) for v, s, _ in STREAMS]


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in ("IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_FORCE_GENERIC",
              "IAMF_HIP_FACADE_UNPACK", "IAMF_HIP_GROUP_UNPACK"):
        monkeypatch.delenv(k, raising=False)


def _reset(A):
    for f in U.MIX_FAMILIES:
        A.route_family_tally(f, reset=True)


def _mix_tallies(A):
    """the launches of the three two-element packet families since the last reset, as one dict"""
    out = {}
    for f in U.MIX_FAMILIES:
        out.update(A.route_family_tally(f, reset=True))
    return out


def _rows(fr):
    """what a single handle must have launched: the ragged instance once per ragged frame, the whole-block one once per whole"""
    import iac_amd as A
    bps, m, oc, k = fr["inst"]
    assert U.inst(bps, m, oc, k) in A.route_family_instances(U.FAM) and U.whole(bps, m, oc, k) in A.route_family_instances(U.WHOLE[bps])
    want = {}
    if fr["ragged"]:
        want[U.inst(bps, m, oc, k)] = len(fr["ragged"])
    if fr["whole"]:
        want[U.whole(bps, m, oc, k)] = len(fr["whole"])
    return want


@pytest.mark.parametrize("variant,seed,fr", STREAMS, ids=IDS)
def test_a_stored_fuzz_stream_through_one_handle(lib, variant, seed, fr):  # noqa: F811
    import iac_amd as A
    want = GOLD[variant][str(seed)]
    stream, c = F.build(seed, variant)
    dlib = _Variant(lib, variant) if variant == "lfe" else lib          # (the set's own switch: the HOA LFE generator compiled in)
    _reset(A)
    pcm, rets = decode_stream(dlib, stream, c["layout"], **F.decode_kwargs(c, variant))
    fam = _mix_tallies(A)
    assert fam == _rows(fr), (variant, seed, fam, _rows(fr))
    assert [int(r) for r in rets][:len(want["rets"])] == want["rets"] and list(pcm.shape) == want["shape"], (variant, seed)
    assert F.digest(pcm) == want["sha256"], (variant, seed, "the PCM hash of the real reference")
    with R.environment({"IAMF_HIP_FACADE_UNPACK": "1"}):
        twin, rets_twin = decode_stream(dlib, stream, c["layout"], **F.decode_kwargs(c, variant))
        fam = _mix_tallies(A)
    assert fam == {} and [int(r) for r in rets_twin] == [int(r) for r in rets], (variant, seed, fam)
    assert np.array_equal(pcm, twin), (variant, seed, "byte-equal with IAMF_HIP_FACADE_UNPACK=1")


@pytest.mark.parametrize("variant,seed,fr", STREAMS, ids=IDS)
def test_a_stored_fuzz_stream_through_a_group_of_four(lib, variant, seed, fr):  # noqa: F811
    """four handles of a group, in step: each handle's PCM is the reference's; the families' rows show (a run of the group is
    one launch over the handles that stand at the same frame, so a row's count is at least one per frame of its kind)"""
    import iac_amd as A
    want = GOLD[variant][str(seed)]
    stream, c = F.build(seed, variant)
    case = dict(c, lfe_hoa=True) if variant == "lfe" else dict(c)

    def run():
        _reset(A)
        rc, outs = group_decode_all(lib, dict(case), stream, 4, 2, starve=lambda r, i: False)
        assert rc == 0, (variant, seed, rc)
        return outs, _mix_tallies(A)

    outs, fam = run()
    rows = _rows(fr)
    assert set(fam) == set(rows) and all(fam[k] >= rows[k] for k in rows), (variant, seed, fam, rows)
    for i, (pcm, rets) in enumerate(outs):
        assert [int(r) for r in rets] == want["rets"], (variant, seed, i)
        assert F.digest(pcm) == want["sha256"], (variant, seed, i, "the PCM hash of the real reference")
    with R.environment({"IAMF_HIP_GROUP_UNPACK": "1"}):
        twins, fam = run()
    assert fam == {}, (variant, seed, fam)
    for i, ((pcm, _), (twin, _)) in enumerate(zip(outs, twins)):
        assert np.array_equal(pcm, twin), (variant, seed, i, "byte-equal with IAMF_HIP_GROUP_UNPACK=1")
