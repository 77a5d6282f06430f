"""-m gpu: the decoder façade and the decoder groups hand BOTH elements' packets of a two-element handle with a resampler behind it,
or with the limiter switched off, to iamf_hip_batch_render_packets_mix_nolim (render_launch of iamf_decoder_facade.c,
group_run_lpcm_mix of iamf_decoder_group.inc), ramps and element-2 gain as the limiter-on two-element path hands them over.

The streams are stored fuzz streams (tests/e2e_fuzz.py, PCM hashes of the real reference in tests/golden/), selected by
configuration (nolim_packets_mix_util.facade_streams; tests/test_nolim_packets_mix_cpu.py names those that must be among them):
each through a single handle and through a group of four.  Each asserts that the PCM hash and the values returned (one handle: the
metadata rows too) are the stored reference's; that the family's tally shows the stream's instance once per frame whose kept samples start at a
multiple of 4 and number a positive multiple of 4, where the first stage's PCM sample-frame is whole dwords of at most 60 bytes
(a group: at least that), and is empty otherwise; that a resampling stream into stereo or mono with the limiter on ran the
interleaved form of the fast kernel behind the resampler, as before; and that the PCM is byte-equal under IAMF_HIP_FACADE_UNPACK=1 /
IAMF_HIP_GROUP_UNPACK=1, where the family's tally stays empty.  No existing test pins another route for a two-element first stage,
so no selected stream is left out."""
import json
import os

import numpy as np
import pytest

import e2e_fuzz as F
import nolim_packets_mix_util as U
import route_cases as R
from decoder_driver import decode_stream
from test_gpu_group import group_decode_all, lib  # noqa: F401  (the fixture that declares the group entry points)

pytestmark = pytest.mark.gpu

_G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = {v: json.load(open(os.path.join(_G, name))) for v, name in U.FACADE_GOLD.items()}
STREAMS = U.facade_streams()
IDS = ["%s_%d" % (v, s) for v, s, _ in STREAMS]
SWITCHES = ("IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED", "IAMF_HIP_NOLIM_PACKETS_UNFUSED", "IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED",
            "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_FACADE_UNPACK", "IAMF_HIP_GROUP_UNPACK", "IAMF_HIP_INTERLEAVED_UNFUSED")


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _instance(c):
    import iac_amd as A
    row = U.facade_instance(c)
    assert row in A.route_family_instances(U.FAM)
    return row


def _tallies(A):
    fam, _, rest = U._tallies(A)
    return fam, {k: v for k, v in rest.items() if k[0] == U.IL}


@pytest.mark.parametrize("variant,seed,frames", STREAMS, ids=IDS)
def test_a_stored_fuzz_stream_through_one_handle(lib, variant, seed, frames):  # noqa: F811
    import iac_amd as A
    want = GOLD[variant][str(seed)]
    stream, c = F.build(seed, variant)
    U._reset(A)
    md = dict(rows=[], owns_anchors=True, strict=False)
    pcm, rets = decode_stream(lib, stream, c["layout"], metadata=md, **F.decode_kwargs(c, variant))
    fam, il = _tallies(A)
    print(variant, seed, "family:", fam, "interleaved:", il, "fused frames:", len(frames), "of", c["frames"])
    assert fam == ({_instance(c): len(frames)} if frames else {}), (variant, seed, fam, len(frames))
    assert bool(il) or not U.facade_resamples_into_one_or_two(c), (variant, seed, il)
    assert [int(r) for r in rets][:len(want["rets"])] == want["rets"] and list(pcm.shape) == want["shape"], (variant, seed)
    assert F.digest(pcm) == want["sha256"], (variant, seed, "the PCM hash of the real reference")
    assert F.meta_digest(md) == want["meta"], (variant, seed, "IAMF_decoder_get_last_metadata rows")
    with R.environment({"IAMF_HIP_FACADE_UNPACK": "1"}):
        twin, rets_twin = decode_stream(lib, stream, c["layout"], metadata=dict(rows=[], owns_anchors=True, strict=False), **F.decode_kwargs(c, variant))
        fam, _ = _tallies(A)
    assert fam == {} and [int(r) for r in rets_twin] == [int(r) for r in rets], (variant, seed, fam)
    assert np.array_equal(pcm, twin), (variant, seed, "byte-equal on the f32 path")


@pytest.mark.parametrize("variant,seed,frames", STREAMS, ids=IDS)
def test_a_stored_fuzz_stream_through_a_group_of_four(lib, variant, seed, frames):  # noqa: F811
    """four handles of a group, in step: each handle's PCM is the reference's; the family's row shows (a run of the group is one
    launch over the handles that stand at the same frame, so the count is at least one per fused frame)"""
    import iac_amd as A
    want = GOLD[variant][str(seed)]
    stream, c = F.build(seed, variant)

    def run():
        U._reset(A)
        rc, outs = group_decode_all(lib, dict(c), stream, 4, 2, starve=lambda r, i: False)
        assert rc == 0, (variant, seed, rc)
        return outs, _tallies(A)

    outs, (fam, il) = run()
    row = _instance(c)
    assert (set(fam) == {row} and fam[row] >= len(frames)) if frames else fam == {}, (variant, seed, fam, len(frames))
    assert bool(il) or not U.facade_resamples_into_one_or_two(c), (variant, seed, il)
    for i, (pcm, rets) in enumerate(outs):
        assert [int(r) for r in rets] == want["rets"], (variant, seed, i)
        assert F.digest(pcm) == want["sha256"], (variant, seed, i, "the PCM hash of the real reference")
    with R.environment({"IAMF_HIP_GROUP_UNPACK": "1"}):
        twins, (fam, _) = run()
    assert fam == {}, (variant, seed, fam)
    for i, ((pcm, _), (twin, _)) in enumerate(zip(outs, twins)):
        assert np.array_equal(pcm, twin), (variant, seed, i, "byte-equal on the f32 path")
