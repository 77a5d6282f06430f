"""-m gpu: the decoder façade and the decoder groups hand element 0's packets to iamf_hip_batch_render_packets_ragged
(render_launch of iamf_decoder_facade.c, group_run_lpcm of iamf_decoder_group.inc), so a frame whose kept samples are no whole
number of 64-sample blocks — a trimmed end, a frame of 1000 — takes the ragged packet form of the headline kernel.

The streams are stored fuzz streams (tests/e2e_fuzz.py, PCM hashes of the real reference in tests/golden/), selected by
configuration (packets_ragged_util.facade_streams; tests/test_packets_ragged_cpu.py asserts that some are selected): one through
a single handle and through a group of four.  Each asserts that the family's tally is not empty, that the PCM hash and the
values returned are the stored reference's, and that the PCM is byte-equal under IAMF_HIP_PACKETS_RAGGED_UNFUSED=1, where the
family's tally stays empty."""
import json
import os

import numpy as np
import pytest

import e2e_fuzz as F
import packets_ragged_util as PU
import route_cases as R
from decoder_driver import decode_stream
from test_gpu_group import group_decode_all, lib  # noqa: F401  (the fixture that declares the group entry points)

pytestmark = pytest.mark.gpu

_G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = {"default": json.load(open(os.path.join(_G, "fuzz.json"))), "wide": json.load(open(os.path.join(_G, "fuzz_wide.json")))}
STREAMS = PU.facade_streams()
UNFUSED = {"IAMF_HIP_PACKETS_RAGGED_UNFUSED": "1"}


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in ("IAMF_HIP_PACKETS_RAGGED_UNFUSED", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_FACADE_UNPACK", "IAMF_HIP_GROUP_UNPACK"):
        monkeypatch.delenv(k, raising=False)


def _family_rows(c, frames):
    """what the family's tally must show for a single handle: the stream's instance, once per selected frame"""
    import iac_amd as A
    form = {(16, False): "s16", (24, False): "s24", (16, True): "s16c"}[(c["sample_size"], c["pair"][0] not in ("zoa", "foa", "soa", "toa"))]
    m = {"zoa": 1, "foa": 4, "soa": 9, "toa": 16, "stereo": 2, "l51": 6, "l512": 8, "l71": 8, "l514": 10, "l712": 10, "l714": 12}[c["pair"][0]]
    oc = 2 if c["layout"] == ("ss", 0) else 1
    assert PU.inst(form, m, oc) in A.route_family_instances(PU.FAM)
    return {PU.inst(form, m, oc): len(frames)}


@pytest.mark.parametrize("variant,seed,frames", STREAMS, ids=["%s_%d" % (v, s) for v, s, _ in STREAMS])
def test_a_stored_fuzz_stream_through_one_handle(lib, variant, seed, frames):  # noqa: F811
    import iac_amd as A
    want = GOLD[variant][str(seed)]
    stream, c = F.build(seed, variant)
    PU._reset(A)
    pcm, rets = decode_stream(lib, stream, c["layout"], **F.decode_kwargs(c, variant))
    fam, _, _ = PU._tallies(A)
    assert fam == _family_rows(c, frames), (variant, seed, fam)
    assert [int(r) for r in rets][:len(want["rets"])] == want["rets"] and list(pcm.shape) == want["shape"], (variant, seed)
    assert F.digest(pcm) == want["sha256"], (variant, seed, "the PCM hash of the real reference")
    with R.environment(UNFUSED):
        twin, rets_twin = decode_stream(lib, stream, c["layout"], **F.decode_kwargs(c, variant))
        fam, _, _ = PU._tallies(A)
    assert fam == {} and [int(r) for r in rets_twin] == [int(r) for r in rets], (variant, seed, fam)
    assert np.array_equal(pcm, twin), (variant, seed, "byte-equal with IAMF_HIP_PACKETS_RAGGED_UNFUSED=1")


@pytest.mark.parametrize("variant,seed,frames", STREAMS, ids=["%s_%d" % (v, s) for v, s, _ in STREAMS])
def test_a_stored_fuzz_stream_through_a_group_of_four(lib, variant, seed, frames):  # noqa: F811
    """four handles of a group, in step: each handle's PCM is the reference's; the family's rows show (a run of the group is
    one launch over the handles that stand at the same frame, so the count is at least one per selected frame)"""
    import iac_amd as A
    want = GOLD[variant][str(seed)]
    stream, c = F.build(seed, variant)

    def run():
        PU._reset(A)
        rc, outs = group_decode_all(lib, dict(c), stream, 4, 2, starve=lambda r, i: False)
        assert rc == 0, (variant, seed, rc)
        return outs, PU._tallies(A)[0]

    outs, fam = run()
    row = next(iter(_family_rows(c, frames)))
    assert set(fam) == {row} and fam[row] >= len(frames), (variant, seed, fam)
    for i, (pcm, rets) in enumerate(outs):
        assert [int(r) for r in rets] == want["rets"], (variant, seed, i)
        assert F.digest(pcm) == want["sha256"], (variant, seed, i, "the PCM hash of the real reference")
    with R.environment(UNFUSED):
        twins, fam = run()
    assert fam == {}, (variant, seed, fam)
    for i, ((pcm, _), (twin, _)) in enumerate(zip(outs, twins)):
        assert np.array_equal(pcm, twin), (variant, seed, i, "byte-equal with IAMF_HIP_PACKETS_RAGGED_UNFUSED=1")
