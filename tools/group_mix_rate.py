#!/usr/bin/env python3
"""Decoder-group rates through the reference's API for a TWO-element stream, the packet path against the unpacked one: a
variant of tools/group_rate.py (its loop, its phases, its modes).

The stream: a 3rd-order mono-coded ambisonics bed plus a coupled stereo element, 16-bit LPCM, frames of --fs samples (1000: every
frame is one launch of the ragged two-element packet form, iamf_hip_batch_render_packets_mix_ragged; 1024: of the whole-block
mix kernel), into stereo.  Every handle decodes it from the start.  Each group size runs with the environment as it is — the
group hands both elements' packets to the render kernel — and with IAMF_HIP_GROUP_UNPACK=1 — two unpack passes, then the f32
kernels: what a two-element group ran before —, alternating, each figure the best of --repeat runs.  Host OBU parsing, the
packet uploads, the renders and the PCM back over PCIe are all inside the time.  Prints ONE JSON line.

usage: python tools/group_mix_rate.py [--fs 1000] [--frames 192] [--sizes 64,256] [--repeat 3]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import group_rate as GR  # noqa: E402

STEREO = 1   # IAChannelLayoutType of a stereo element; sound system A (0) is the stereo output layout


def make_stream(fs, frames):
    import iamf_writer as W
    import synth
    in_ch = 16
    x = W.quantize(np.clip(synth.hot(4242, in_ch, frames * fs), -1, 1 - 2 ** -15).astype(np.float32), 16)
    x2 = W.quantize(np.clip(0.25 * synth.hot(4343, 2, frames * fs), -1, 1 - 2 ** -15).astype(np.float32), 16)
    pd = lambda pid: W.param_definition(pid, 48000, mode=1)
    s = W.sequence_header(1) + W.codec_config_lpcm(0, fs, 16, 48000)
    s += W.audio_element_ambisonics_mono(1, 0, in_ch, list(range(in_ch)))
    s += W.audio_element_channel(2, 0, STEREO, [in_ch])
    s += W.mix_presentation(1, [dict(eid=1, pdef=pd(100), default_q78=0), dict(eid=2, pdef=pd(102), default_q78=0)],
                            dict(pdef=pd(101), default_q78=0), [("ss", 0)])
    for f in range(frames):
        s += W.temporal_delimiter()
        subs = [(i, W.lpcm_bytes(x[i:i + 1, f * fs:(f + 1) * fs], 16)) for i in range(in_ch)]
        s += W.audio_frames(subs + W.channel_element_substreams(STEREO, x2[:, f * fs:(f + 1) * fs], in_ch, 16))
    return s


class _Stereo:
    """the decoder library with tools/group_rate.py's binaural layout call turned into "sound system A" """

    def __init__(self, L):
        self._L = L
        L.IAMF_decoder_output_layout_set_sound_system.argtypes = [C.c_void_p, C.c_int]

    def __getattr__(self, name):
        if name == "IAMF_decoder_output_layout_set_binaural":
            return lambda d: self._L.IAMF_decoder_output_layout_set_sound_system(d, 0)
        return getattr(self._L, name)


def tallies(A):
    out = {}
    for f in ("PACKETS_MIX_RAGGED", "LPCM_MIX", "LPCM24_MIX"):
        out.update({"%s_v%d_m%d_c%d_k%d" % k: v for k, v in A.route_family_tally(f, reset=True).items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    assert torch.cuda.is_available()
    L = _Stereo(GR.lib())
    stream = make_stream(a.fs, a.frames)
    os.environ.pop("IAMF_HIP_GROUP_UNPACK", None)

    def once(n, pipelined, unpack):
        if unpack:
            os.environ["IAMF_HIP_GROUP_UNPACK"] = "1"
        try:
            return GR.run(L, stream, n, pipelined)
        finally:
            os.environ.pop("IAMF_HIP_GROUP_UNPACK", None)

    routes = {}
    for unpack in (False, True):     # code objects loaded outside the timing; which kernels a round runs
        tallies(A)
        once(8, False, unpack)
        once(8, True, unpack)
        routes["unpack" if unpack else "packets"] = tallies(A)
    res = {}
    for n in (int(v) for v in a.sizes.split(",")):
        for mode in ("sync", "pipelined"):
            best = {"packets": None, "unpack": None}
            for _ in range(a.repeat):
                for name in ("packets", "unpack"):
                    r = once(n, mode == "pipelined", name == "unpack")
                    if best[name] is None or r["msamples_s"] > best[name]["msamples_s"]:
                        best[name] = r
            res["%d_%s" % (n, mode)] = dict(best, ratio=round(best["packets"]["msamples_s"] / best["unpack"]["msamples_s"], 3))
    print(json.dumps({"tool": "group_mix_rate", "workload": "TOA + coupled stereo -> stereo, 16-bit LPCM .iamf, %d frames of %d samples per handle, "
                      "through the reference's API (PCIe and host parsing included); the group's packet path against IAMF_HIP_GROUP_UNPACK=1"
                      % (a.frames, a.fs), "gpu": torch.cuda.get_device_name(0), "mix_family_launches_in_the_warm_up": routes, "results": res}))


if __name__ == "__main__":
    main()
