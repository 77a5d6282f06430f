#!/usr/bin/env python3
"""Decoder-group rates through the reference's API for a RATE-CONVERTING stream, the packet path against the unpacked one: a
variant of tools/group_rate.py (its loop, its phases, its modes), after tools/group_mix_rate.py.

The stream: a 3rd-order mono-coded ambisonics element, 16-bit LPCM at 44.1 kHz, frames of --fs samples, into stereo at the
reference's default output rate of 48 kHz: render -> resampler -> limiter.  Every handle decodes it from the start.  Each group
size runs with the environment as it is — the first stage reads the packets (iamf_hip_batch_render_packets_nolim), the last
stage is the interleaved form of the fast kernel (iamf_hip_batch_render_interleaved) — and with IAMF_HIP_GROUP_UNPACK=1
IAMF_HIP_INTERLEAVED_UNFUSED=1 — unpack, the f32 limiter-less kernel, the resampler, the general kernel: what such a group ran
before —, alternating, --repeat runs each: the best, and every run's figure with the spread (max / min - 1) per side.  Round by
round (sync) and with two rounds in flight (pipelined).  Host OBU parsing, the packet uploads, the three stages and the PCM back
over PCIe are all inside the time.  Prints ONE JSON line.

usage: python tools/group_resample_rate.py [--fs 1024] [--frames 192] [--sizes 64,256] [--repeat 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import group_mix_rate as GM  # noqa: E402
import group_rate as GR  # noqa: E402

OFF = ("IAMF_HIP_GROUP_UNPACK", "IAMF_HIP_INTERLEAVED_UNFUSED")
RATE = 44100


def make_stream(fs, frames):
    import iamf_writer as W
    import synth
    in_ch = 16
    x = W.quantize(np.clip(synth.hot(4242, in_ch, frames * fs), -1, 1 - 2 ** -15).astype(np.float32), 16)
    pd = lambda pid: W.param_definition(pid, RATE, mode=1)
    s = W.sequence_header(1) + W.codec_config_lpcm(0, fs, 16, RATE)
    s += W.audio_element_ambisonics_mono(1, 0, in_ch, list(range(in_ch)))
    s += W.mix_presentation(1, [dict(eid=1, pdef=pd(100), default_q78=0)], dict(pdef=pd(101), default_q78=0), [("ss", 0)])
    for f in range(frames):
        s += W.temporal_delimiter()
        s += W.audio_frames([(i, W.lpcm_bytes(x[i:i + 1, f * fs:(f + 1) * fs], 16)) for i in range(in_ch)])
    return s


def tallies(A):
    out = {}
    for f in ("NOLIM_PACKETS", "FAST_INTERLEAVED"):
        out.update({"%s_v%d_m%d_c%d_k%d" % k: v for k, v in A.route_family_tally(f, reset=True).items()})
    out.update({"%s_v%d_m%d_c%d_k%d" % k: v for k, v in A.route_tally().items() if k[0] in ("NOLIM", "GENERIC")})
    A.route_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    assert torch.cuda.is_available()
    L = GM._Stereo(GR.lib())
    stream = make_stream(a.fs, a.frames)
    for k in OFF:
        os.environ.pop(k, None)

    def once(n, pipelined, unpack):
        if unpack:
            for k in OFF:
                os.environ[k] = "1"
        try:
            return GR.run(L, stream, n, pipelined)
        finally:
            for k in OFF:
                os.environ.pop(k, None)

    routes = {}
    for unpack in (False, True):     # code objects loaded outside the timing; which kernels a round runs
        tallies(A)
        once(8, False, unpack)
        once(8, True, unpack)
        routes["unpack" if unpack else "packets"] = tallies(A)
    res = {}
    for n in (int(v) for v in a.sizes.split(",")):
        for mode in ("sync", "pipelined"):
            runs = {"packets": [], "unpack": []}
            for _ in range(a.repeat):
                for name in ("packets", "unpack"):
                    runs[name].append(once(n, mode == "pipelined", name == "unpack"))
            best = {name: max(v, key=lambda r: r["msamples_s"]) for name, v in runs.items()}
            every = {name: [r["msamples_s"] for r in v] for name, v in runs.items()}
            spread = {name: round(max(v) / min(v) - 1.0, 4) for name, v in every.items()}
            res["%d_%s" % (n, mode)] = dict(best, msamples_s_every_run=every, spread_max_over_min=spread,
                                            ratio=round(best["packets"]["msamples_s"] / best["unpack"]["msamples_s"], 3),
                                            ratio_of_medians=round(float(np.median(every["packets"]) / np.median(every["unpack"])), 3))
    print(json.dumps({"tool": "group_resample_rate", "workload": "TOA 16-bit LPCM at 44.1 kHz -> stereo at 48 kHz, %d frames of %d samples per handle, "
                      "through the reference's API (PCIe and host parsing included; output sample-frames counted); the group's packet path against "
                      "IAMF_HIP_GROUP_UNPACK=1 IAMF_HIP_INTERLEAVED_UNFUSED=1" % (a.frames, a.fs), "gpu": torch.cuda.get_device_name(0),
                      "launches_in_the_warm_up": routes, "results": res}))


if __name__ == "__main__":
    main()
