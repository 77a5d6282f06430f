#!/usr/bin/env python3
"""24-bit LPCM packets into the headline kernel: one fused iamf_hip_batch_render_lpcm call (render_fast_kernel<.., LP,
EARLY, LPB = 3> reads the packets itself) against the same call with IAMF_HIP_LPCM_UNFUSED=1 (iamf_hip_lpcm_unpack, then the
f32 kernel: what every 24-bit call ran before the form existed), in ONE process, alternating, through the same library.
The protocol is tools/fanout_rate.py's.

Geometry: bench.py's — S streams x 64 frames x 1024 samples, 3rd-order ambisonics element -> Sound System A, s16 — the
element resident in HBM as 24-bit little-endian packet rows, the hot programme (tests/synth.py) quantised to 24 bit, for
S = 512, 2048 and 4096.  A step = one call over all frames on fresh state: the batch is reset before each step, outside the
timing, and EACH STEP is timed on its own by a pair of HIP events on the stream around it.  A region's figure is the mean of
its --steps step times; per series the median / min / max of --regions regions after one discarded region.  Series:
  x_early, x_late = the fused call with the prefetch variant forced (IAMF_HIP_LP_EARLY / IAMF_HIP_LP_LATE)
  y               = the call with IAMF_HIP_LPCM_UNFUSED=1
  y2              = y again (the spread y against y2 is what a ratio has to clear)
Before the timing the PCM of x (both variants) and y at the timed geometry is compared by SHA-256 ("verified"), and the
route tables say which kernels ran.

What the host does with the figures (iac_amd/csrc/render_route.hpp): a size at which y / x does not exceed 1 by more than
that run's y-against-y2 spread is not fused (lpcm24_fused); the prefetch variant is the faster one per size (lpcm24_early).

Prints ONE JSON line.  usage: python tools/lpcm24_rate.py [--streams 512,2048,4096] [--frames 64] [--steps 10] [--regions 5]"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12   # MI355X peak
SWITCHES = ("IAMF_HIP_LP_EARLY", "IAMF_HIP_LP_LATE", "IAMF_HIP_LPCM_UNFUSED")


@contextlib.contextmanager
def switch(name):
    """exactly one of SWITCHES set (the library reads them at every call)"""
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ[name] = "1"
    try:
        yield
    finally:
        os.environ.pop(name, None)


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run(A, torch, d_raw, L, row, S, F, fs, steps, regions):
    m, oc = 16, 2
    b = A.Batch(S, A.get_h2m_matrix(3, A.SS["A"]), oc, frame_size=fs, out_format=A.FMT_S16)
    cap = F * fs * oc * 2
    pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    inp = A.LpcmInput()
    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.first_sample, inp.layout = d_raw.data_ptr(), F * row, row, 0, L
    a = A.RenderArgs()
    a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = F, pcm.data_ptr(), cap, st
    names = {"x_early": "IAMF_HIP_LP_EARLY", "x_late": "IAMF_HIP_LP_LATE", "y": "IAMF_HIP_LPCM_UNFUSED", "y2": "IAMF_HIP_LPCM_UNFUSED"}

    def step(series):
        with switch(names[series]):
            b.render_lpcm(inp, a)

    def region(series):
        ms = 0.0
        for _ in range(steps):   # every step starts from fresh state: the same work each time (the reset is not timed)
            b.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(series)
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        return ms / steps

    # warm-up, verification and routes at the timed geometry
    hashes, routes = {}, {}
    for series in ("x_early", "x_late", "y"):
        b.reset()
        pcm.zero_()
        A.route_reset()
        A.route_table_tally(2, reset=True)
        step(series)
        torch.cuda.synchronize()
        hashes[series] = sha(pcm)
        routes[series] = sorted("%s_v%d_m%d_c%d" % (r[0], r[1], r[2], r[3])
                                for r in list(A.route_table_tally(2, reset=True)) + list(A.route_tally()))
    verified = hashes["x_early"] == hashes["y"] and hashes["x_late"] == hashes["y"]
    out = {n: [] for n in names}
    for r in range(regions + 1):
        t = {n: region(n) for n in ("x_early", "y", "x_late", "y2")}
        if r:   # the first region is discarded
            for n in names:
                out[n].append(t[n])
    b.close()
    med = {n: float(np.median(v)) for n, v in out.items()}
    frames = S * F * fs
    fused_b, unfused_b = 3 * m + oc * 2, (3 * m + 4 * m) + (4 * m + oc * 2)   # 52 and 180 for a 3rd-order element into stereo s16
    best = "x_early" if med["x_early"] <= med["x_late"] else "x_late"
    spread = abs(med["y"] / med["y2"] - 1.0)

    def stats(v):
        return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))

    return dict(verified=verified, sha256_fused_early=hashes["x_early"], sha256_fused_late=hashes["x_late"], sha256_unfused=hashes["y"],
                routes=routes, fused_early=stats(out["x_early"]), fused_late=stats(out["x_late"]), unfused=stats(out["y"]),
                unfused_again=stats(out["y2"]), faster_variant=best[2:],
                ratio_unfused_over_fused_early=round(med["y"] / med["x_early"], 4),
                ratio_unfused_over_fused_late=round(med["y"] / med["x_late"], 4),
                ratio_unfused_over_fused=round(med["y"] / med[best], 4), spread_unfused_vs_unfused=round(spread, 4),
                fuse=bool(med["y"] / med[best] - 1.0 > spread),
                fused_gsample_frames_s=round(frames / med[best] / 1e6, 2), unfused_gsample_frames_s=round(frames / med["y"] / 1e6, 2),
                fused_bytes_per_frame=fused_b, unfused_bytes_per_frame=unfused_b,
                fused_share_of_8TBs=round(frames * fused_b / (med[best] * 1e-3) / HBM_BYTES_PER_S, 4),
                unfused_share_of_8TBs=round(frames * unfused_b / (med["y"] * 1e-3) / HBM_BYTES_PER_S, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import lpcm_util as LP
    import synth
    assert torch.cuda.is_available()
    # hot programme, quantised to 24 bit: 16 seeded streams, tiled over the batch (the limiter's work per stream is what
    # matters, not that every stream differs)
    basis = np.stack([synth.hot(4242 + i, 16, a.frames * a.fs) for i in range(16)])
    ints = np.clip(np.rint(basis.astype(np.float64) * 8388608.0), -8388608, 8388607).astype(np.int64)
    ints = np.ascontiguousarray(ints.reshape(16, 16, a.frames, a.fs).transpose(0, 2, 1, 3))        # [16][F][ch][fs]
    raw, L, row = LP.rows(ints, 3, True, [1] * 16, list(range(16)), head=16, pad=0, frame_size=a.fs)
    res = {}
    for S in (int(v) for v in a.streams.split(",")):
        reps = (S + 15) // 16
        d_raw = torch.from_numpy(raw).cuda().repeat(reps, 1, 1)[:S].contiguous()
        res["%d_streams" % S] = run(A, torch, d_raw, L, row, S, a.frames, a.fs, a.steps, a.regions)
        del d_raw
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "lpcm24_rate", "workload": "TOA element as 24-bit little-endian LPCM packets -> Sound System A s16, "
                      "%d frames of %d samples per stream, packets resident in HBM, hot programme quantised to 24 bit; one fused "
                      "call against the same call unfused (unpack, then the f32 kernel)" % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
