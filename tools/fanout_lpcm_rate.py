#!/usr/bin/env python3
"""One element held as LPCM packets into K renditions: iamf_hip_batch_render_fanout_lpcm (the packets read once) against K
iamf_hip_batch_render_lpcm calls on twin batches (the packets read K times), in ONE process, alternating, through the same
library.  The protocol is tools/fanout_rate.py's.

Geometry: bench.py's — S streams x 64 frames x 1024 samples, 3rd-order ambisonics element resident in HBM as 16-bit
little-endian packet rows, the hot programme (tests/synth.py) quantised to 16 bit — for S = 512, 2048 and 4096 (at 4096
the single LPCM call switches to its late-prefetch variant).  K = 2 {Sound System A, mono} s16, 3 {+ A with other gains},
4 {+ mono s24}.  A step = one call over all frames on fresh state: the batches are reset before each step, outside the
timing, and EACH STEP is timed on its own by a pair of HIP events on the stream around it.  A region's figure is the mean of
its --steps step times; per series the median / min / max of --regions regions after one discarded region.  Series:
  x  = the packet fan-out call
  y  = K single iamf_hip_batch_render_lpcm calls on twin batches
  y2 = y again (the spread y against y2 is what a ratio has to clear)
  z  = the f32 fan-out (iamf_hip_batch_render_fanout) on the element unpacked beforehand — informational: its unpack pass
       is not in the figure
Before the timing the PCM of x and y at the timed geometry is compared by SHA-256 ("verified").

Prints ONE JSON line.  usage: python tools/fanout_lpcm_rate.py [--streams 512,2048,4096] [--frames 64] [--steps 10] [--regions 5]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12   # MI355X peak


def members(A, k):
    a16 = dict(layout="A", fmt=A.FMT_S16, gains=None)
    m16 = dict(layout="MONO", fmt=A.FMT_S16, gains=None)
    a16g = dict(layout="A", fmt=A.FMT_S16, gains=(0.9, 1.1))
    m24 = dict(layout="MONO", fmt=A.FMT_S24, gains=None)
    return {2: [a16, m16], 3: [a16, a16g, m16], 4: [a16, a16g, m16, m24]}[k]


def make(A, sp, S, fs):
    oc = A.layout_channels(A.SS[sp["layout"]])
    b = A.Batch(S, A.get_h2m_matrix(3, A.SS[sp["layout"]]), oc, frame_size=fs, out_format=sp["fmt"])
    if sp["gains"]:
        b.set_gains(element=[sp["gains"][0]] * S, output=[sp["gains"][1]] * S)
    b.out_bytes = oc * {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4}[sp["fmt"]]
    return b


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_k(A, torch, d_raw, L, row, xin, S, F, fs, k, steps, regions):
    m = 16
    specs = members(A, k)
    fan = [make(A, sp, S, fs) for sp in specs]
    twin = [make(A, sp, S, fs) for sp in specs]
    f32 = [make(A, sp, S, fs) for sp in specs]
    caps = [F * fs * b.out_bytes for b in fan]
    pcm_x = [torch.zeros((S, c), dtype=torch.uint8, device="cuda") for c in caps]
    pcm_y = [torch.zeros((S, c), dtype=torch.uint8, device="cuda") for c in caps]
    st = torch.cuda.current_stream().cuda_stream
    inp = A.LpcmInput()
    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.first_sample, inp.layout = d_raw.data_ptr(), F * row, row, 0, L
    reports = []

    def step_x():
        _, rep = A.render_fanout_lpcm(fan, inp, F, [p.data_ptr() for p in pcm_x], caps, st)
        reports.append(rep)

    def step_y():
        for b, p, c in zip(twin, pcm_y, caps):
            a = A.RenderArgs()
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = F, p.data_ptr(), c, st
            b.render_lpcm(inp, a)

    def step_z():   # (into the buffers of y: their content is not looked at after the verification)
        A.render_fanout(f32, xin.data_ptr(), F * m * fs, m * fs, F, [p.data_ptr() for p in pcm_y], caps, st)

    def region(step, batches):
        ms = 0.0
        for _ in range(steps):   # every step starts from fresh state: the same work each time (the reset is not timed)
            for b in batches:
                b.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        return ms / steps

    # warm-up and verification at the timed geometry
    step_x()
    step_y()
    torch.cuda.synchronize()
    verified = all(sha(a) == sha(b) for a, b in zip(pcm_x, pcm_y))
    A.route_reset()
    step_y()
    torch.cuda.synchronize()
    single_routes = sorted("%s_v%d_m%d_c%d" % (r[0], r[1], r[2], r[3]) for r in A.route_tally())
    step_z()
    torch.cuda.synchronize()
    series = {"x": [], "y": [], "y2": [], "z": []}
    for r in range(regions + 1):
        tx = region(step_x, fan)
        ty = region(step_y, twin)
        ty2 = region(step_y, twin)
        tz = region(step_z, f32)
        if r:   # the first region is discarded
            series["x"].append(tx)
            series["y"].append(ty)
            series["y2"].append(ty2)
            series["z"].append(tz)
    for b in fan + twin + f32:
        b.close()
    med = {n: float(np.median(v)) for n, v in series.items()}
    frames = S * F * fs
    out_bytes = sum(b.out_bytes for b in fan)
    shared_b, single_b, f32_b = 2 * m + out_bytes, 2 * m * k + out_bytes, 4 * m + out_bytes

    def stats(v):
        return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))

    return dict(members=[sp["layout"] + ("_s24" if sp["fmt"] == A.FMT_S24 else "_s16") + ("_gains" if sp["gains"] else "") for sp in specs],
                report=sorted(set(reports)), verified=verified, single_routes=single_routes,
                fanout_lpcm=stats(series["x"]), singles=stats(series["y"]), singles_again=stats(series["y2"]),
                f32_fanout_unpacked_beforehand=stats(series["z"]),
                ratio_singles_over_fanout_lpcm=round(med["y"] / med["x"], 4),
                spread_singles_vs_singles=round(abs(med["y"] / med["y2"] - 1.0), 4),
                ratio_f32_fanout_over_fanout_lpcm=round(med["z"] / med["x"], 4),
                fanout_lpcm_gsample_frames_s=round(frames / med["x"] / 1e6, 2), singles_gsample_frames_s=round(frames / med["y"] / 1e6, 2),
                fanout_lpcm_bytes_per_frame=shared_b, singles_bytes_per_frame=single_b, f32_fanout_bytes_per_frame=f32_b,
                fanout_lpcm_share_of_8TBs=round(frames * shared_b / (med["x"] * 1e-3) / HBM_BYTES_PER_S, 4),
                singles_share_of_8TBs=round(frames * single_b / (med["y"] * 1e-3) / HBM_BYTES_PER_S, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--k", default="2,3,4")
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import lpcm_util as LP
    import synth
    assert torch.cuda.is_available()
    # hot programme, quantised to 16 bit: 16 seeded streams, tiled over the batch (the limiter's work per stream is what
    # matters, not that every stream differs)
    basis = np.stack([synth.hot(4242 + i, 16, a.frames * a.fs) for i in range(16)])
    ints = np.clip(np.rint(basis.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64)
    ints = np.ascontiguousarray(ints.reshape(16, 16, a.frames, a.fs).transpose(0, 2, 1, 3))        # [16][F][ch][fs]
    raw, L, row = LP.rows(ints, 2, True, [1] * 16, list(range(16)), head=16, pad=0, frame_size=a.fs)
    fr = (ints.astype(np.float32) / np.float32(32768.0))                                            # what the unpacker writes
    res = {}
    for S in (int(v) for v in a.streams.split(",")):
        reps = (S + 15) // 16
        d_raw = torch.from_numpy(raw).cuda().repeat(reps, 1, 1)[:S].contiguous()
        xin = torch.from_numpy(fr).cuda().repeat(reps, 1, 1, 1)[:S].contiguous()
        for k in (int(v) for v in a.k.split(",")):
            res["%d_streams_k%d" % (S, k)] = run_k(A, torch, d_raw, L, row, xin, S, a.frames, a.fs, k, a.steps, a.regions)
        del d_raw, xin
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "fanout_lpcm_rate", "workload": "TOA element as 16-bit LPCM packets -> K renditions, %d frames of %d "
                      "samples per stream, packets resident in HBM, hot programme quantised to 16 bit; one packet fan-out call "
                      "against K single LPCM calls on twin batches" % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
