#!/usr/bin/env python3
"""One element into K renditions: iamf_hip_batch_render_fanout (the input read once) against K iamf_hip_batch_render calls
on twin batches (the input read K times), in ONE process, alternating, through the same library.

Geometry: bench.py's — S streams x 64 frames x 1024 samples, 3rd-order ambisonics element resident in HBM, hot programme
(tests/synth.py) — for S = 512 and 2048.  K = 2 {Sound System A, mono} s16, 3 {+ A with other gains}, 4 {+ mono s24}.  A
step = one call over all frames on fresh state, so that every step is the same work: the batches are reset before each
step, outside the timing, and EACH STEP is timed on its own by a pair of HIP events on the stream around it (recorded,
then waited for).  A region's figure is the mean of its --steps step times; per series the median / min / max of
--regions regions after one discarded region.  (bench.py instead brackets a region of back-to-back steps on continuing
state; here a step is one launch of 0.5 ms or more, or K of them queued back to back, and both sides are timed alike.)  Series:
x = the fan-out call, y = K single calls, y2 = the K single calls again (the spread y against y2 is what a ratio has to
clear).  Before the timing the PCM of x and y at the timed geometry is compared by SHA-256 ("verified").

Prints ONE JSON line.  usage: python tools/fanout_rate.py [--streams 512,2048] [--frames 64] [--steps 10] [--regions 5]"""
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


def run_k(A, torch, xin, S, F, fs, k, steps, regions):
    m = 16
    specs = members(A, k)
    fan = [make(A, sp, S, fs) for sp in specs]
    twin = [make(A, sp, S, fs) for sp in specs]
    caps = [F * fs * b.out_bytes for b in fan]
    pcm_x = [torch.zeros((S, c), dtype=torch.uint8, device="cuda") for c in caps]
    pcm_y = [torch.zeros((S, c), dtype=torch.uint8, device="cuda") for c in caps]
    st = torch.cuda.current_stream().cuda_stream
    ss, fstr = F * m * fs, m * fs
    fused = []

    def step_x():
        _, nf = A.render_fanout(fan, xin.data_ptr(), ss, fstr, F, [p.data_ptr() for p in pcm_x], caps, st)
        fused.append(nf)

    def step_y():
        for b, p, c in zip(twin, pcm_y, caps):
            b.render(xin.data_ptr(), ss, fstr, F, p.data_ptr(), c, st)

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
    series = {"x": [], "y": [], "y2": []}
    for r in range(regions + 1):
        tx = region(step_x, fan)
        ty = region(step_y, twin)
        ty2 = region(step_y, twin)
        if r:   # the first region is discarded
            series["x"].append(tx)
            series["y"].append(ty)
            series["y2"].append(ty2)
    for b in fan + twin:
        b.close()
    med = {n: float(np.median(v)) for n, v in series.items()}
    frames = S * F * fs
    out_bytes = sum(b.out_bytes for b in fan)
    shared_b, single_b = 4 * m + out_bytes, 4 * m * k + out_bytes

    def stats(v):
        return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))

    return dict(members=[sp["layout"] + ("_s24" if sp["fmt"] == A.FMT_S24 else "_s16") + ("_gains" if sp["gains"] else "") for sp in specs],
                n_fused=sorted(set(fused)), verified=verified,
                fanout=stats(series["x"]), singles=stats(series["y"]), singles_again=stats(series["y2"]),
                ratio_singles_over_fanout=round(med["y"] / med["x"], 4),
                spread_singles_vs_singles=round(abs(med["y"] / med["y2"] - 1.0), 4),
                fanout_gsample_frames_s=round(frames / med["x"] / 1e6, 2), singles_gsample_frames_s=round(frames / med["y"] / 1e6, 2),
                fanout_bytes_per_frame=shared_b, singles_bytes_per_frame=single_b,
                fanout_share_of_8TBs=round(frames * shared_b / (med["x"] * 1e-3) / HBM_BYTES_PER_S, 4),
                singles_share_of_8TBs=round(frames * single_b / (med["y"] * 1e-3) / HBM_BYTES_PER_S, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--k", default="2,3,4")
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import synth
    assert torch.cuda.is_available()
    res = {}
    for S in (int(v) for v in a.streams.split(",")):
        # hot programme: 16 seeded streams, tiled over the batch (the limiter's work per stream is what matters, not that
        # every stream differs)
        basis = np.stack([synth.hot(4242 + i, 16, a.frames * a.fs) for i in range(16)])
        fr = np.ascontiguousarray(basis.reshape(16, 16, a.frames, a.fs).transpose(0, 2, 1, 3))
        xin = torch.from_numpy(fr).cuda().repeat((S + 15) // 16, 1, 1, 1)[:S].contiguous()
        for k in (int(v) for v in a.k.split(",")):
            res["%d_streams_k%d" % (S, k)] = run_k(A, torch, xin, S, a.frames, a.fs, k, a.steps, a.regions)
        del xin
    print(json.dumps({"tool": "fanout_rate", "workload": "TOA element -> K renditions, %d frames of %d samples per stream, element "
                      "resident in HBM, hot programme; one fan-out call against K single calls on twin batches" % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
