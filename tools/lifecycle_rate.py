#!/usr/bin/env python3
"""What a stream's start, end and move cost on the batch ABI: iamf_hip_batch_restart_range and _export_range /
_import_range against the whole-batch iamf_hip_batch_reset, in ONE process through the same library.

Geometry: the headline batch — S = 512 streams, 3rd-order ambisonics -> binaural, s16, 64 frames x 1024 samples per call,
hot programme (tests/synth.py), element resident in HBM.  Timed as tools/fanout_rate.py times: a pair of HIP events on
the stream around each step (recorded, then waited for), a region = the mean of --steps steps, per series the median / min
/ max of --regions regions after one discarded region.  Host times are time.perf_counter around the call alone.

  (a) a new programme in ONE slot.  The parent's way: iamf_hip_batch_reset — which waits for the whole device and wipes the
      other S - 1 streams as well — against restart_range(s, 1, gains).  Each with the device idle and behind a queued
      64-frame render (the case of a live service: the reset's device-wide wait then drains that render on the host).
  (b) export + import of 64 streams into a second batch: device time, bytes moved against the state's size.
  (c) the headline call with 64 one-stream restarts queued in front of it against the same call with none (x; y; y again:
      the spread y against y2 is what a difference has to clear).  Every step starts from fresh state (reset, untimed) so
      that the whole batch stands at one position.

Prints ONE JSON line.  usage: python tools/lifecycle_rate.py [--streams 512] [--frames 64] [--steps 10] [--regions 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v, scale=1.0, nd=3):
    v = [x * scale for x in v]
    return dict(min=round(min(v), nd), median=round(float(np.median(v)), nd), max=round(max(v), nd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--moved", type=int, default=64)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import synth
    assert torch.cuda.is_available()
    S, F, fs, m = a.streams, a.frames, a.fs, 16
    basis = np.stack([synth.hot(4242 + i, m, F * fs) for i in range(16)])
    fr = np.ascontiguousarray(basis.reshape(16, m, F, fs).transpose(0, 2, 1, 3))
    xin = torch.from_numpy(fr).cuda().repeat((S + 15) // 16, 1, 1, 1)[:S].contiguous()
    mx = A.get_h2m_matrix(3, A.SS["BINAURAL"])
    b, b2 = A.Batch(S, mx, 2, frame_size=fs), A.Batch(S, mx, 2, frame_size=fs)
    cap = F * fs * 2 * 2
    pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    one = A.stream_gains(element=[0.9], output=[1.1], loudness=[1.0])

    def render(batch=b):
        batch.render(xin.data_ptr(), F * m * fs, m * fs, F, pcm.data_ptr(), cap, st)

    def timed(call, before=None):
        """(host seconds of the call alone, device ms between the events around it)"""
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return host, e0.elapsed_time(e1)

    def series(call, before=None, after=None):
        host, dev = [], []
        for r in range(a.regions + 1):
            hs = ds = 0.0
            for _ in range(a.steps):
                h, d = timed(call, before)
                hs += h
                ds += d
                if after:
                    after()
                torch.cuda.synchronize()
            if r:   # the first region is discarded
                host.append(hs / a.steps)
                dev.append(ds / a.steps)
        return dict(host_us=stats(host, 1e6), device_us=stats(dev, 1e3))

    render()
    torch.cuda.synchronize()
    res = {}
    # ---- (a) one slot, the parent's way and the new one ----
    slot = S // 2
    res["a_reset_idle"] = series(b.reset)
    res["a_reset_behind_render"] = series(b.reset, before=render)
    res["a_restart_one_idle"] = series(lambda: b.restart_range(slot, 1, one, st))
    # the restarted slot leaves the batch's common position: put it back (untimed) for the next step's render
    res["a_restart_one_behind_render"] = series(lambda: b.restart_range(slot, 1, one, st), before=render, after=b.reset)
    res["a_note"] = "reset also wipes the other %d streams of the batch; restart_range leaves them running" % (S - 1)
    # ---- (b) export + import of `moved` streams ----
    nbytes = b.stream_state_bytes()
    blob = torch.zeros((a.moved, nbytes), dtype=torch.uint8, device="cuda")
    b.reset()
    render()

    def move():
        t = b.export_range(0, a.moved, blob.data_ptr(), nbytes, st)
        b2.import_range(0, a.moved, blob.data_ptr(), nbytes, t, st)

    r = series(move)
    moved = 4 * a.moved * nbytes   # export reads the state and writes the blob, import reads the blob and writes the state
    r.update(streams=a.moved, state_bytes_per_stream=nbytes, bytes_moved=moved,
             gbytes_per_s=round(moved / (r["device_us"]["median"] * 1e-6) / 1e9, 2))
    res["b_export_import"] = r
    # ---- (c) the headline call with and without restarts in front of it ----
    every = max(S // 64, 1)

    def with_restarts():
        for s in range(0, S, every):
            b.restart_range(s, 1, one, st)
        render()

    x, y, y2 = (series(with_restarts, before=b.reset), series(render, before=b.reset), series(render, before=b.reset))
    frames = S * F * fs
    mx_, my, my2 = (v["device_us"]["median"] for v in (x, y, y2))
    res["c_render_with_restarts"] = dict(restarts_per_call=len(range(0, S, every)), with_restarts=x, without=y, without_again=y2,
                                         gsample_frames_s_with=round(frames / mx_ / 1e3, 2),
                                         gsample_frames_s_without=round(frames / my / 1e3, 2),
                                         ratio_with_over_without=round(mx_ / my, 4),
                                         spread_without_vs_without=round(abs(my / my2 - 1.0), 4),
                                         added_us_per_restart=round((mx_ - my) / len(range(0, S, every)), 3))
    b.close()
    b2.close()
    print(json.dumps({"tool": "lifecycle_rate", "workload": "TOA -> binaural s16, %d streams, %d frames of %d samples per call, hot "
                      "programme, element resident in HBM" % (S, F, fs), "gpu": torch.cuda.get_device_name(0),
                      "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
