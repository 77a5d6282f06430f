#!/usr/bin/env python3
"""Interleaved f32 of any call length: iamf_hip_batch_render_interleaved (render_fast_kernel<.., IL, RAG>) against what the
call ran before — iamf_hip_batch_render_range on a twin frame_size == 1 batch, the general kernel, the parent commit's path
(its kernel is unchanged: tools/kernel_hashes.py) — in ONE process, the two alternating.  The protocol is
tools/lpcm_mix_rate.py's.

    python tools/interleaved_rate.py > profiles/r12_interleaved_rate.json

Geometry: the limiter stage behind a rate converter — S streams of mono or stereo through the identity, s16 — in calls of
1115 sample-frames (what 44.1 -> 48 kHz hands out for 1024), 1024 and 64 x 1115, for S = 512, 2048 and 4096; the hot
programme (tests/synth.py) resident in HBM.  A step = 64 x 1115 (or 64 x 1024) sample-frames per stream on fresh state: 64
calls of the short lengths, one of the long, every call's PCM into a 16-byte aligned slot of its own; the batch is reset
before each step, outside the timing, and EACH STEP is timed by a pair of HIP events around it.  A region's figure is the
mean of its --steps step times; per series the median / min / max of --regions regions after one discarded region.  Series:
  x      = the new entry
  y, y2  = iamf_hip_batch_render_range on the twin batch, twice (the spread y against y2 is what a ratio has to clear)
Every series is verified in the same run: four streams of the PCM a step left against the oracle bit for bit (oracle_lib:
render, 0 + y, limiter_run over the calls, pack), every byte of every stream's PCM equal across the series (compared on the
device, again after every timed region), and the route listings say which kernels ran.

The chain: stereo 44.1 -> 48 kHz, 64 frames of 1024 per stream — render to f32 with the limiter off, iamf_hip_resampler_process,
the limiter stage — both ways, in input sample-frames per second, verified against the oracle's resampler + limiter.

What the host does with the figures (iac_amd/csrc/render_route.hpp): a size at which y / x does not exceed 1 by more than
that run's y-against-y2 spread is not fused (interleaved_fused).

Prints ONE JSON line.  usage: python tools/interleaved_rate.py [--streams 512,2048,4096] [--steps 10] [--regions 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = {"1115": (1115, 64), "1024": (1024, 64), "64x1115": (64 * 1115, 1)}     # name -> (sample-frames per call, calls per step)
FAM = "FAST_INTERLEAVED"


def r16(n):
    return (n + 15) & ~15


def stats(v):
    return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))


def timed(torch, fn, reset, steps):
    ms = 0.0
    for _ in range(steps):   # every step starts from fresh state: the same work each time (the reset is not timed)
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
    return ms / steps


def routes_now(A):
    return sorted("%s_v%d_m%d_c%d_k%d" % r for r in list(A.route_family_tally(FAM, reset=True)) + list(A.route_tally()))


def run(A, O, IU, torch, ch, S, n, calls, steps, regions):
    """calls of n sample-frames of ch channels through the identity into s16; the same n sample-frames of input every call"""
    import synth
    amx, omx = IU.identity_matrices(ch)
    basis = np.stack([synth.hot(6100 + i, ch, n) for i in range(16)])                         # [16][ch][n]
    ss = (n * ch + 3) & ~3       # the stream stride on the 16-byte grid
    h = np.zeros((16, ss), dtype=np.float32)
    h[:, :n * ch] = np.ascontiguousarray(basis.transpose(0, 2, 1)).reshape(16, n * ch)
    d_in = torch.from_numpy(h).cuda().repeat((S + 15) // 16, 1)[:S].contiguous()
    slot = r16(n * ch * 2)
    pcm = torch.zeros((S, calls * slot), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    b = {k: A.Batch(S, amx, ch, frame_size=1, out_format=A.FMT_S16, projection=A.PROJ_EXACT) for k in ("x", "y")}
    emitted = []

    def step(series):
        del emitted[:]
        bb = b["x" if series == "x" else "y"]
        for k in range(calls):
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = d_in.data_ptr(), ss, ch
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n, pcm.data_ptr() + k * slot, calls * slot, st
            emitted.append(bb.render_interleaved(a) if series == "x" else bb.render_range(a, 0, S))

    def reset(series):
        b["x" if series == "x" else "y"].reset()

    def gathered(rows):
        return [np.concatenate([rows[i, k * slot:k * slot + e * ch * 2] for k, e in enumerate(emitted)]) for i in range(rows.shape[0])]

    ids = sorted({0, S // 3, (2 * S) // 3, S - 1})
    want = {}
    for s in ids:
        x = np.tile(basis[s % 16], (1, calls))
        z = np.ascontiguousarray(np.zeros_like(x) + O.render(omx, x, ch), dtype=np.float32)
        z, _ = O.limiter_run(z, [n] * calls, flush=False)
        want[s] = O.pack(z, 16)
    snap, routes, oracle_ok = {}, {}, {}
    for series in ("x", "y"):
        reset(series)
        pcm.zero_()
        A.route_reset()
        A.route_family_tally(FAM, reset=True)
        step(series)
        torch.cuda.synchronize()
        snap[series] = pcm.clone()
        g = gathered(pcm[ids].cpu().numpy())
        oracle_ok[series] = all(np.array_equal(g[i].view(np.int16).reshape(-1, ch), want[s]) for i, s in enumerate(ids))
        routes[series] = routes_now(A)
    verified = all(oracle_ok.values()) and torch.equal(snap["x"], snap["y"])
    ref = snap.pop("y")
    snap.clear()
    verified = verified and routes["x"] == ["%s_v0_m%d_c%d_k0" % (FAM, ch, ch)] and routes["y"] == ["GENERIC_v0_m%d_c0_k0" % ch]
    out = {"x": [], "y": [], "y2": []}
    for r in range(regions + 1):
        t = {name: timed(torch, lambda: step(name), lambda: reset(name), steps) for name in ("x", "y", "y2")}
        verified = verified and torch.equal(pcm, ref)     # what the region's last step left: the verified PCM
        if r:   # the first region is discarded
            for name in out:
                out[name].append(t[name])
    for bb in b.values():
        bb.close()
    med = {k: float(np.median(v)) for k, v in out.items()}
    frames = S * n * calls
    spread = abs(med["y"] / med["y2"] - 1.0)
    return dict(verified=bool(verified), oracle=oracle_ok, oracle_stream_ids=ids, routes=routes, new_entry=stats(out["x"]),
                render_range=stats(out["y"]), render_range_again=stats(out["y2"]),
                ratio_render_range_over_new_entry=round(med["y"] / med["x"], 4), spread_render_range_vs_itself=round(spread, 4),
                fuse=bool(med["y"] / med["x"] - 1.0 > spread), new_entry_gsample_frames_s=round(frames / med["x"] / 1e6, 2),
                render_range_gsample_frames_s=round(frames / med["y"] / 1e6, 2))


def chain(A, O, IU, torch, S, F, steps, regions):
    """stereo 44.1 -> 48 kHz: render f32 (limiter off), resample, limiter stage; F frames of 1024, frame by frame"""
    import synth
    ch, fs = 2, 1024
    amx, omx = IU.identity_matrices(ch)
    basis = np.stack([synth.hot(7100 + i, ch, F * fs) for i in range(16)])                    # [16][ch][F * fs]
    xf = np.ascontiguousarray(basis.reshape(16, ch, F, fs).transpose(0, 2, 1, 3))             # [16][F][ch][fs] planar frames
    d_x = torch.from_numpy(xf).cuda().repeat((S + 15) // 16, 1, 1, 1)[:S].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    b1 = A.Batch(S, amx, ch, frame_size=fs, sample_rate=44100, out_format=A.FMT_F32, limiter=False, projection=A.PROJ_EXACT)
    rs = A.Resampler(S, ch, 44100, 48000)
    b3 = {k: A.Batch(S, amx, ch, frame_size=1, out_format=A.FMT_S16, projection=A.PROJ_EXACT) for k in ("x", "y")}
    cap = rs.out_capacity(fs)
    ss = (cap * ch + 3) & ~3
    d_f32 = torch.zeros((S, fs * ch), dtype=torch.float32, device="cuda")
    d_rs = torch.zeros((S, ss), dtype=torch.float32, device="cuda")
    slot = r16(cap * ch * 2)
    pcm = torch.zeros((S, F * slot), dtype=torch.uint8, device="cuda")
    emitted = []

    def step(series):
        del emitted[:]
        bb = b3["x" if series == "x" else "y"]
        for f in range(F):
            b1.render(d_x.data_ptr() + 4 * f * ch * fs, F * ch * fs, ch * fs, 1, d_f32.data_ptr(), fs * ch * 4, st)
            n = rs.process(d_f32.data_ptr(), fs * ch, fs, d_rs.data_ptr(), ss, st)
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = d_rs.data_ptr(), ss, ch
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = n, pcm.data_ptr() + f * slot, F * slot, st
            emitted.append(bb.render_interleaved(a) if series == "x" else bb.render_range(a, 0, S))

    def reset(series):
        b1.reset()
        rs.restart_range(0, S, st)
        b3["x" if series == "x" else "y"].reset()

    ids = sorted({0, S // 3, (2 * S) // 3, S - 1})
    want = {}
    for s in ids:
        y, counts = O.resample_run(basis[s % 16], 44100, 48000, [fs] * F, flush=False)
        z, _ = O.limiter_run(np.ascontiguousarray(np.zeros_like(y) + y, dtype=np.float32), list(counts), flush=False)
        want[s] = O.pack(z, 16)
    snap, oracle_ok, routes = {}, {}, {}
    for series in ("x", "y"):
        reset(series)
        pcm.zero_()
        A.route_reset()
        A.route_family_tally(FAM, reset=True)
        step(series)
        torch.cuda.synchronize()
        snap[series] = pcm.clone()
        rows = pcm[ids].cpu().numpy()
        g = [np.concatenate([rows[i, k * slot:k * slot + e * ch * 2] for k, e in enumerate(emitted)]) for i in range(len(ids))]
        oracle_ok[series] = all(np.array_equal(g[i].view(np.int16).reshape(-1, ch), want[s]) for i, s in enumerate(ids))
        routes[series] = routes_now(A)
    verified = all(oracle_ok.values()) and torch.equal(snap["x"], snap["y"])
    snap.clear()
    out = {"x": [], "y": [], "y2": []}
    for r in range(regions + 1):
        t = {name: timed(torch, lambda: step(name), lambda: reset(name), steps) for name in ("x", "y", "y2")}
        if r:
            for name in out:
                out[name].append(t[name])
    for bb in list(b3.values()) + [b1]:
        bb.close()
    rs.close()
    med = {k: float(np.median(v)) for k, v in out.items()}
    frames = S * F * fs
    return dict(verified=bool(verified), oracle=oracle_ok, oracle_stream_ids=ids, routes=routes, new_entry=stats(out["x"]),
                render_range=stats(out["y"]), render_range_again=stats(out["y2"]),
                ratio_render_range_over_new_entry=round(med["y"] / med["x"], 4),
                spread_render_range_vs_itself=round(abs(med["y"] / med["y2"] - 1.0), 4),
                new_entry_ginput_frames_s=round(frames / med["x"] / 1e6, 2), render_range_ginput_frames_s=round(frames / med["y"] / 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--lengths", default=",".join(LENGTHS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--chain-frames", type=int, default=64)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import interleaved_util as IU
    import oracle_lib as O
    assert torch.cuda.is_available()
    res = {}
    for S in (int(v) for v in a.streams.split(",")):
        for name in a.lengths.split(","):
            n, calls = LENGTHS[name]
            for ch, label in ((1, "mono"), (2, "stereo")):
                res["%s_%s_%d_streams" % (label, name, S)] = run(A, O, IU, torch, ch, S, n, calls, a.steps, a.regions)
                torch.cuda.empty_cache()
        res["chain_stereo_44100_48000_%d_streams" % S] = chain(A, O, IU, torch, S, a.chain_frames, a.steps, a.regions)
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "interleaved_rate", "workload": "mono / stereo interleaved f32 through the identity -> s16 on a frame_size == 1 "
                      "batch, 64 x 1115 (or 64 x 1024) sample-frames per stream and step, input resident in HBM, hot programme; "
                      "iamf_hip_batch_render_interleaved against iamf_hip_batch_render_range on a twin batch; chain: stereo 44.1 -> 48 "
                      "kHz, %d frames of 1024 (render f32, resample, limiter stage)" % a.chain_frames,
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
