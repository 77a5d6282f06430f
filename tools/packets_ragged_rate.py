#!/usr/bin/env python3
"""LPCM packets of any call length: iamf_hip_batch_render_packets_ragged (render_fast_kernel<.., LP, true, LPB, LPC, 0, IL = false,
RAG = true>) against what the call ran before — iamf_hip_batch_render_packets on a twin batch, the parent commit's path (its
kernels are unchanged: tools/kernel_hashes.py): iamf_hip_lpcm_unpack, then the general kernel — in ONE process, the two
alternating.  The protocol is tools/ragged_rate.py's.

    python tools/packets_ragged_rate.py > profiles/r17_packets_ragged_rate.json

Geometry: S streams into stereo s16, for S = 512, 2048 and 4096, of a 3rd-order ambisonics element as 16- and as 24-bit
mono-coded packets (toa16, toa24), of 5.1 as coupled packets of both widths (l51_16, l51_24) and of 7.1.4 the same (l714_16,
l714_24), each through the library's matrix; the hot programme (tests/synth.py) on the packets' grid, resident in HBM.
Lengths: one frame of 1000 per call, one frame of 480 per call, 64 frames of 1000 in one call.  A step = 64 frames per stream
on fresh state: 64 calls of one frame, or one call of 64, every call's PCM into a 16-byte aligned slot of its own; the batch
is reset before each step, outside the timing, and EACH STEP is timed by a pair of HIP events around it.  A region's figure is
the mean of its --steps step times; per series the median / min / max of --regions regions after one discarded region.
Series:
  x      = the new entry
  y, y2  = iamf_hip_batch_render_packets on the twin batch, twice (the spread y against y2 is what a ratio has to clear)
Every series is verified in the same run: four streams of the PCM a step left against the oracle bit for bit, every byte of
every stream's PCM equal across the series (compared on the device, again after every timed region), and the route listings
say which kernels ran.  (64 frames of 1000 are 1000 whole 64-sample blocks: both entries run the form's whole-block family
there, and the listing says so; the figure shows what the new entry's own checks cost.)

What the host does with the figures (iac_amd/csrc/render_route.hpp): a (shape, size) at which y / x does not exceed 1 by more
than that run's y-against-y2 spread is not fused (packets_ragged_fused).

Prints ONE JSON line.  usage: python tools/packets_ragged_rate.py [--streams 512,2048,4096] [--steps 10] [--regions 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = {"1000": (1000, 1, 64), "480": (480, 1, 64), "64x1000": (1000, 64, 1)}     # name -> (frame size, frames per call, calls per step)
SHAPES = {"toa16": ("s16", 16), "toa24": ("s24", 16), "l51_16": ("s16c", 6), "l51_24": ("s24c", 6), "l714_16": ("s16c", 12), "l714_24": ("s24c", 12)}
ELEMENT = {6: "L51", 12: "L714"}
FAM = "PACKETS_RAGGED"


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


def routes_now(A, PU):
    fam, base, rest = PU._tallies(A)
    return sorted("%s_v%d_m%d_c%d_k%d" % r for r in list(fam) + list(base) + list(rest))


def run(A, O, torch, shape, S, fs, nf, calls, steps, regions):
    """calls of nf frames of fs samples into stereo s16; every call reads the same nf frames of packets"""
    import packets_ragged_util as PU
    import synth
    form, m = SHAPES[shape]
    bps = PU.FORMS[form][0]
    if m == 16:
        amx, omx = A.get_h2m_matrix(3, A.SS["A"]), O.get_h2m(3, O.SS["A"])
    else:
        amx, omx = A.get_m2m_matrix(A.SS[ELEMENT[m]], A.SS["A"]), O.get_m2m(O.SS[ELEMENT[m]], O.SS["A"])
    oc, n = 2, nf * fs
    ints = PU.quantise(np.stack([synth.hot(8100 + i, m, n) for i in range(16)]), bps)            # [16][m][n], playback order
    raw, L, row = PU.packets_of(form, ints, nf, fs, head=0, pad=0)                                # [16][nf][row]
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).cuda().repeat((S + 15) // 16, 1, 1)[:S].contiguous()
    slot = r16(n * oc * 2)
    pcm = torch.zeros((S, calls * slot), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    b = {k: A.Batch(S, amx, oc, frame_size=fs, out_format=A.FMT_S16, projection=A.PROJ_EXACT) for k in ("x", "y")}
    emitted = []

    def step(series):
        del emitted[:]
        bb = b["x" if series == "x" else "y"]
        for k in range(calls):
            inp, a = A.LpcmInput(), A.RenderArgs()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr() + k * slot, calls * slot, st
            emitted.append(bb.render_packets_ragged(inp, a) if series == "x" else bb.render_packets(inp, a))

    def reset(series):
        b["x" if series == "x" else "y"].reset()

    def gathered(rows):
        return [np.concatenate([rows[i, k * slot:k * slot + e * oc * 2] for k, e in enumerate(emitted)]) for i in range(rows.shape[0])]

    ids = sorted({0, S // 3, (2 * S) // 3, S - 1})
    want = {}
    for s in ids:
        x = np.tile(PU.as_f32(ints[s % 16], bps), (1, calls))
        y = O.render(omx, x, oc)
        z = np.ascontiguousarray(np.zeros_like(y) + y, dtype=np.float32)
        z, _ = O.limiter_run(z, [n] * calls, flush=False)
        want[s] = O.pack(z, 16)
    snap, routes, oracle_ok = {}, {}, {}
    for series in ("x", "y"):
        reset(series)
        pcm.zero_()
        PU._reset(A)
        step(series)
        torch.cuda.synchronize()
        snap[series] = pcm.clone()
        g = gathered(pcm[ids].cpu().numpy())
        oracle_ok[series] = all(np.array_equal(g[i].view(np.int16).reshape(-1, oc), want[s]) for i, s in enumerate(ids))
        routes[series] = routes_now(A, PU)
    verified = all(oracle_ok.values()) and torch.equal(snap["x"], snap["y"])
    ref = snap.pop("y")
    snap.clear()
    ragged = n % 64 != 0
    whole = [r for r in routes["y"] if r.split("_v")[0] == PU.WHOLE[form] and r.endswith("_m%d_c%d_k0" % (m, oc))]
    verified = verified and (routes["x"] == ["%s_v0_m%d_c%d_k%d" % (FAM, m, oc, bps)] if ragged else (len(whole) == 1 and routes["x"] == whole))
    verified = verified and (routes["y"] == ["GENERIC_v0_m%d_c0_k0" % m] if ragged else routes["y"] == whole)
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
    samples = S * n * calls
    spread = abs(med["y"] / med["y2"] - 1.0)
    return dict(verified=bool(verified), oracle=oracle_ok, oracle_stream_ids=ids, routes=routes, new_entry=stats(out["x"]),
                render_packets=stats(out["y"]), render_packets_again=stats(out["y2"]),
                ratio_render_packets_over_new_entry=round(med["y"] / med["x"], 4), spread_render_packets_vs_itself=round(spread, 4),
                fuse=bool(med["y"] / med["x"] - 1.0 > spread), new_entry_gsamples_s=round(samples / med["x"] / 1e6, 2),
                render_packets_gsamples_s=round(samples / med["y"] / 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--lengths", default=",".join(LENGTHS))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import oracle_lib as O
    assert torch.cuda.is_available()
    res = {}
    for S in (int(v) for v in a.streams.split(",")):
        for name in a.lengths.split(","):
            fs, nf, calls = LENGTHS[name]
            for shape in a.shapes.split(","):
                res["%s_%s_%d_streams" % (shape, name, S)] = run(A, O, torch, shape, S, fs, nf, calls, a.steps, a.regions)
                torch.cuda.empty_cache()
    print(json.dumps({"tool": "packets_ragged_rate", "workload": "3rd-order ambisonics as 16- / 24-bit mono-coded packets, 5.1 and 7.1.4 as coupled "
                      "packets of both widths -> stereo s16, 64 frames of 1000 (or 480) samples per stream and step, packets resident in HBM, hot "
                      "programme; iamf_hip_batch_render_packets_ragged against iamf_hip_batch_render_packets on a twin batch",
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
