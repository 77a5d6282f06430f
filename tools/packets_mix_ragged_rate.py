#!/usr/bin/env python3
"""Both elements of a two-element mix as LPCM packets of any call length: iamf_hip_batch_render_packets_mix_ragged
(render_fast_kernel<.., IN2, LP, true, LPB, LPC, LP2, IL = false, RAG = true>) against what the call ran before —
iamf_hip_batch_render_packets_mix on a twin batch, the parent commit's path (its kernels are unchanged: tools/kernel_hashes.py):
two iamf_hip_lpcm_unpack passes, then the general kernel — in ONE process, the two alternating.  The protocol is
tools/packets_ragged_rate.py's.

    python tools/packets_mix_ragged_rate.py > profiles/r18_packets_mix_ragged_rate.json

Geometry: S streams into stereo s16, for S = 512, 2048 and 4096, of a 3rd-order ambisonics bed with a coupled stereo second
element (toa+stereo), 5.1 as coupled packets with a mono second element (l51+mono) and 7.1.4 with a coupled stereo one
(l714+stereo), each in 16 and in 24 bit on both elements, each element through the library's matrix; the hot programme
(tests/synth.py) on the packets' grid, the second element at a quarter of its level, resident in HBM.
Lengths: one frame of 1000 per call, one frame of 480 per call, 64 frames of 1000 in one call.  A step = 64 frames per stream
on fresh state: 64 calls of one frame, or one call of 64, every call's PCM into a 16-byte aligned slot of its own; the batch
is reset before each step, outside the timing, and EACH STEP is timed by a pair of HIP events around it.  A region's figure is
the mean of its --steps step times; per series the median / min / max of --regions regions after one discarded region.
Series:
  x      = the new entry
  y, y2  = iamf_hip_batch_render_packets_mix on the twin batch, twice (the spread y against y2 is what a ratio has to clear)
Every series is verified in the same run: four streams of the PCM a step left against the oracle bit for bit, every byte of
every stream's PCM equal across the series (compared on the device, again after every timed region), and the route listings
say which kernels ran.  (64 frames of 1000 are 1000 whole 64-sample blocks: both entries run the whole-block mix family there,
and the listing says so; the figure shows what the new entry's own checks cost.)

What the host does with the figures (iac_amd/csrc/render_route.hpp): a (shape, size) at which y / x does not exceed 1 by more
than that run's y-against-y2 spread is not fused (packets_mix_ragged_fused).

Prints ONE JSON line.  usage: python tools/packets_mix_ragged_rate.py [--streams 512,2048,4096] [--steps 10] [--regions 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = {"1000": (1000, 1, 64), "480": (480, 1, 64), "64x1000": (1000, 64, 1)}     # name -> (frame size, frames per call, calls per step)
# name -> (bytes per sample, bed's channels, second element's channels, LP2)
SHAPES = {"toa+stereo_16": (2, 16, 2, 2), "toa+stereo_24": (3, 16, 2, 2), "l51+mono_16": (2, 6, 1, 1), "l51+mono_24": (3, 6, 1, 1),
          "l714+stereo_16": (2, 12, 2, 2), "l714+stereo_24": (3, 12, 2, 2)}
ELEMENT = {6: "L51", 12: "L714"}
FAM = "PACKETS_MIX_RAGGED"
WHOLE = {2: "LPCM_MIX", 3: "LPCM24_MIX"}


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


def routes_now(A, U):
    fam, base, rest = U.tallies(A)
    return sorted("%s_v%d_m%d_c%d_k%d" % r for r in list(fam) + list(base) + list(rest))


def run(A, O, torch, shape, S, fs, nf, calls, steps, regions):
    """calls of nf frames of fs samples into stereo s16; every call reads the same nf frames of packets"""
    import packets_mix_ragged_util as U
    import packets_ragged_util as PU
    import synth
    bps, m, m2, k = SHAPES[shape]
    form0 = {(2, False): "s16", (2, True): "s16c", (3, False): "s24", (3, True): "s24c"}[(bps, m != 16)]
    form1 = {(2, 1): "s16", (2, 2): "s16c", (3, 1): "s24", (3, 2): "s24c"}[(bps, k)]
    if m == 16:
        amx, omx = A.get_h2m_matrix(3, A.SS["A"]), O.get_h2m(3, O.SS["A"])
    else:
        amx, omx = A.get_m2m_matrix(A.SS[ELEMENT[m]], A.SS["A"]), O.get_m2m(O.SS[ELEMENT[m]], O.SS["A"])
    e2 = "STEREO" if m2 == 2 else "MONO"
    amx2, omx2 = A.get_m2m_matrix(A.SS[e2], A.SS["A"]), O.get_m2m(O.SS[e2], O.SS["A"])
    oc, n = 2, nf * fs
    ints0 = PU.quantise(np.stack([synth.hot(8100 + i, m, n) for i in range(16)]), bps)                 # [16][m][n], playback order
    ints1 = PU.quantise(np.stack([synth.hot(9100 + i, m2, n) for i in range(16)]) * 0.25, bps)         # [16][m2][n]
    raw0, L0, row0 = PU.packets_of(form0, ints0, nf, fs, head=0, pad=0)                                 # [16][nf][row]
    raw1, L1, row1 = PU.packets_of(form1, ints1, nf, fs, head=0, pad=0)
    rep = (S + 15) // 16
    d_raw0 = torch.from_numpy(np.ascontiguousarray(raw0)).cuda().repeat(rep, 1, 1)[:S].contiguous()
    d_raw1 = torch.from_numpy(np.ascontiguousarray(raw1)).cuda().repeat(rep, 1, 1)[:S].contiguous()
    slot = r16(n * oc * 2)
    pcm = torch.zeros((S, calls * slot), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    b = {}
    for name in ("x", "y"):
        b[name] = A.Batch(S, amx, oc, frame_size=fs, out_format=A.FMT_S16, projection=A.PROJ_EXACT)
        b[name].set_second_element(amx2)
    emitted = []

    def step(series):
        del emitted[:]
        bb = b["x" if series == "x" else "y"]
        for c in range(calls):
            ins = []
            for d_raw, row, L in ((d_raw0, row0, L0), (d_raw1, row1, L1)):
                inp = A.LpcmInput()
                inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr(), nf * row, row, L
                ins.append(inp)
            a = A.RenderArgs()
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr() + c * slot, calls * slot, st
            emitted.append((bb.render_packets_mix_ragged if series == "x" else bb.render_packets_mix)(ins[0], ins[1], a))

    def reset(series):
        b["x" if series == "x" else "y"].reset()

    def gathered(rows):
        return [np.concatenate([rows[i, c * slot:c * slot + e * oc * 2] for c, e in enumerate(emitted)]) for i in range(rows.shape[0])]

    ids = sorted({0, S // 3, (2 * S) // 3, S - 1})
    want = {}
    for s in ids:
        x0, x1 = np.tile(PU.as_f32(ints0[s % 16], bps), (1, calls)), np.tile(PU.as_f32(ints1[s % 16], bps), (1, calls))
        y0, y1 = O.render(omx, x0, oc), O.render(omx2, x1, oc)
        z = np.ascontiguousarray((np.zeros_like(y0) + y0) + y1, dtype=np.float32)
        z, _ = O.limiter_run(z, [n] * calls, flush=False)
        want[s] = O.pack(z, 16)
    snap, routes, oracle_ok = {}, {}, {}
    for series in ("x", "y"):
        reset(series)
        pcm.zero_()
        U.reset_tallies(A)
        step(series)
        torch.cuda.synchronize()
        snap[series] = pcm.clone()
        g = gathered(pcm[ids].cpu().numpy())
        oracle_ok[series] = all(np.array_equal(g[i].view(np.int16).reshape(-1, oc), want[s]) for i, s in enumerate(ids))
        routes[series] = routes_now(A, U)
    verified = all(oracle_ok.values()) and torch.equal(snap["x"], snap["y"])
    ref = snap.pop("y")
    snap.clear()
    ragged = n % 64 != 0
    whole = ["%s_v0_m%d_c%d_k%d" % (WHOLE[bps], m, oc, k)]
    verified = verified and (routes["x"] == ["%s_v%d_m%d_c%d_k%d" % (FAM, bps, m, oc, k)] if ragged else routes["x"] == whole)
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
    med = {name: float(np.median(v)) for name, v in out.items()}
    samples = S * n * calls
    spread = abs(med["y"] / med["y2"] - 1.0)
    return dict(verified=bool(verified), oracle=oracle_ok, oracle_stream_ids=ids, routes=routes, new_entry=stats(out["x"]),
                render_packets_mix=stats(out["y"]), render_packets_mix_again=stats(out["y2"]),
                ratio_render_packets_mix_over_new_entry=round(med["y"] / med["x"], 4), spread_render_packets_mix_vs_itself=round(spread, 4),
                fuse=bool(med["y"] / med["x"] - 1.0 > spread), new_entry_gsamples_s=round(samples / med["x"] / 1e6, 2),
                render_packets_mix_gsamples_s=round(samples / med["y"] / 1e6, 2))


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
    print(json.dumps({"tool": "packets_mix_ragged_rate", "workload": "3rd-order ambisonics + coupled stereo, 5.1 coupled + mono, 7.1.4 coupled + "
                      "coupled stereo, 16 and 24 bit on both elements -> stereo s16, 64 frames of 1000 (or 480) samples per stream and step, packets "
                      "resident in HBM, hot programme; iamf_hip_batch_render_packets_mix_ragged against iamf_hip_batch_render_packets_mix on a twin "
                      "batch", "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
