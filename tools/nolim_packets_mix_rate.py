#!/usr/bin/env python3
"""A two-element packet mix on a batch without the limiter: iamf_hip_batch_render_packets_mix_nolim (render_nolim_kernel<M, LPB,
LPC, LP2>) against what the call ran before — iamf_hip_batch_render_packets_mix_ragged on a twin limiter-off batch, the parent
commit's path (its kernels are unchanged: tools/kernel_hashes.py --anon): two iamf_hip_lpcm_unpack passes, then the general
kernel — in ONE process, the two alternating.  The protocol is tools/nolim_packets_rate.py's.

    python tools/nolim_packets_mix_rate.py > profiles/r20_nolim_packets_mix_rate.json

Geometry: S streams, for S = 512, 2048 and 4096, limiter off:
  toa_stereo16_f32  a 3rd-order ambisonics bed as 16-bit mono-coded packets plus a coupled stereo element into stereo f32 — the
                    first stage of a rate-converting stream (36 + 72 + 72 + 8 = 188 against 36 + 8 = 44 bytes per sample-frame by
                    the shapes)
  l714_mono24_s16   7.1.4 as coupled 24-bit packets plus a mono element into stereo s16 — a stream whose limiter is switched off
                    (39 + 52 + 52 + 4 = 147 against 39 + 4 = 43)
element 0 through the library's matrix, element 1 through a seeded dense one, every gain 1; the hot programme (tests/synth.py) on
the packets' grid, resident in HBM.  Lengths: one frame of 1024 per call (64 calls per step), and 64 frames of 1024 in one call.
A step = 64 frames per stream; every call's PCM goes into a 16-byte aligned slot of its own; EACH STEP is timed by a pair of HIP
events around it.  A region's figure is the mean of its --steps step times; per series the median / min / max of --regions
regions after one discarded region.
Series:
  x      = the new entry
  y, y2  = iamf_hip_batch_render_packets_mix_ragged on the twin batch, twice (the spread y against y2 is what a ratio has to clear)
Every series is verified in the same run: four streams of the PCM a step left against the oracle bit for bit, every byte of
every stream's PCM equal across the series (compared on the device, again after every timed region), and the route listings
say which kernels ran.

What the host does with the figures (iac_amd/csrc/render_route.hpp): a (shape, size) at which y / x does not exceed 1 by more
than that run's y-against-y2 spread is not fused (nolim_packets_mix_fused).

Prints ONE JSON line.  usage: python tools/nolim_packets_mix_rate.py [--streams 512,2048,4096] [--steps 5] [--regions 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = {"1024": (1024, 1, 64), "64x1024": (1024, 64, 1)}     # name -> (frame size, frames per call, calls per step)
# name -> (element 0's form, its channels, element 1's form, its channels, LP2, PCM bit depth; -32: f32)
SHAPES = {"toa_stereo16_f32": ("s16", 16, "s16c", 2, 2, -32), "l714_mono24_s16": ("s24c", 12, "s24", 1, 1, 16)}


def r16(n):
    return (n + 15) & ~15


def stats(v):
    return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))


def timed(torch, fn, steps):
    ms = 0.0
    for _ in range(steps):   # (no state the next step's time depends on: every step is the same work)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
    return ms / steps


def routes_now(A, U):
    fam, base, rest = U._tallies(A)
    return sorted("%s_v%d_m%d_c%d_k%d" % r for r in list(fam) + list(base) + list(rest))


def want(O, omx, omx2, oc, x0, x1, bd):
    """the oracle of one stream with every gain 1: both elements rendered, 0 + y, + y2, the format's conversion"""
    y0, y1 = O.render(omx, np.ascontiguousarray(x0), oc), O.render(omx2, np.ascontiguousarray(x1), oc)
    z = np.ascontiguousarray((np.zeros_like(y0) + y0) + y1, dtype=np.float32)
    return np.ascontiguousarray(z.T) if bd == -32 else O.pack(z, bd)


def run(A, O, torch, shape, S, fs, nf, calls, steps, regions):
    """calls of nf frames of fs samples into stereo; every call reads the same nf frames of packets"""
    import nolim_packets_mix_util as U
    import packets_ragged_util as PU
    import route_cases as R
    import synth
    form, m, form2, m2, lp2, bd = SHAPES[shape]
    bps, pb = PU.FORMS[form][0], U.BPS[bd]
    if m == 16:
        amx, omx = A.get_h2m_matrix(3, A.SS["A"]), O.get_h2m(3, O.SS["A"])
    else:
        amx, omx = A.get_m2m_matrix(A.SS["L714"], A.SS["A"]), O.get_m2m(O.SS["L714"], O.SS["A"])
    oc, n = 2, nf * fs
    amx2, omx2 = R.matrices(m2, oc, table=False, salt=1)
    ints = PU.quantise(np.stack([synth.hot(8100 + i, m, n) for i in range(16)]), bps)            # [16][m][n], playback order
    ints2 = PU.quantise(0.5 * np.stack([synth.hot(9100 + i, m2, n) for i in range(16)]), bps)
    rep = (S + 15) // 16
    d_raw, Ls, rows = [], [], []
    for f, v in ((form, ints), (form2, ints2)):
        raw, L, row = PU.packets_of(f, v, nf, fs, head=0, pad=0)                                  # [16][nf][row]
        d_raw.append(torch.from_numpy(np.ascontiguousarray(raw)).cuda().repeat(rep, 1, 1)[:S].contiguous())
        Ls.append(L)
        rows.append(row)
    slot = r16(n * oc * pb)
    pcm = torch.zeros((S, calls * slot), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    b = {k: A.Batch(S, amx, oc, frame_size=fs, out_format=getattr(A, U.BD_FMT[bd]), projection=A.PROJ_EXACT, limiter=False) for k in ("x", "y")}
    for bb in b.values():
        bb.set_second_element(amx2, [1.0] * S)
    emitted = []

    def step(series):
        del emitted[:]
        bb = b["x" if series == "x" else "y"]
        for k in range(calls):
            ins = []
            for e in range(2):
                inp = A.LpcmInput()
                inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw[e].data_ptr(), nf * rows[e], rows[e], Ls[e]
                ins.append(inp)
            a = A.RenderArgs()
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = nf, pcm.data_ptr() + k * slot, calls * slot, st
            emitted.append((bb.render_packets_mix_nolim if series == "x" else bb.render_packets_mix_ragged)(ins[0], ins[1], a))

    def gathered(r):
        return [np.concatenate([r[i, k * slot:k * slot + e * oc * pb] for k, e in enumerate(emitted)]) for i in range(r.shape[0])]

    ids = sorted({0, S // 3, (2 * S) // 3, S - 1})
    wants = {s: np.tile(want(O, omx, omx2, oc, PU.as_f32(ints[s % 16], bps), PU.as_f32(ints2[s % 16], bps), bd), (calls, 1)) for s in ids}
    snap, routes, oracle_ok = {}, {}, {}
    for series in ("x", "y"):
        pcm.zero_()
        U._reset(A)
        step(series)
        torch.cuda.synchronize()
        snap[series] = pcm.clone()
        g = gathered(pcm[ids].cpu().numpy())
        oracle_ok[series] = all(np.array_equal(g[i].view(np.float32 if bd == -32 else np.int16).reshape(-1, oc), wants[s]) for i, s in enumerate(ids))
        routes[series] = routes_now(A, U)
    verified = all(oracle_ok.values()) and torch.equal(snap["x"], snap["y"])
    ref = snap.pop("y")
    snap.clear()
    verified = verified and routes["x"] == ["%s_v%d_m%d_c0_k%d" % (U.FAM, bps, m, lp2)] and routes["y"] == ["GENERIC_v0_m%d_c0_k0" % m]
    out = {"x": [], "y": [], "y2": []}
    for r in range(regions + 1):
        t = {name: timed(torch, lambda: step(name), steps) for name in ("x", "y", "y2")}
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
                packets_mix_ragged=stats(out["y"]), packets_mix_ragged_again=stats(out["y2"]),
                ratio_packets_mix_ragged_over_new_entry=round(med["y"] / med["x"], 4), spread_packets_mix_ragged_vs_itself=round(spread, 4),
                fuse=bool(med["y"] / med["x"] - 1.0 > spread), new_entry_gsamples_s=round(samples / med["x"] / 1e6, 2),
                packets_mix_ragged_gsamples_s=round(samples / med["y"] / 1e6, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--lengths", default=",".join(LENGTHS))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=5)
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
    print(json.dumps({"tool": "nolim_packets_mix_rate", "workload": "limiter off, two elements: 3rd-order ambisonics as 16-bit mono-coded packets + "
                      "a coupled stereo element -> stereo f32 (the first stage of a rate-converting stream) and 7.1.4 as coupled 24-bit packets + a "
                      "mono element -> stereo s16, 64 frames of 1024 samples per stream and step, packets resident in HBM, hot programme; "
                      "iamf_hip_batch_render_packets_mix_nolim against iamf_hip_batch_render_packets_mix_ragged on a twin batch",
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
