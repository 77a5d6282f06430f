#!/usr/bin/env python3
"""One element held as 24-bit or coupled LPCM packets into K renditions: iamf_hip_batch_render_fanout_packets (the packets read
once, render_fanout_kernel<M, K, true, LPB, LPC>) against BOTH of its baselines on the same packets — K single
iamf_hip_batch_render_packets calls on twin batches (the packets read K times) and iamf_hip_batch_render_fanout_lpcm on a second
set of twins (one unpack pass and the f32 fan-out: what the entry ran for these packets before) — in ONE process, alternating,
through the same library.  The protocol is tools/fanout_lpcm_rate.py's.

Cases: a 3rd-order ambisonics element as 24-bit mono-coded packets, 5.1 as coupled 16-bit packets, 7.1.4 as coupled 24-bit
packets; S streams x 64 frames x 1024 samples resident in HBM, the hot programme (tests/synth.py) quantised to the packets'
sample size, for S = 512, 2048 and 4096.  K = 2 {Sound System A, mono} s16, 3 {+ A with other gains}, 4 {+ mono s24}.  A step =
one call over all frames on fresh state: the batches are reset before each step, outside the timing, and EACH STEP is timed on
its own by a pair of HIP events on the stream around it.  A region's figure is the mean of its --steps step times; per series
the median / min / max of --regions regions after one discarded region.  Series:
  x      = the new entry
  y, y2  = K single iamf_hip_batch_render_packets calls on twin batches, twice (their spread is what a ratio over y has to clear)
  w, w2  = iamf_hip_batch_render_fanout_lpcm on twin batches, twice (likewise)
Before the timing the PCM of x, y and w at the timed geometry is compared by SHA-256 and every s16 member of x is compared
with the oracle on the 16 seeded streams the batch tiles ("verified"); the family tally names the kernel x ran.
"fuse" per (case, K, S): x beats the BETTER baseline by more than that baseline's spread against itself — what fan_pk_fuse_max
(iamf_render.hip) follows.

Prints ONE JSON line.  usage: python tools/fanout_packets_rate.py [--streams 512,2048,4096] [--frames 64] [--steps 10] [--regions 5]"""
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
CASES = [("toa_24bit", "s24", 16), ("5.1_coupled_16bit", "s16c", 6), ("7.1.4_coupled_24bit", "s24c", 12)]


def members(A, k):
    a16 = dict(layout="A", fmt=A.FMT_S16, gains=None)
    m16 = dict(layout="MONO", fmt=A.FMT_S16, gains=None)
    a16g = dict(layout="A", fmt=A.FMT_S16, gains=(0.9, 1.1))
    m24 = dict(layout="MONO", fmt=A.FMT_S24, gains=None)
    return {2: [a16, m16], 3: [a16, a16g, m16], 4: [a16, a16g, m16, m24]}[k]


def make(A, PU, element, sp, S, fs):
    oc = A.layout_channels(A.SS[sp["layout"]])
    b = A.Batch(S, PU.mats(element, sp["layout"])[0], oc, frame_size=fs, out_format=sp["fmt"])
    if sp["gains"]:
        b.set_gains(element=[sp["gains"][0]] * S, output=[sp["gains"][1]] * S)
    b.oc = oc
    b.out_bytes = oc * {A.FMT_S16: 2, A.FMT_S24: 3, A.FMT_S32: 4}[sp["fmt"]]
    return b


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_k(A, PU, O, torch, form, element, d_raw, L, row, x, S, F, fs, k, steps, regions):
    m, bps = L.channels, L.sample_bytes
    specs = members(A, k)
    sets = {n: [make(A, PU, element, sp, S, fs) for sp in specs] for n in ("x", "y", "w")}
    caps = [F * fs * b.out_bytes for b in sets["x"]]
    pcm = {n: [torch.zeros((S, c), dtype=torch.uint8, device="cuda") for c in caps] for n in ("x", "y", "w")}
    st = torch.cuda.current_stream().cuda_stream
    inp = A.LpcmInput()
    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.first_sample, inp.layout = d_raw.data_ptr(), F * row, row, 0, L
    reports = {"x": [], "w": []}

    def step_x():
        _, rep = A.render_fanout_packets(sets["x"], inp, F, [p.data_ptr() for p in pcm["x"]], caps, st)
        reports["x"].append(rep)

    def step_y():
        for b, p, c in zip(sets["y"], pcm["y"], caps):
            a = A.RenderArgs()
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = F, p.data_ptr(), c, st
            b.render_packets(inp, a)

    def step_w():
        _, rep = A.render_fanout_lpcm(sets["w"], inp, F, [p.data_ptr() for p in pcm["w"]], caps, st)
        reports["w"].append(rep)

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
    PU.reset_tallies()
    step_x()
    torch.cuda.synchronize()
    ran = sorted("%s_v%d_m%d_k%d" % (r[0], r[1], r[2], r[4]) for r in A.route_family_tally(PU.FAM, reset=True))
    step_y()
    torch.cuda.synchronize()
    single_routes = sorted("%s_v%d_m%d_c%d" % (r[0], r[1], r[2], r[3]) for r in A.route_family_tally(PU.FORMS[form][3], reset=True))
    step_w()
    torch.cuda.synchronize()
    verified = all(sha(a) == sha(b) == sha(c) for a, b, c in zip(pcm["x"], pcm["y"], pcm["w"]))
    n_out = F * fs - 240
    for j, sp in enumerate(specs):      # the s16 members of x against the oracle, on the seeded streams the batch tiles
        if sp["fmt"] != A.FMT_S16 or not verified:
            continue
        oc = sets["x"][j].oc
        omx = PU.mats(element, sp["layout"])[1]
        host = pcm["x"][j][:min(S, x.shape[0])].cpu().numpy()
        eg, og = sp["gains"] or (1.0, 1.0)
        for s in range(host.shape[0]):
            want = O.stream_run(omx, oc, x[s], fs, flush=False, element_gain=eg, output_gain=og)
            got = host[s][:n_out * oc * 2].view(np.int16).reshape(-1, oc)
            verified = verified and want.shape[0] == n_out and bool(np.array_equal(got, want))
    series = {n: [] for n in ("x", "y", "y2", "w", "w2")}
    for r in range(regions + 1):
        t = dict(x=region(step_x, sets["x"]), y=region(step_y, sets["y"]), w=region(step_w, sets["w"]))
        t["y2"] = region(step_y, sets["y"])
        t["w2"] = region(step_w, sets["w"])
        if r:   # the first region is discarded
            for n in series:
                series[n].append(t[n])
    for bs in sets.values():
        for b in bs:
            b.close()
    med = {n: float(np.median(v)) for n, v in series.items()}
    frames = S * F * fs
    out_bytes = sum(b.out_bytes for b in sets["x"])
    shared_b, single_b, old_b = bps * m + out_bytes, bps * m * k + out_bytes, bps * m + 8 * m + out_bytes

    def stats(v):
        return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))

    sp_y, sp_w = abs(med["y"] / med["y2"] - 1.0), abs(med["w"] / med["w2"] - 1.0)
    best, sp_best = ("singles", sp_y) if min(med["y"], med["y2"]) <= min(med["w"], med["w2"]) else ("fanout_lpcm", sp_w)
    best_ms = min(med["y"], med["y2"]) if best == "singles" else min(med["w"], med["w2"])
    return dict(members=[sp["layout"] + ("_s24" if sp["fmt"] == A.FMT_S24 else "_s16") + ("_gains" if sp["gains"] else "") for sp in specs],
                report=sorted(set(reports["x"])), report_fanout_lpcm=sorted(set(reports["w"])), ran=ran, single_routes=single_routes,
                verified=verified, fanout_packets=stats(series["x"]), singles=stats(series["y"]), singles_again=stats(series["y2"]),
                fanout_lpcm=stats(series["w"]), fanout_lpcm_again=stats(series["w2"]),
                ratio_singles_over_fanout_packets=round(med["y"] / med["x"], 4), spread_singles_vs_singles=round(sp_y, 4),
                ratio_fanout_lpcm_over_fanout_packets=round(med["w"] / med["x"], 4), spread_fanout_lpcm_vs_fanout_lpcm=round(sp_w, 4),
                better_baseline=best, ratio_better_baseline_over_fanout_packets=round(best_ms / med["x"], 4),
                fuse=bool(best_ms / med["x"] - 1.0 > sp_best),
                fanout_packets_gsample_frames_s=round(frames / med["x"] / 1e6, 2),
                fanout_packets_bytes_per_frame=shared_b, singles_bytes_per_frame=single_b, fanout_lpcm_bytes_per_frame=old_b,
                fanout_packets_share_of_8TBs=round(frames * shared_b / (med["x"] * 1e-3) / HBM_BYTES_PER_S, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--k", default="2,3,4")
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    a = ap.parse_args()
    import torch

    import fanout_packets_util as PU
    import iac_amd as A
    import oracle_lib as O
    import synth
    assert torch.cuda.is_available()
    res = {}
    for name, form, m in CASES:
        if name not in a.cases.split(","):
            continue
        bps = PU.FORMS[form][0]
        full = float(1 << (8 * bps - 1))
        # hot programme, quantised to the packets' sample size: 16 seeded streams, tiled over the batch (the limiter's work per
        # stream is what matters, not that every stream differs)
        basis = np.stack([synth.hot(4242 + i, m, a.frames * a.fs) for i in range(16)])
        ints = np.clip(np.rint(basis.astype(np.float64) * full), -full, full - 1).astype(np.int64)
        ints = np.ascontiguousarray(ints.reshape(16, m, a.frames, a.fs).transpose(0, 2, 1, 3))        # [16][F][ch][fs]
        raw, L, row, x = PU.packet_rows(form, ints, a.fs)
        for S in (int(v) for v in a.streams.split(",")):
            reps = (S + 15) // 16
            d_raw = torch.from_numpy(raw).cuda().repeat(reps, 1, 1)[:S].contiguous()
            for k in (int(v) for v in a.k.split(",")):
                res["%s_%d_streams_k%d" % (name, S, k)] = run_k(A, PU, O, torch, form, PU.ELEMENT[m], d_raw, L, row, x, S, a.frames, a.fs, k,
                                                                a.steps, a.regions)
                print("%s, %d streams, K = %d: done" % (name, S, k), file=sys.stderr, flush=True)
            del d_raw
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "fanout_packets_rate", "workload": "one element as 24-bit or coupled LPCM packets -> K renditions, %d frames "
                      "of %d samples per stream, packets resident in HBM, hot programme quantised to the sample size; one "
                      "iamf_hip_batch_render_fanout_packets call against K single iamf_hip_batch_render_packets calls and against "
                      "iamf_hip_batch_render_fanout_lpcm, each on twin batches" % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions,
                      "all_verified": all(r["verified"] for r in res.values()), "results": res}))


if __name__ == "__main__":
    main()
