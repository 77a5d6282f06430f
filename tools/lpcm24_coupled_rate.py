#!/usr/bin/env python3
"""Coupled 24-bit LPCM packets into the headline kernel: one fused iamf_hip_batch_render_packets call
(render_fast_kernel<.., LP, EARLY, 3, LPC> reads the packets itself) against what the PARENT commit does for the same packets —
iamf_hip_batch_render_lpcm: iamf_hip_lpcm_unpack, then the f32 kernel — timed from a build of the parent commit loaded beside
this build in ONE process, the two alternating.  The protocol is tools/lpcm_coupled_rate.py's.

    git worktree add ../parent HEAD~1 && make -C ../parent/iac_amd/csrc
    python tools/lpcm24_coupled_rate.py --baseline-lib ../parent/iac_amd/lib/libiamf_hip.so > profiles/r15_lpcm24_coupled_rate.json

Geometry: bench.py's — S streams x 64 frames x 1024 samples into Sound System A, s16 — for a stereo, a 5.1 and a 7.1.4
element whose pairs are coupled sub-streams (C and LFE mono ones), resident in HBM as 24-bit little-endian packet rows in
the decoder façade's layout, the hot programme (tests/synth.py) quantised to 24 bit, for S = 512, 2048 and 4096.  A step =
one call over all frames on fresh state: the batch is reset before each step, outside the timing, and EACH STEP is timed on
its own by a pair of HIP events on the stream around it.  A region's figure is the mean of its --steps step times; per
series the median / min / max of --regions regions after one discarded region.  Series:
  x_early, x_late = the fused call with the prefetch variant forced (IAMF_HIP_LP_EARLY / IAMF_HIP_LP_LATE), this build
  y, y2           = the BASELINE: the same call through the parent build, twice (the spread y against y2 is what a ratio has
                    to clear)
  u               = this build's new entry with IAMF_HIP_LPCM_UNFUSED=1: a cross-check beside the baseline, never the baseline
Without --baseline-lib the tool stops: a figure against `u` alone decides nothing.
Every timed launch is verified: the PCM a step left is hashed after the region's last step and compared with the hash of the
PCM that the oracle-checked launch of the same series left at the timed geometry (stream_ids against oracle_lib.stream_run
bit for bit, every stream by SHA-256 across the series); the route listings say which kernels ran.

What the host does with the figures (iac_amd/csrc/render_route.hpp): a size at which y / x does not exceed 1 by more than
that run's y-against-y2 spread is not fused (lpcm24_coupled_fused); the prefetch variant per size is the one that is faster
by more than that spread (lpcm24_coupled_early).

Prints ONE JSON line.  usage: python tools/lpcm24_coupled_rate.py --baseline-lib PATH [--streams 512,2048,4096]
[--elements 2,6,12] [--frames 64] [--steps 10] [--regions 5]"""
import argparse
import contextlib
import ctypes as C
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
ELEMENT = {2: "STEREO", 6: "L51", 12: "L714"}
FAM = "LPCM24_COUPLED"
FULL = 1 << 23


@contextlib.contextmanager
def switch(name):
    """at most one of SWITCHES set (the library reads them at every call)"""
    for k in SWITCHES:
        os.environ.pop(k, None)
    if name:
        os.environ[name] = "1"
    try:
        yield
    finally:
        if name:
            os.environ.pop(name, None)


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def coupled(m):
    """(widths, perm) of lpcm_util.rows: sub-streams in audio-layer order, playback channel p takes decoded channel perm[p]"""
    if m == 2:
        return [2], [0, 1]
    return [2] * ((m - 2) // 2) + [1, 1], [0, 1, m - 2, m - 1] + list(range(2, m - 2))


class Baseline:
    """the entries this tool calls, bound on another build of the library (the parent commit's)"""

    def __init__(self, A, path):
        L = C.CDLL(path)
        L.iamf_hip_batch_create.argtypes = [C.POINTER(A.hipabi.BatchConfig), C.POINTER(C.c_void_p)]
        L.iamf_hip_batch_destroy.argtypes = [C.c_void_p]
        L.iamf_hip_batch_destroy.restype = None
        L.iamf_hip_batch_reset.argtypes = [C.c_void_p]
        L.iamf_hip_batch_render_lpcm.argtypes = [C.c_void_p, C.POINTER(A.LpcmInput), C.POINTER(A.RenderArgs)]
        L.iamf_hip_route_tally.argtypes = [C.POINTER(A.RouteRow), C.c_int, C.c_int]
        self.L, self.A = L, A

    def batch(self, cfg):
        h = C.c_void_p()
        r = self.L.iamf_hip_batch_create(C.byref(cfg), C.byref(h))
        assert r == 0, "the baseline library refused the batch: %d" % r
        return h

    def routes(self):
        rows = (self.A.RouteRow * 64)()
        n = min(self.L.iamf_hip_route_tally(rows, 64, 1), 64)
        return sorted("%s_v%d_m%d_c%d" % (self.A.hipabi.ROUTE_NAME.get(r.family, str(r.family)), r.variant, r.m, r.c) for r in rows[:n])


def run(A, O, torch, base, d_raw, L, row, x, m, S, F, fs, steps, regions):
    oc = 2
    mx, omx = A.get_m2m_matrix(A.SS[ELEMENT[m]], A.SS["A"]), O.get_m2m(O.SS[ELEMENT[m]], O.SS["A"])
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16)
    hb = base.batch(b.cfg)
    cap = F * fs * oc * 2
    pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    inp = A.LpcmInput()
    inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.first_sample, inp.layout = d_raw.data_ptr(), F * row, row, 0, L
    a = A.RenderArgs()
    a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = F, pcm.data_ptr(), cap, st
    names = {"x_early": "IAMF_HIP_LP_EARLY", "x_late": "IAMF_HIP_LP_LATE", "y": None, "y2": None, "u": "IAMF_HIP_LPCM_UNFUSED"}

    def reset(series):
        if series in ("y", "y2"):
            assert base.L.iamf_hip_batch_reset(hb) == 0
        else:
            b.reset()

    def step(series):
        with switch(names[series]):
            if series in ("y", "y2"):
                r = base.L.iamf_hip_batch_render_lpcm(hb, C.byref(inp), C.byref(a))
                assert r >= 0, "the baseline library refused the call: %d" % r
            else:
                b.render_packets(inp, a)

    def region(series):
        ms = 0.0
        for _ in range(steps):   # every step starts from fresh state: the same work each time (the reset is not timed)
            reset(series)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(series)
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        return ms / steps

    # warm-up, verification against the oracle and routes at the timed geometry
    hashes, routes, oracle_ok = {}, {}, {}
    ids = sorted({0, S // 3, (2 * S) // 3, S - 1})
    n_out = F * fs - 240
    want = {s: O.stream_run(omx, oc, x[s % x.shape[0]], fs, flush=False) for s in ids}
    for series in ("x_early", "x_late", "y", "u"):
        reset(series)
        pcm.zero_()
        A.route_reset()
        A.route_family_tally(FAM, reset=True)
        base.routes()
        step(series)
        torch.cuda.synchronize()
        hashes[series] = sha(pcm)
        h = pcm[ids].cpu().numpy()
        oracle_ok[series] = all(np.array_equal(h[i, :n_out * oc * 2].view(np.int16).reshape(-1, oc), want[s]) for i, s in enumerate(ids))
        routes[series] = base.routes() if series == "y" else sorted(
            "%s_v%d_m%d_c%d" % (r[0], r[1], r[2], r[3]) for r in list(A.route_family_tally(FAM, reset=True)) + list(A.route_tally()))
    verified = all(oracle_ok.values()) and len(set(hashes.values())) == 1
    out = {n: [] for n in names}
    timed_ok = True
    for r in range(regions + 1):
        t = {}
        for n in ("x_early", "y", "x_late", "y2", "u"):
            t[n] = region(n)
            timed_ok = timed_ok and sha(pcm) == hashes["y"]   # what the region's last launch left: the verified PCM
        if r:   # the first region is discarded
            for n in names:
                out[n].append(t[n])
    b.close()
    base.L.iamf_hip_batch_destroy(hb)
    med = {n: float(np.median(v)) for n, v in out.items()}
    frames = S * F * fs
    fused_b, unfused_b = 3 * m + oc * 2, (3 * m + 4 * m) + (4 * m + oc * 2)   # 10 / 22 / 40 and 26 / 70 / 136 bytes per sample-frame
    spread = abs(med["y"] / med["y2"] - 1.0)
    best = "x_early" if med["x_early"] <= med["x_late"] else "x_late"
    other = "x_late" if best == "x_early" else "x_early"
    decided = med[other] / med[best] - 1.0 > spread

    def stats(v):
        return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))

    return dict(verified=bool(verified and timed_ok), oracle=oracle_ok, oracle_stream_ids=ids, sha256=hashes, routes=routes,
                fused_early=stats(out["x_early"]), fused_late=stats(out["x_late"]), baseline=stats(out["y"]),
                baseline_again=stats(out["y2"]), unfused_this_build=stats(out["u"]),
                faster_variant=best[2:], variant_decided=bool(decided),
                ratio_baseline_over_fused_early=round(med["y"] / med["x_early"], 4),
                ratio_baseline_over_fused_late=round(med["y"] / med["x_late"], 4),
                ratio_baseline_over_fused=round(med["y"] / med[best], 4), spread_baseline_vs_baseline=round(spread, 4),
                ratio_unfused_this_build_over_baseline=round(med["u"] / med["y"], 4),
                fuse=bool(med["y"] / med[best] - 1.0 > spread),
                fused_gsample_frames_s=round(frames / med[best] / 1e6, 2), baseline_gsample_frames_s=round(frames / med["y"] / 1e6, 2),
                fused_bytes_per_frame=fused_b, baseline_bytes_per_frame=unfused_b,
                fused_share_of_8TBs=round(frames * fused_b / (med[best] * 1e-3) / HBM_BYTES_PER_S, 4),
                baseline_share_of_8TBs=round(frames * unfused_b / (med["y"] * 1e-3) / HBM_BYTES_PER_S, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True, help="libiamf_hip.so built from the parent commit")
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--elements", default="2,6,12", help="channel counts: 2 = stereo, 6 = 5.1, 12 = 7.1.4")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import lpcm_util as LP
    import oracle_lib as O
    import synth
    assert torch.cuda.is_available()
    assert os.path.realpath(a.baseline_lib) != os.path.realpath(A.lib_path()), "the baseline is this build"
    base = Baseline(A, a.baseline_lib)
    res = {}
    for m in (int(v) for v in a.elements.split(",")):
        # hot programme, quantised to 24 bit: 16 seeded streams, tiled over the batch (the limiter's work per stream is what
        # matters, not that every stream differs)
        basis = np.stack([synth.hot(4242 + i, m, a.frames * a.fs) for i in range(16)])
        ints = np.clip(np.rint(basis.astype(np.float64) * FULL), -FULL, FULL - 1).astype(np.int64)
        ints = np.ascontiguousarray(ints.reshape(16, m, a.frames, a.fs).transpose(0, 2, 1, 3))        # [16][F][ch][fs]
        widths, perm = coupled(m)
        raw, L, row = LP.rows(ints, 3, True, widths, perm, head=0, pad=0, frame_size=a.fs)
        x = (ints[:, :, perm, :].astype(np.float64) / FULL).astype(np.float32)
        x = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(16, m, a.frames * a.fs)
        for S in (int(v) for v in a.streams.split(",")):
            reps = (S + 15) // 16
            d_raw = torch.from_numpy(raw).cuda().repeat(reps, 1, 1)[:S].contiguous()
            res["%s_%d_streams" % (ELEMENT[m].lower(), S)] = run(A, O, torch, base, d_raw, L, row, x, m, S, a.frames, a.fs, a.steps, a.regions)
            del d_raw
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "lpcm24_coupled_rate", "workload": "stereo / 5.1 / 7.1.4 element as coupled 24-bit little-endian LPCM packets -> "
                      "Sound System A s16, %d frames of %d samples per stream, packets resident in HBM, hot programme quantised to 24 "
                      "bit; one fused iamf_hip_batch_render_packets call against iamf_hip_batch_render_lpcm on the same packets through "
                      "the parent commit's build (unpack, then the f32 kernel)"
                      % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
