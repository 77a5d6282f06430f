#!/usr/bin/env python3
"""A two-element mix from 24-bit LPCM packets: one fused iamf_hip_batch_render_packets_mix call (render_fast_kernel<.., LP, true,
3, LPC, LP2> reads both elements' packets itself) against what the PARENT commit does for the same packets —
iamf_hip_batch_render_lpcm_mix, which unpacks both elements there (two iamf_hip_lpcm_unpack passes, then the f32 mixing kernel)
— timed from a build of the parent commit loaded beside this build in ONE process, the two alternating.  The protocol is
tools/lpcm_mix_rate.py's.

    git worktree add ../parent HEAD~1 && make -C ../parent/iac_amd/csrc
    python tools/lpcm24_mix_rate.py --baseline-lib ../parent/iac_amd/lib/libiamf_hip.so > profiles/r16_lpcm24_mix_rate.json

Geometry: bench.py's — S streams x 64 frames x 1024 samples into Sound System A, s16 — for three beds with their second
element: 3rd-order ambisonics (16 mono-coded runs) + a coupled stereo pair, 5.1 (coupled) + mono, 7.1.4 (coupled) + a coupled
stereo pair; both elements resident in HBM as 24-bit little-endian packet rows, the hot programme (tests/synth.py)
quantised to 24 bit, for S = 512, 2048 and 4096.  A step = the work of one call over all frames on fresh state: the batch is
reset before each step, outside the timing, and EACH STEP is timed on its own by a pair of HIP events on the stream around
it.  A region's figure is the mean of its --steps step times; per series the median / min / max of --regions regions after
one discarded region.  Series:
  x      = the fused call, this build
  y, y2  = the BASELINE through the parent build, twice (the spread y against y2 is what a ratio has to clear):
           iamf_hip_batch_render_lpcm_mix on the same two inputs
  u      = this build's new entry with IAMF_HIP_LPCM_UNFUSED=1: a cross-check beside the baseline, never the baseline
Without --baseline-lib the tool stops: a figure against `u` alone decides nothing.
Every timed launch is verified: the PCM a step left is hashed after the region's last step and compared with the hash of the
PCM that the oracle-checked launch of the same series left at the timed geometry (four streams against the oracle bit for
bit — oracle_lib.render of each element, (0 + y0) + y1, limiter_run, pack — every stream by SHA-256 across the series, the
baseline twin's included); the route listings say which kernels ran.

What the host does with the figures (iac_amd/csrc/render_route.hpp): a (shape, size) at which y / x does not exceed 1 by more
than that run's y-against-y2 spread is not fused (lpcm24_mix_fused).

Prints ONE JSON line.  usage: python tools/lpcm24_mix_rate.py --baseline-lib PATH [--streams 512,2048,4096]
[--shapes hoa3+stereo,l51+mono,l714+stereo] [--frames 64] [--steps 10] [--regions 5]"""
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
# shape -> (bed channels, bed layout or ambisonics order, second element's channels, its form)
SHAPES = {"hoa3+stereo": (16, 3, 2, "pair"), "l51+mono": (6, "L51", 1, "mono"), "l714+stereo": (12, "L714", 2, "pair")}
FAM = "LPCM24_MIX"
FULL = 1 << 23


@contextlib.contextmanager
def switch(name):
    os.environ.pop("IAMF_HIP_LPCM_UNFUSED", None)
    if name:
        os.environ[name] = "1"
    try:
        yield
    finally:
        if name:
            os.environ.pop(name, None)


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


class Baseline:
    """the entries this tool calls, bound on another build of the library (the parent commit's)"""

    def __init__(self, A, path):
        L = C.CDLL(path)
        FP = C.POINTER(C.c_float)
        L.iamf_hip_batch_create.argtypes = [C.POINTER(A.hipabi.BatchConfig), C.POINTER(C.c_void_p)]
        L.iamf_hip_batch_destroy.argtypes = [C.c_void_p]
        L.iamf_hip_batch_destroy.restype = None
        L.iamf_hip_batch_reset.argtypes = [C.c_void_p]
        L.iamf_hip_batch_set_second_element.argtypes = [C.c_void_p, C.POINTER(A.Matrix), FP]
        L.iamf_hip_batch_render_lpcm_mix.argtypes = [C.c_void_p, C.POINTER(A.LpcmMixCall), C.c_int32, C.c_int32]
        L.iamf_hip_route_tally.argtypes = [C.POINTER(A.RouteRow), C.c_int, C.c_int]
        assert not hasattr(L, "iamf_hip_batch_render_packets_mix"), "the baseline library already has the entry: not the parent's build"
        self.L, self.A = L, A

    def batch(self, cfg, mx2):
        h = C.c_void_p()
        r = self.L.iamf_hip_batch_create(C.byref(cfg), C.byref(h))
        assert r == 0, "the baseline library refused the batch: %d" % r
        r = self.L.iamf_hip_batch_set_second_element(h, C.byref(mx2), None)
        assert r == 0, "the baseline library refused the second element: %d" % r
        return h

    def routes(self):
        rows = (self.A.RouteRow * 64)()
        n = min(self.L.iamf_hip_route_tally(rows, 64, 1), 64)
        return sorted("%s_v%d_m%d_c%d" % (self.A.hipabi.ROUTE_NAME.get(r.family, str(r.family)), r.variant, r.m, r.c) for r in rows[:n])


def oracle(O, omx, omx2, oc, x0, x1, fs):
    """gains of 1 are skipped by the reference: render, (0 + y0) + y1, limiter, pack"""
    y0, y1 = O.render(omx, x0, oc), O.render(omx2, x1, oc)
    z = np.ascontiguousarray((np.zeros_like(y0) + y0) + y1, dtype=np.float32)
    z, _ = O.limiter_run(z, [fs] * (x0.shape[1] // fs), flush=False)
    return O.pack(z, 16)


def run(A, O, torch, base, shape, packets, S, F, fs, steps, regions):
    m, bed, m2, form2 = SHAPES[shape]
    d_raw0, L0, row0, x0, d_raw1, L1, row1, x1 = packets
    oc = 2
    if isinstance(bed, int):
        mx, omx = A.get_h2m_matrix(bed, A.SS["A"]), O.get_h2m(bed, O.SS["A"])
    else:
        mx, omx = A.get_m2m_matrix(A.SS[bed], A.SS["A"]), O.get_m2m(O.SS[bed], O.SS["A"])
    e2 = "STEREO" if m2 == 2 else "MONO"
    mx2, omx2 = A.get_m2m_matrix(A.SS[e2], A.SS["A"]), O.get_m2m(O.SS[e2], O.SS["A"])
    b = A.Batch(S, mx, oc, frame_size=fs, out_format=A.FMT_S16)
    b.set_second_element(mx2)
    hb = base.batch(b.cfg, mx2)
    cap = F * fs * oc * 2
    pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    in0, in1 = A.LpcmInput(), A.LpcmInput()
    in0.d_raw, in0.raw_stream_stride, in0.raw_frame_stride, in0.first_sample, in0.layout = d_raw0.data_ptr(), F * row0, row0, 0, L0
    in1.d_raw, in1.raw_stream_stride, in1.raw_frame_stride, in1.first_sample, in1.layout = d_raw1.data_ptr(), F * row1, row1, 0, L1
    a = A.RenderArgs()
    a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = F, pcm.data_ptr(), cap, st
    old = A.LpcmMixCall()
    old.in_[0], old.in_[1], old.args = in0, in1, a
    names = {"x": None, "y": None, "y2": None, "u": "IAMF_HIP_LPCM_UNFUSED"}

    def reset(series):
        if series in ("y", "y2"):
            assert base.L.iamf_hip_batch_reset(hb) == 0
        else:
            b.reset()

    def step(series):
        with switch(names[series]):
            if series in ("y", "y2"):
                r = base.L.iamf_hip_batch_render_lpcm_mix(hb, C.byref(old), 0, S)
                assert r >= 0, "the baseline library refused the call: %d" % r
            else:
                b.render_packets_mix(in0, in1, a)

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
    want = {s: oracle(O, omx, omx2, oc, x0[s % x0.shape[0]], x1[s % x1.shape[0]], fs) for s in ids}
    for series in ("x", "y", "u"):
        reset(series)
        pcm.zero_()
        A.route_reset()
        A.route_family_tally(FAM, reset=True)
        base.routes()
        step(series)
        torch.cuda.synchronize()
        hashes[series] = sha(pcm)
        h = pcm[ids].cpu().numpy()
        oracle_ok[series] = all(np.array_equal(h[i, :n_out * oc * 2].view(np.int16).reshape(-1, oc), want[s][:n_out]) for i, s in enumerate(ids))
        routes[series] = base.routes() if series == "y" else sorted(
            "%s_v%d_m%d_c%d_k%d" % r for r in list(A.route_family_tally(FAM, reset=True)) + list(A.route_tally()))
    verified = all(oracle_ok.values()) and len(set(hashes.values())) == 1
    verified = verified and any(r.startswith(FAM) for r in routes["x"]) and not any(r.startswith(FAM) for r in routes["u"])
    out = {n: [] for n in names}
    timed_ok = True
    for r in range(regions + 1):
        t = {}
        for n in ("x", "y", "u", "y2"):
            t[n] = region(n)
            timed_ok = timed_ok and sha(pcm) == hashes["y"]   # what the region's last launch left: the verified PCM
        if r:   # the first region is discarded
            for n in names:
                out[n].append(t[n])
    b.close()
    base.L.iamf_hip_batch_destroy(hb)
    med = {n: float(np.median(v)) for n, v in out.items()}
    frames = S * F * fs
    fused_b = 3 * (m + m2) + oc * 2                                            # 58 / 25 / 46 bytes per sample-frame
    base_b = (3 * m + 4 * m) + (3 * m2 + 4 * m2) + (4 * (m + m2) + oc * 2)     # 202 / 81 / 158
    spread = abs(med["y"] / med["y2"] - 1.0)

    def stats(v):
        return dict(min_ms=round(min(v), 4), median_ms=round(float(np.median(v)), 4), max_ms=round(max(v), 4))

    return dict(verified=bool(verified and timed_ok), oracle=oracle_ok, oracle_stream_ids=ids, sha256=hashes, routes=routes,
                fused=stats(out["x"]), baseline=stats(out["y"]), baseline_again=stats(out["y2"]), unfused_this_build=stats(out["u"]),
                ratio_baseline_over_fused=round(med["y"] / med["x"], 4),
                ratio_min=round(min(out["y"]) / max(out["x"]), 4), ratio_max=round(max(out["y"]) / min(out["x"]), 4),
                spread_baseline_vs_baseline=round(spread, 4),
                ratio_unfused_this_build_over_baseline=round(med["u"] / med["y"], 4),
                fuse=bool(med["y"] / med["x"] - 1.0 > spread),
                fused_gsample_frames_s=round(frames / med["x"] / 1e6, 2), baseline_gsample_frames_s=round(frames / med["y"] / 1e6, 2),
                fused_bytes_per_frame=fused_b, baseline_bytes_per_frame=base_b,
                fused_share_of_8TBs=round(frames * fused_b / (med["x"] * 1e-3) / HBM_BYTES_PER_S, 4),
                baseline_share_of_8TBs=round(frames * base_b / (med["y"] * 1e-3) / HBM_BYTES_PER_S, 4))


def element(synth, LP, seed, m, widths, perm, F, fs, level=1.0):
    """the hot programme quantised to 24 bit: 16 seeded streams -> (packet rows, layout, row bytes, planar f32 [16][m][F * fs])"""
    basis = np.stack([synth.hot(seed + i, m, F * fs) for i in range(16)]) * level
    ints = np.clip(np.rint(basis.astype(np.float64) * FULL), -FULL, FULL - 1).astype(np.int64)
    ints = np.ascontiguousarray(ints.reshape(16, m, F, fs).transpose(0, 2, 1, 3))        # [16][F][ch][fs]
    raw, L, row = LP.rows(ints, 3, True, widths, perm, head=0, pad=0, frame_size=fs)
    x = (ints[:, :, perm, :].astype(np.float64) / FULL).astype(np.float32)
    return raw, L, row, np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(16, m, F * fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True, help="libiamf_hip.so built from the parent commit")
    ap.add_argument("--streams", default="512,2048,4096")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    import torch

    import iac_amd as A
    import lpcm_util as LP
    import oracle_lib as O
    import route_cases_lpcm_mix as RM
    import synth
    assert torch.cuda.is_available()
    assert os.path.realpath(a.baseline_lib) != os.path.realpath(A.lib_path()), "the baseline is this build"
    base = Baseline(A, a.baseline_lib)
    res = {}
    for shape in a.shapes.split(","):
        m, _, m2, form2 = SHAPES[shape]
        w0, p0 = RM.elem0_substreams(m, np.random.default_rng(11))
        w1, p1 = RM.elem1_substreams(m2, form2)
        raw0, L0, row0, x0 = element(synth, LP, 4242, m, w0, p0, a.frames, a.fs)
        raw1, L1, row1, x1 = element(synth, LP, 5151, m2, w1, p1, a.frames, a.fs, level=0.5)     # (the second element 6 dB down)
        for S in (int(v) for v in a.streams.split(",")):
            reps = (S + 15) // 16
            d_raw0 = torch.from_numpy(raw0).cuda().repeat(reps, 1, 1)[:S].contiguous()
            d_raw1 = torch.from_numpy(raw1).cuda().repeat(reps, 1, 1)[:S].contiguous()
            res["%s_%d_streams" % (shape, S)] = run(A, O, torch, base, shape, (d_raw0, L0, row0, x0, d_raw1, L1, row1, x1), S, a.frames,
                                                    a.fs, a.steps, a.regions)
            del d_raw0, d_raw1
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "lpcm24_mix_rate", "workload": "bed + second element as 24-bit little-endian LPCM packets -> Sound System A "
                      "s16, %d frames of %d samples per stream, packets resident in HBM, hot programme quantised to 24 bit; one fused "
                      "iamf_hip_batch_render_packets_mix call against iamf_hip_batch_render_lpcm_mix on the same packets through the "
                      "parent commit's build (two unpacks, then the f32 mixing kernel)" % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "steps_per_region": a.steps, "regions": a.regions, "results": res}))


if __name__ == "__main__":
    main()
