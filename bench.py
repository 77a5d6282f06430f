#!/usr/bin/env python3
"""bench.py — throughput of the IAMF post-decode rendering hot path on MI355X.

Workload (BASELINE.json configs[3]/[4], the one `metric` is quoted on): every GPU renders its
shard of the "4096 concurrent mix presentations" batch — 512 independent streams, each
3rd-order HOA (16 ch planar f32, 48 kHz, 1024-sample frames) -> binaural (the reference's
buildable `-sb` path: the 16->2 static matrix) -> peak limiter (-1 dBFS) -> interleaved int16.
A "step" is one pass of that path over one batch of `--frames` frames per stream; the element
PCM is synthetic ("hot" programme, tests/synth.py recipe) and resident in HBM before the timed
region starts.  One process per GPU; streams shard over ranks with no collective in the render
path; the job's one exchange is the gather of the packed PCM to rank 0 over RCCL after the last
step (--gather step gathers every step instead, overlapped with the next render).

`python bench.py --gpus N` with no launcher around it starts the N rank processes itself (before
any GPU call, iac_amd/launch.py) and relays rank 0's line; under torchrun it is one rank.  It
refuses to print a line whose n_gpus differs from --gpus.

Prints ONE JSON line on rank 0.  value = sample-frames rendered by all ranks / wall time of the
median of --repeats timed regions of exactly --steps launches each (all regions are listed under
"repeats").  At N=1 the line also carries "configs": BASELINE configs 2, 3 and the HRTF form of
config 4 measured in the same process with the same harness.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
WORKLOADS = {
    # name: (kind, in_id, out_id, in_ch, algorithmic bytes per sample-frame)
    "toa_binaural_limiter_s16": ("h2m", 3, 0x1020, 16, 16 * 4 + 2 * 2),
    # SURVEY §8 N1 on the device: the headline with element 0 handed over as the stream's own 16-bit LPCM packets
    # (iamf_hip_batch_render_lpcm: the reference's pcm decoder, IAMF_pcm_decoder.c:64-83, fused into the render kernel's
    # loads) instead of the f32 decoder buffer: 16 x 2 B read + 2 x 2 B written per sample-frame
    "toa_binaural_limiter_s16_lpcm16": ("h2m_lpcm", 3, 0x1020, 16, 16 * 2 + 2 * 2),
    "toa_ssH_limiter_s16": ("h2m", 3, 0x9A3, 16, 16 * 4 + 24 * 2),
    "toa_ssB_limiter_s16": ("h2m", 3, 0x050, 16, 16 * 4 + 6 * 2),
    # the same with the HOA LFE generator on (h2m_rdr.c:1151-1239, the reference built
    # -DDISABLE_LFE_HOA=0): two pre-pass kernels (render_lfe.hpp: the serial biquad, one lane per stream)
    # + the general render kernel; bytes = the render's own 76 + 16 of scratch traffic (u and y, written and read)
    "toa_ssB_lfe_limiter_s16": ("h2m_lfe", 3, 0x050, 16, 16 * 4 + 6 * 2 + 16),
    "714_ssJ_limiter_s16": ("m2m", 0x714, 0x470, 12, 12 * 4 + 12 * 2),
    # binaural by HRTF FIR (256-tap synthetic HRIRs; the reference's own binauraliser is not in its
    # tree -> "parity unpinned"): compute-bound on the f32 MFMA, 2*16*2*256 flop per sample-frame
    "toa_hrtf256_limiter_s16": ("fir", 3, 0x1020, 16, 16 * 4 + 2 * 2),
    # scalable channel audio, layers stereo -> 5.1.2 -> 7.1.4 (12 decoded channels in
    # bitstream order) through the demixer (output gains, S1to2..S5to7 / T2toT4 with a demixing mode
    # per frame, recon-gain smoothing), then 7.1.4 -> J, limiter, s16: the general kernel
    "scalable_714_ssJ_limiter_s16": ("demix", 0x714, 0x470, 12, 12 * 4 + 12 * 2),
    # §8 A8: a mix presentation of two elements: 3rd-order HOA bed + stereo dialogue -> binaural
    "toa_plus_stereo_binaural_limiter_s16": ("h2m_in2", 3, 0x1020, 16, 16 * 4 + 2 * 4 + 2 * 2),
    "714_plus_stereo_ssJ_limiter_s16": ("m2m_in2", 0x714, 0x470, 12, 12 * 4 + 2 * 4 + 12 * 2),
    # §8 A5: a 7.1.4 element that carries a demixing parameter, rendered to a smaller IAMF layout by the
    # parametric down-mixer (downmix_renderer.c) with a mode per frame, instead of a gain matrix
    # (the reference takes the down-mixer unless the input has height channels and the output none)
    "714_downmix_512_limiter_s16": ("dmx", 7, 3, 12, 12 * 4 + 8 * 2),
    # (the kernel never reads the LFE row: 7 of the 8 input channels reach a stereo down-mix)
    "710_downmix_stereo_limiter_s16": ("dmx", 5, 1, 8, 7 * 4 + 2 * 2),
    # projection-mode 3rd-order ambisonics: 16 decoded channels -> de-mapping matrix ->
    # 16 ambisonics channels -> binaural / 5.1.  Tolerance mode (AUTO): one composed matrix on the
    # fast / wide4-MFMA kernel; IAMF_HIP_PROJECTION=exact in the environment gives the two exact stages
    "toa_projection_binaural_limiter_s16": ("h2m_proj", 3, 0x1020, 16, 16 * 4 + 2 * 2),
    "toa_projection_ssB_limiter_s16": ("h2m_proj", 3, 0x050, 16, 16 * 4 + 6 * 2),
}
F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: f32-input MFMA, dense (155 TF measured)
F16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: bf16 / f16 MFMA, dense
F32_VALU_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: vector f32 (packed FMA), dense
FIR_TAPS = 256
HRIR_SCALE_R2 = 0.08   # tap scale of the synthetic HRIR set (per-ear gain 1.49)


def synth_hot_device(n_streams, in_ch, frames, fs, seed, device):
    """'hot' programme on the device: N(0, 0.25) noise + a 1.5-amplitude 5 ms burst every 0.5 s
    on every channel (alternating sign), stream-dependent phase.  Layout [S][F][ch][fs]."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    x = torch.randn((n_streams, frames, in_ch, fs), generator=g, device=device, dtype=torch.float32) * 0.25
    t = torch.arange(frames * fs, device=device).view(1, frames, 1, fs)
    phase = (torch.arange(n_streams, device=device) * 997 % 24000).view(n_streams, 1, 1, 1)
    in_burst = ((t - phase) % 24000) < 240
    sign = torch.where(t % 2 == 0, 1.0, -1.0)
    x += in_burst * sign * 1.5
    return x.contiguous()


def measured_traffic(kernel_tag, sf_per_step, workload=None):
    """HBM bytes per launch from the newest committed PMC summary (profiles/*_pmc.json, made by
    tools/prof_summary.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this
    same command), scaled to this run's launch size; None if no summary covers the kernel."""
    import glob
    best = None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")))
    import re
    own = [f for f in files if workload and re.fullmatch(r"r\d+_%s_pmc\.json" % re.escape(workload), os.path.basename(f))]
    for f in own or files:   # this workload's own summary if there is one
        try:
            d = json.load(open(f))
        except Exception:
            continue
        tags = kernel_tag if isinstance(kernel_tag, tuple) else (kernel_tag,)   # a step of several kernels: all of them
        hit = [v["hbm_bytes_per_sample_frame"] for t in tags for name, v in d.get("pmc", {}).items()
               if t in name and "hbm_bytes_per_sample_frame" in v]
        if len(hit) == len(tags):
            best = (sum(hit) * sf_per_step, os.path.basename(f))
    return best


def measured_mfma(workload, kernel_tags):
    """matrix-pipe busy fraction of this workload's kernel from the newest committed SQ-counter summary
    (profiles/r*_sq_counters.json: tools/sq_all.sh + tools/sq_summary.py, rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES)"""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_sq_counters.json")), reverse=True):
        try:
            d = json.load(open(f)).get(workload, {})
        except Exception:
            continue
        tags = kernel_tags if isinstance(kernel_tags, tuple) else (kernel_tags,)
        for name, v in d.items():
            if any(t in name for t in tags) and "mfma_busy_frac_at_2p4GHz" in v:
                return {"busy_frac": v["mfma_busy_frac_at_2p4GHz"], "kernel": name, "source": os.path.basename(f),
                        "note": "SQ_VALU_MFMA_BUSY_CYCLES / (dispatch duration x 2.4 GHz x 1024 SIMDs), a separate rocprofv3 --pmc pass of this workload"}
    return None


def cpu_share():
    """(threads to use, how that was decided): the cores this process may run on, capped by the container's CPU quota
    (cgroup v2 cpu.max / v1 cfs quota) when there is one.  The box's nproc is reported beside it."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    if quota is not None and quota < aff:
        return max(1, int(round(quota))), "cgroup cpu quota %.1f of %d schedulable cores" % (quota, aff)
    return aff, "sched_getaffinity (no cgroup cpu quota)"


def cpu_baseline(workload, fs, seconds_target=12.0):
    """The oracle (oracle/liboracle.so: scalar C port of the reference loops) timed on this box's
    host cores on a bounded sample of the same workload: one stream per thread."""
    import concurrent.futures as cf
    import ctypes as C

    import oracle_lib as O
    import synth
    kind, in_id, out_id, in_ch, _ = WORKLOADS[workload]
    mx = O.get_h2m(in_id, out_id) if kind in ("h2m", "h2m_lfe") else O.get_m2m(in_id, out_id)
    out_ch = O.OUT_CH[out_id]
    frames = 256
    xf = np.ascontiguousarray(synth.hot(4242, in_ch, frames * fs).reshape(in_ch, frames, fs).transpose(1, 0, 2))

    def one_stream(_):
        pcm = np.zeros(fs * out_ch * 4, dtype=np.uint8)
        return O.lib().orc_stream_run_frames(C.byref(mx), out_ch, 1, -1.0, 48000, 16, O.fp(xf), frames, fs,
                                             pcm.ctypes.data_as(C.c_void_p))

    t0 = time.perf_counter()
    n1 = one_stream(0)
    t1 = time.perf_counter() - t0
    single = n1 / t1 / 1e6
    cores, cores_basis = cpu_share()
    reps = max(1, min(int(seconds_target / max(t1, 1e-4)), 256))   # ~seconds_target of wall time on `cores` threads
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(cores) as ex:   # ctypes drops the GIL for the whole C call
        total = sum(ex.map(one_stream, range(cores * reps)))
    tm = time.perf_counter() - t0
    return {"value": round(total / tm / 1e6, 3), "unit": "Msamples/s", "cores": cores, "cores_basis": cores_basis, "nproc": os.cpu_count(), "kind": "port",
            "single_core_value": round(single, 3),
            "sample": "%d streams x %d frames x %d samples of %s through oracle/ (scalar C port of "
                      "the reference loops), one stream per thread" % (cores * reps, frames, fs, workload)}


def reference_baseline(workload, fs, seconds_target=12.0):
    """The REAL reference (oracle/_ref/libiamf_ref.so, built from /root/reference's own sources by
    oracle/Makefile; the built library travels with the repo snapshot) timed on this box's host
    cores: one IAMF_DecoderHandle per thread decoding a synthetic LPCM .iamf stream of the same
    workload through IAMF_decoder_decode (OBU parsing + LPCM unpack + the whole rendering path).
    Returns None when the library is not there (then the oracle port is timed instead)."""
    import concurrent.futures as cf
    import ctypes as C
    path = os.path.join(ROOT, "oracle", "_ref", "libref_driver.so")
    if not os.path.exists(path):
        return None
    try:
        import iamf_writer as W
        import synth
        kind, in_id, out_id, in_ch, _ = WORKLOADS[workload]
        frames = 48
        x = W.quantize(np.clip(synth.hot(4242, in_ch, frames * fs), -1, 1 - 2 ** -15).astype(np.float32), 16)
        pd = lambda pid: W.param_definition(pid, 48000, mode=1)
        stream = W.sequence_header(1) + W.codec_config_lpcm(0, fs, 16, 48000)
        if kind in ("h2m", "h2m_proj", "h2m_in2", "h2m_lfe"):
            stream += W.audio_element_ambisonics_mono(1, 0, in_ch, list(range(in_ch)))
        else:
            stream += W.audio_element_channel(1, 0, 7, list(range(W.LAYOUT_SUBSTREAMS[7][0])))
            perm = [0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9]   # playback -> audio-layer order of 7.1.4
            xal = np.empty_like(x)
            for p_, a in enumerate(perm):
                xal[a] = x[p_]
        ss = {0x1020: None, 0x9A3: 7, 0x470: 9, 0x050: 1}[out_id]
        layouts = [("binaural",)] if ss is None else [("ss", ss)]
        stream += W.mix_presentation(1, [dict(eid=1, pdef=pd(100), default_q78=0)], dict(pdef=pd(101), default_q78=0), layouts)
        desc_len = len(stream)
        for f in range(frames):
            stream += W.temporal_delimiter()
            if kind in ("h2m", "h2m_proj", "h2m_in2", "h2m_lfe"):
                stream += W.audio_frames([(i, W.lpcm_bytes(x[i:i + 1, f * fs:(f + 1) * fs], 16)) for i in range(in_ch)])
            else:
                stream += W.audio_frames(W.channel_element_substreams(7, xal[:, f * fs:(f + 1) * fs], 0, 16))
        buf = (C.c_char * len(stream)).from_buffer_copy(stream)
        drv = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_driver.so"))   # oracle/ref_driver.c
        drv.refdrv_decode.restype = C.c_long
        drv.refdrv_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_double)]

        def one_stream(_):
            sec = C.c_double(0.0)
            n = drv.refdrv_decode(C.addressof(buf), len(stream), -1 if ss is None else ss, 16, -1.0, C.byref(sec))
            return n, sec.value

        n1, t1 = one_stream(0)
        if n1 <= 0:
            return None
        single = n1 / t1 / 1e6
        cores, cores_basis = cpu_share()
        reps = max(1, min(int(seconds_target / max(t1, 1e-4)), 256))   # ~seconds_target of wall time
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(cores) as ex:   # ctypes drops the GIL for the whole C call
            res = list(ex.map(one_stream, range(cores * reps)))
        tm = time.perf_counter() - t0
        total = sum(r[0] for r in res)
        return {"value": round(total / tm / 1e6, 3), "unit": "Msamples/s", "cores": cores, "cores_basis": cores_basis, "nproc": os.cpu_count(),
                "kind": "reference", "single_core_value": round(single, 3),
                "sample": "%d decoder handles x %d frames x %d samples of %s through IAMF_decoder_decode of the "
                          "reference itself (oracle/_ref/libiamf_ref.so: LPCM .iamf stream -> PCM), one handle per "
                          "thread" % (cores * reps, frames, fs, workload)}
    except Exception as e:   # anything missing on this box: fall back to the port
        sys.stderr.write("reference baseline unavailable (%s)\n" % e)
        return None


def facade_rates(fs, n_group=64, frames=96):
    """What a caller of the reference's OWN API gets (VERDICT r2 missing #1): the same synthetic LPCM .iamf stream (TOA ->
    binaural, 16-bit) decoded (a) by one IAMF_DecoderHandle, one IAMF_decoder_decode per temporal unit, and (b) by a group
    of `n_group` handles, one iamf_hip_decoder_group_decode per round of temporal units (include/iamf_hip.h).  Host OBU
    parsing, LPCM unpacking, the uploads and the download are all inside: PCIe-inclusive rates, never `value`."""
    import ctypes as C

    import iamf_writer as W
    import synth
    import iac_amd
    L = C.CDLL(iac_amd.lib_path())
    L.IAMF_decoder_open.restype = C.c_void_p
    L.IAMF_decoder_close.argtypes = [C.c_void_p]
    L.IAMF_decoder_configure.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.IAMF_decoder_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_void_p]
    L.IAMF_decoder_output_layout_set_binaural.argtypes = [C.c_void_p]
    L.IAMF_decoder_set_bit_depth.argtypes = [C.c_void_p, C.c_uint32]
    L.iamf_hip_decoder_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.iamf_hip_decoder_group_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iamf_hip_decoder_group_destroy.argtypes = [C.c_void_p]
    L.iamf_hip_decoder_group_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.iamf_hip_decoder_group_destroy.restype = None
    in_ch = 16
    x = W.quantize(np.clip(synth.hot(4242, in_ch, frames * fs), -1, 1 - 2 ** -15).astype(np.float32), 16)
    pd = lambda pid: W.param_definition(pid, 48000, mode=1)
    stream = W.sequence_header(1) + W.codec_config_lpcm(0, fs, 16, 48000)
    stream += W.audio_element_ambisonics_mono(1, 0, in_ch, list(range(in_ch)))
    stream += W.mix_presentation(1, [dict(eid=1, pdef=pd(100), default_q78=0)], dict(pdef=pd(101), default_q78=0), [("binaural",)])
    for f in range(frames):
        stream += W.temporal_delimiter()
        stream += W.audio_frames([(i, W.lpcm_bytes(x[i:i + 1, f * fs:(f + 1) * fs], 16)) for i in range(in_ch)])
    buf = C.create_string_buffer(stream, len(stream))
    base = C.addressof(buf)

    def handle():
        d = L.IAMF_decoder_open()
        L.IAMF_decoder_set_bit_depth(d, 16)
        L.IAMF_decoder_output_layout_set_binaural(d)
        rs = C.c_uint32(0)
        assert L.IAMF_decoder_configure(d, base, len(stream), C.byref(rs)) == 0
        return d, rs.value

    # (a) one handle
    d, used = handle()
    pcm = C.create_string_buffer(2 * 6144 * 2)
    rs = C.c_uint32(0)
    # steady state: the first 8 calls are not timed (the first launch of a kernel loads its code object and opts into its
    # LDS size once per process: ~1 ms, which a 96-frame stream would otherwise carry as 10 us per call)
    total, calls, t0 = 0, 0, time.perf_counter()
    while used < len(stream):
        n = L.IAMF_decoder_decode(d, base + used, len(stream) - used, C.byref(rs), pcm)
        assert n >= 0
        calls += 1
        if calls == 8:
            total, t0 = 0, time.perf_counter()
        elif calls > 8:
            total += n
        used += rs.value
        if not rs.value:
            break
    total += max(0, L.IAMF_decoder_decode(d, None, 0, C.byref(rs), pcm))
    t_single = time.perf_counter() - t0
    L.IAMF_decoder_close(d)
    single = total / t_single / 1e6
    # (b) a group
    phases = {}

    def group_rate(n_group):
        hs, used0 = [], 0
        for _ in range(n_group):
            d, used0 = handle()
            hs.append(d)
        harr = (C.c_void_p * n_group)(*hs)
        g = C.c_void_p()
        assert L.iamf_hip_decoder_group_create(harr, n_group, 0, C.byref(g)) == 0
        pcms = [C.create_string_buffer(2 * 6144 * 2) for _ in range(n_group)]
        parr = (C.c_void_p * n_group)(*[C.addressof(p_) for p_ in pcms])
        data, sizes, rsz, res = (C.c_uint64 * n_group)(), (C.c_int32 * n_group)(), (C.c_uint32 * n_group)(), (C.c_int32 * n_group)()
        vd, vs, vr, vres = (np.frombuffer(a_, dtype=t_) for a_, t_ in ((data, np.uint64), (sizes, np.int32), (rsz, np.uint32), (res, np.int32)))
        used = np.full(n_group, used0, dtype=np.int64)
        total, rounds, t0 = 0, 0, time.perf_counter()
        while int(used.min()) < len(stream):
            vd[:] = (base + used).astype(np.uint64)
            vs[:] = (len(stream) - used).astype(np.int32)
            assert L.iamf_hip_decoder_group_decode(g, data, sizes, rsz, parr, res) == 0
            assert int(vres.min()) >= 0
            total += int(vres.sum())
            used += vr.astype(np.int64)
            rounds += 1
            if int(vr.min()) == 0:
                break
        vd[:] = 0
        vs[:] = 0
        assert L.iamf_hip_decoder_group_decode(g, data, sizes, rsz, parr, res) == 0
        total += int(np.maximum(vres, 0).sum())
        t_group = time.perf_counter() - t0
        ph, nr = (C.c_double * 4)(), C.c_int64(0)
        L.iamf_hip_decoder_group_times(g, ph, C.byref(nr))
        phases[n_group] = {k: round(ph[i_] / max(nr.value, 1) * 1e6, 1) for i_, k in
                           enumerate(("host_parse_stage_us", "enqueue_us", "device_wait_us", "copy_out_us"))}
        L.iamf_hip_decoder_group_destroy(g)
        for d in hs:
            L.IAMF_decoder_close(d)
        return total / t_group / 1e6, t_group / max(rounds + 1, 1) * 1e3

    g64, ms64 = group_rate(n_group)
    g256, ms256 = group_rate(4 * n_group)
    return {"workload": "TOA -> binaural, 16-bit LPCM .iamf, %d frames of %d samples per handle, through the reference's API"
                        % (frames, fs),
            "single_handle_msamples_s": round(single, 2), "single_handle_us_per_call": round(t_single / (frames + 1 - 8) * 1e6, 1),
            "single_handle_note": "steady state: the first 8 of the %d calls are not timed" % (frames + 1),
            "group_handles": n_group, "group_msamples_s": round(g64, 2), "group_ms_per_round": round(ms64, 3),
            "group%d_msamples_s" % (4 * n_group): round(g256, 2), "group%d_ms_per_round" % (4 * n_group): round(ms256, 3),
            "group_phases_per_round": {str(k): v for k, v in phases.items()},
            "note": "host OBU parsing + the LPCM packets over PCIe + device unpack + render + PCM back over PCIe, per call: never `value`"}


SIGNALS = {"hot": "hot (sigma 0.25 + 1.5 bursts)", "quiet": "quiet (sigma 0.05)",
           "sparse": "sparse (sigma 0.05 + an 8-sample 1.5 peak every 1531 samples)",
           "zero": "digital silence (diagnostic: the same instruction stream without data-dependent switching)"}
# BASELINE.json configs that fit one GPU besides the headline (configs[3] matrix form): measured in
# the same process and reported under "configs" of the one JSON line (N=1 only)
# (workload, streams per GPU, placement tries).  BASELINE fixes 512 streams per GPU only for the headline (config 5:
# 4096 over 8 GPUs); configs 2 and 3 name no batch size, and the wide-layout kernels are bound by chunk latency x
# workgroups per CU, so they run on a larger shard (2048 streams: +4-8 % over 512, profiles/r02_streams_sweep.txt).
# Their input's placement does not matter (candidates within 2 %): one try.
# streams per GPU = a whole number of rounds of the workgroups a CU holds (256 CUs x 3 for the 12-channel kernel,
# x 2 for the 24-channel and HRTF kernels)
EXTRA_CONFIGS = [("714_ssJ_limiter_s16", 3072, 4), ("toa_ssH_limiter_s16", 2048, 4), ("toa_hrtf256_limiter_s16", 1024, 1),
                 # the headline fed with the stream's own 16-bit LPCM packets (SURVEY 8 N1 on the device; 36 B per sample-frame)
                 ("toa_binaural_limiter_s16_lpcm16", 4096, 1),   # not HBM-bound: 512: 85, 1024: 116, 2048: 120-125, 4096: 132 Gsamples/s
                 # secondary kernels of SURVEY 8 rows N2 / N4 / A5: in the driver's line so that it times them
                 ("scalable_714_ssJ_limiter_s16", 2048, 1),
                 # the LFE generator's serial recurrence takes 0.61 ms per call WHATEVER the stream count (one lane per stream,
                 # 65 536 dependent steps): the shard is sized to amortise it (1024: 37.6, 2048: 46.5, 4096: 51.9 Gsamples/s)
                 ("toa_ssB_lfe_limiter_s16", 4096, 1),
                 ("710_downmix_stereo_limiter_s16", 2048, 1)]   # (2048: 108 Gsamples/s; 1024: 102, 4096: 110)


def kernel_tag(kind, in_ch, out_ch):
    if kind == "h2m_in2":
        return "render_fast_kernel<%d, %d, 0, false, true" % (in_ch, out_ch)
    if kind == "m2m_in2":
        return "render_wide4_kernel<%d, %d, false, false, false, true" % (in_ch, out_ch)
    if kind == "dmx":
        return ("render_fast_kernel<%d, %d, 0, true" if out_ch <= 2 else
                "render_wide4_kernel<%d, %d, false, false, true") % (in_ch, out_ch)
    if kind == "demix":
        return "render_wide4_kernel<%d, %d, false, true" % (in_ch, out_ch)
    if kind == "h2m_lpcm":
        return "render_fast_kernel<%d, %d, 0, false, false, true" % (in_ch, out_ch)
    if kind == "fir":
        # default: the overlap-save FFT stage as a kernel of its own (the dominant one) + the two-channel matrix kernel over
        # its output; IAMF_HIP_FIR_FUSED: the same stage inside the limiter kernel (3); _F16 / _F32: the MFMA stages (2 / 1)
        for env, st in (("IAMF_HIP_FIR_F32", 1), ("IAMF_HIP_FIR_F16", 2), ("IAMF_HIP_FIR_FUSED", 3)):
            if os.environ.get(env):
                return "render_fast_kernel<%d, 2, %d" % (in_ch, st)
        return ("fir_fft_kernel<%d" % in_ch, "render_fast_kernel<2, 2, 0, false, false")
    if kind == "h2m_lfe":   # render_wide4_kernel<.., LFE>, behind the generator's two kernels (render_lfe.hpp)
        # (the dominant kernel first; the summaries keep 80 characters of a name)
        return ("render_wide4_kernel<%d, %d, true, false, false, false" % (in_ch, out_ch), "lfe_chain_kernel", "lfe_ff_kernel")
    if out_ch <= 2:
        return "render_fast_kernel<%d, %d, 0, false, false" % (in_ch, out_ch)
    # whole 1024-sample chunks of s16: the 4-samples-per-lane kernel (else render_wide_kernel)
    return "render_wide4_kernel<%d, %d" % (in_ch, out_ch)


class Workload:
    """One named workload set up on one device: synthetic element PCM resident in HBM, the batch,
    two PCM buffers, and render_into(buf, events) = ONE launch of the hot path over the batch."""

    def __init__(self, A, name, args, rank, dev):
        self.A, self.name = A, name
        kind, in_id, out_id, in_ch, self.bytes_per_sf = WORKLOADS[name]
        self.kind, self.in_ch, self.in_id, self.out_id = kind, in_ch, in_id, out_id
        self.hrir = self.proj = self.mx = None
        if kind == "fir":
            rng = np.random.default_rng(5)
            hr = (rng.standard_normal((2, in_ch, FIR_TAPS)) * np.exp(-np.arange(FIR_TAPS) / 40.0) * getattr(args, "hrir_scale", HRIR_SCALE_R2)).astype(np.float32)
            mx = A.fir_matrix(hr)
            self.hrir = hr
        elif kind == "dmx":
            mx = A.dmx_matrix(in_id, out_id)
        else:
            mx = A.get_h2m_matrix(in_id, out_id) if kind in ("h2m", "h2m_proj", "h2m_in2", "h2m_lfe", "h2m_lpcm") else A.get_m2m_matrix(in_id, out_id)
        out_ch = self.out_ch = mx.channels if kind == "dmx" else A.layout_channels(out_id)
        self.mx = mx
        S, F, fs = args.streams, args.frames, args.frame_size
        self.S, self.F, self.fs = S, F, fs
        batch = self.batch = A.Batch(S, mx, out_ch, frame_size=fs, out_format=A.FMT_S16, limiter=True,
                                     fir_taps=FIR_TAPS if kind == "fir" else 0, lfe_hoa=kind == "h2m_lfe")
        self.stride_bytes = F * fs * out_ch * 2 + args.pcm_pad_kb * 1024
        self.pcm = [torch.zeros((S, self.stride_bytes), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.stream = torch.cuda.current_stream().cuda_stream
        self.stream_stride, self.frame_stride = F * in_ch * fs + args.pad_kb * 256, in_ch * fs
        self.sf_per_step = S * F * fs     # sample-frames one launch processes on this GPU
        # The element PCM's buffer FIRST, before any other large allocation of this process: which region of
        # memory it lands in decides between two modes of the same kernel (pick_placement).
        if kind == "h2m_proj":   # a well-conditioned Q15 de-mapping matrix (identity/2 + noise)
            rngp = np.random.default_rng(5)
            Pm = rngp.integers(-6000, 6000, size=(in_ch, in_ch)).astype(np.float32) * np.float32(2.0 ** -15)
            Pm[np.arange(in_ch), np.arange(in_ch)] += np.float32(0.5)
            batch.set_projection(Pm.astype(np.float32))
            self.proj = Pm.astype(np.float32)
        self.placement = {"candidates_msamples_s": [], "picked": 0,
                          "note": "no search for this workload / --placement-tries <= 1: the buffers as they came"}
        self.x = None
        self.x_first = None
        self.pcm_first = None
        self.pcm_placement = {"candidate_buffers_msamples_s": [], "picked": [0, 1], "note": "no search: the first two PCM buffers"}
        if args.placement_tries > 1 and kind in ("h2m", "m2m", "fir", "h2m_lfe", "h2m_proj"):
            self.pick_placement(args.placement_tries, dev)
            if args.pcm_placement_tries > 2:
                self.pcm_spacer_gib = max(0, int(args.pcm_spacer_gib))
                self.pick_pcm_placement(args.pcm_placement_tries, dev)

        x = synth_hot_device(S, in_ch, F, fs, 1000 + rank, dev)
        if args.signal == "quiet":
            x = (torch.randn_like(x) * 0.05).contiguous()
        if args.signal == "zero":
            x = torch.zeros_like(x)
        if args.signal == "sparse":
            x = torch.randn_like(x) * 0.05
            tt = torch.arange(F * fs, device=dev).view(1, F, 1, fs)
            ph = (torch.arange(S, device=dev) * 389 % 1531).view(S, 1, 1, 1)
            x += (((tt - ph) % 1531) < 8) * torch.where(tt % 2 == 0, 1.0, -1.0) * 1.5
            x = x.contiguous()
            del tt, ph
        self.extra = None
        self.x2 = None
        if kind in ("h2m_in2", "m2m_in2"):
            batch.set_second_element(A.get_m2m_matrix(A.SS["STEREO"], out_id), [0.7] * S)
            self.x2 = synth_hot_device(S, 2, F, fs, 2000 + rank, dev) * 0.5
            self.extra = self.x2   # any non-None value: the call goes through render_ex
        if kind == "dmx":   # host control plane: a down-mix mode per frame and stream (DMRenderer_set_mode_weight)
            import ctypes as C
            fr_ = (A.DmxFrame * (S * F))()
            st_ = A.DmxState()
            for s_ in range(S):
                A.lib().iamf_hip_dmx_state_init(C.byref(st_))
                A.lib().iamf_hip_dmx_set_mode_weight(C.byref(st_), 1, 3)
                for f_ in range(F):
                    fr_[s_ * F + f_].offset = 0
                    A.lib().iamf_hip_dmx_coefficients(C.byref(st_), fr_[s_ * F + f_].prev)
                    A.lib().iamf_hip_dmx_set_mode_weight(C.byref(st_), (0, 1, 2, 4, 5, 6)[(s_ + f_) % 6], -1)
                    A.lib().iamf_hip_dmx_coefficients(C.byref(st_), fr_[s_ * F + f_].cur)
            self.extra = torch.from_numpy(np.frombuffer(bytes(fr_), dtype=np.uint8).copy()).to(dev)
        if kind == "demix":
            import ctypes as C
            import demix_cases as D
            layers = [1, 3, 7]
            order, _ = D.channels_order(layers)
            rec = D.recon_order(7, D.recon_flags(1, 7))
            batch.set_demixer(7, order, D.output_gain_list(layers, {0: (0b110000, 0.7079458), 1: (0b001111, 1.4125376)}))
            frames_rec = (A.DemixFrame * (S * F))()
            rc = (C.c_int32 * 12)(*rec)
            st = A.DemixState()
            for s_ in range(S):   # host control plane: a demixing mode and recon gains per frame and stream
                A.lib().iamf_hip_demix_state_init(C.byref(st))
                A.lib().iamf_hip_demix_set_info(C.byref(st), 1, 3)
                for f_ in range(F):
                    A.lib().iamf_hip_demix_set_info(C.byref(st), (0, 1, 2, 4, 5, 6)[(s_ + f_) % 6], -1)
                    gains_ = (C.c_float * 12)(*[0.75 + 0.25 * ((s_ * 7 + f_ * 3 + i) % 16) / 15.0 for i in range(len(rec))])
                    A.lib().iamf_hip_demix_frame_fill(C.byref(st), len(rec), rc, gains_, C.byref(frames_rec[s_ * F + f_]))
            self.extra = torch.from_numpy(np.frombuffer(bytes(frames_rec), dtype=np.uint8).copy()).to(dev)
            # The decoded layers are the DOWN-MIX of the programme x (7.1.4 playback order), made with the
            # same per-frame factors the demixer will use (the encoder side of the codec: IAMF spec 7.2),
            # so that what leaves the demixer is the programme every other workload renders.
            raw = np.frombuffer(bytes(frames_rec), dtype=np.float32).reshape(S, F, -1)
            cf = torch.from_numpy(raw[:, :, 5:10].copy()).to(dev).view(S, F, 5, 1)   # cur: alpha beta gamma delta w
            al, be, ga, de = cf[:, :, 0], cf[:, :, 1], cf[:, :, 2], cf[:, :, 3]
            L7, R7, Cc, LFE, SL7, SR7, BL7, BR7, HFL, HFR, HBL, HBR = [x[:, :, i] for i in range(12)]
            SL5, SR5 = al * SL7 + be * BL7, al * SR7 + be * BR7
            L2, R2 = L7 + de * SL5 + 0.707 * Cc, R7 + de * SR5 + 0.707 * Cc
            HL, HR = HFL + ga * HBL, HFR + ga * HBR
            x = torch.stack([L2 / 0.7079458, R2 / 0.7079458, L7, R7, HL / 1.4125376, HR / 1.4125376, Cc, LFE,
                             SL7, SR7, HFL, HFR], dim=2).contiguous()
            del L7, R7, Cc, LFE, SL7, SR7, BL7, BR7, HFL, HFR, HBL, HBR, SL5, SR5, L2, R2, HL, HR
        n = F * in_ch * fs
        self.raw = None
        if kind == "h2m_lpcm":
            # the programme as a 16-bit LPCM stream carries it: one mono sub-stream packet per ambisonics channel and frame
            # (fs x 2 bytes), the packets of a frame one after the other, frames back to back, streams 4 KiB apart like the
            # f32 buffer's.  What the oracle is given (self.x) is the reference's decode of those packets: sample / 32768.
            q = torch.clamp(torch.round(x * 32768.0), -32768, 32767).to(torch.int16)
            self.raw_frame, self.raw_stride = in_ch * fs * 2, F * in_ch * fs * 2 + args.pad_kb * 1024
            self.raw = torch.zeros((S, self.raw_stride), dtype=torch.uint8, device=dev)
            self.raw[:, :F * self.raw_frame] = q.reshape(S, -1).view(torch.uint8)
            x = q.to(torch.float32) * (1.0 / 32768.0)
            L = A.LpcmLayout()
            L.sample_bytes, L.little_endian, L.channels, L.frame_size = 2, 1, in_ch, fs
            for c_ in range(in_ch):
                L.src_offset[c_], L.src_step[c_] = c_ * fs * 2, 2
            self.lpcm_layout = L
            del q
        if self.x is None:
            self.x = torch.zeros((S, self.stream_stride), dtype=torch.float32, device=dev)
        self.x[:, :n] = x.reshape(S, -1)   # into the chosen buffer
        del x
        self.ktag = kernel_tag(kind, in_ch, out_ch)

    def pick_placement(self, tries, dev):
        """Setup, untimed.  The same kernel on the same bytes runs in one of two modes depending on WHICH
        allocation holds the element PCM (tools/debug/placement_probe*.py: e.g. 79 or 91 Gsamples/s quiet, 73 or 86
        hot; not the stride, not the base offset inside the allocation, not the PCM / state buffers; a plain
        streaming read gets 7.0 TB/s from either).  A long-lived serving buffer is allocated once, so the
        harness does what a deployment would: it allocates up to `tries` candidates, measures a few launches
        on each, keeps the fastest and frees the rest.  Every candidate's rate goes into the JSON line."""
        cands, rates = [], []
        need = self.S * self.stream_stride * 4
        for i in range(tries):
            free_b, _total_b = torch.cuda.mem_get_info(dev)
            if i >= 1 and need > free_b // 2:   # bounded: a candidate is only added while it takes less than half of what is free
                break
            cands.append(torch.zeros((self.S, self.stream_stride), dtype=torch.float32, device=dev))  # earlier ones stay alive
            self.x = cands[i]
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4)]
            for a, b in ev:   # on silence: the modes differ by the same ~13 % on any programme
                a.record()
                self.batch.render(self.x.data_ptr(), self.stream_stride, self.frame_stride, self.F,
                                  self.pcm[0].data_ptr(), self.stride_bytes, self.stream)
                b.record()
            torch.cuda.synchronize()
            self.batch.reset()
            ms = float(np.median([a.elapsed_time(b) for a, b in ev[1:]]))
            rates.append(round(self.sf_per_step / (ms * 1e-3) / 1e6, 1))
            if i >= 2 and rates[-1] >= 0.97 * max(rates) and max(rates) > 1.07 * min(rates):
                break   # both modes showed and the current candidate is in the fast one; else all `tries` are looked at
                        # (the first PCM buffer may be of the same kind as every input candidate of a long run, NOTEBOOK.md 3)
        best = int(np.argmax(rates))
        self.x = cands[best]
        self.x_first = cands[0] if best != 0 else None   # what an unsearched deployment gets: timed after the regions
        self.placement = {"candidates_msamples_s": rates, "picked": best,
                          "note": "same kernel on silence, different allocations of the input buffer, tried before "
                                  "anything else is allocated (setup, untimed)"}
        del cands
        torch.cuda.empty_cache()

    def pick_pcm_placement(self, tries, dev):
        """Setup, untimed: the same search for the two PCM output buffers.  What is slow is a PAIR: an input region and an
        output region of the same kind (tools/debug/placement_va_probe.hip `out`: every input buffer is slow with one group of
        output buffers and fast with the other, or fast with both — NOTEBOOK.md 3), and the timed region alternates
        between two PCM buffers, so BOTH have to suit the chosen input.  Candidates are therefore pairs: the two buffers
        already allocated, and `tries` - 1 more, each pair ONE allocation cut in two (neighbours share their kind of region;
        with single buffers as candidates a run found one fast buffer among six and timed every other step on a slow one).
        The chosen input, silence; the pair whose slower half is fastest stays."""
        def rate(buf):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4)]
            for a, b in ev:
                a.record()
                self.batch.render(self.x.data_ptr(), self.stream_stride, self.frame_stride, self.F,
                                  buf.data_ptr(), self.stride_bytes, self.stream)
                b.record()
            torch.cuda.synchronize()
            self.batch.reset()
            ms = float(np.median([a.elapsed_time(b) for a, b in ev[1:]]))
            return round(self.sf_per_step / (ms * 1e-3) / 1e6, 1)

        # Round 4, late: what is fast or slow is ONE output buffer with the chosen input, and which of the two it is changes
        # from one 128 MiB allocation to the next (tools/debug/pcm_offset_probe.py: the first two PCM buffers of a process
        # measured 88.1 / 76.8 on one card, 80.0 / 88.9 on another; offsets inside an arena, or 12 GiB spacers between
        # candidates, change nothing) — roughly one allocation in six to twelve lands in a region of another kind than the
        # input's.  So the candidates are SINGLE buffers, up to 8 x `tries` of them, kept alive while the search runs; the
        # two fastest become the PCM double buffer.  (What a deployment does once for its long-lived output ring.)
        singles = list(self.pcm)
        rates = [rate(b) for b in singles]
        limit = 8 * max(1, tries)
        need = self.S * self.stride_bytes
        while len(singles) < limit:
            fast = sorted(rates, reverse=True)
            if len(fast) >= 2 and fast[1] > 1.07 * min(rates):
                break   # two buffers of the fast kind
            if len(rates) >= 12 and max(rates) < 1.04 * min(rates):
                break   # a dozen allocations, one kind: on this card the output's placement is not what decides
            free_b, _total_b = torch.cuda.mem_get_info(dev)
            if need > free_b // 4 or (len(singles) + 1) * need > (32 << 30):
                break   # bounded: the candidates stay alive while the search runs (cfg3's buffers are 6 GiB each)
            try:
                singles.append(torch.zeros((self.S, self.stride_bytes), dtype=torch.uint8, device=dev))
            except torch.OutOfMemoryError:
                break
            rates.append(rate(singles[-1]))
        order = list(np.argsort(rates)[::-1][:2])
        if sorted(order) != [0, 1]:
            self.pcm_first = [singles[0], singles[1]]
        self.pcm = [singles[int(order[0])], singles[int(order[1])]]
        self.pcm_placement = {"candidate_buffers_msamples_s": rates, "picked": [int(v) for v in order],
                              "note": "single 128 MiB output buffers with the chosen input, the two fastest kept"}
        pairs, spacers = singles, None
        del pairs, spacers
        torch.cuda.empty_cache()

    def render_into(self, buf, ev_pair=None):
        # events bracket only the render kernel (recorded on the stream it is launched on); the
        # gather runs on RCCL's own stream
        A, kind = self.A, self.kind
        if ev_pair:
            ev_pair[0].record()
        if kind == "h2m_lpcm":
            inp, a = A.LpcmInput(), A.RenderArgs()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride = self.raw.data_ptr(), self.raw_stride, self.raw_frame
            inp.layout = self.lpcm_layout
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = self.F, buf.data_ptr(), self.stride_bytes, self.stream
            n = self.batch.render_lpcm(inp, a)
        elif self.extra is not None:
            a = A.RenderArgs()
            a.d_in, a.in_stream_stride, a.in_frame_stride = self.x.data_ptr(), self.stream_stride, self.frame_stride
            a.n_frames, a.d_pcm, a.pcm_stream_stride_bytes, a.stream = self.F, buf.data_ptr(), self.stride_bytes, self.stream
            if kind in ("h2m_in2", "m2m_in2"):
                a.d_in2, a.in2_stream_stride, a.in2_frame_stride = self.x2.data_ptr(), self.F * 2 * self.fs, 2 * self.fs
            elif kind == "dmx":
                a.d_dmx_frames = self.extra.data_ptr()
            else:
                a.d_demix_frames = self.extra.data_ptr()
            n = self.batch.render_ex(a)
        else:
            n = self.batch.render(self.x.data_ptr(), self.stream_stride, self.frame_stride, self.F,
                                  buf.data_ptr(), self.stride_bytes, self.stream)
        if ev_pair:
            ev_pair[1].record()
        self.last_n = n
        return n

    def dump_outputs(self, buf, out_dir, budget_bytes=60_000_000):
        """What the last launch gave its caller: the packed s16 PCM of every stream, `last_n` sample-frames x out_ch.
        Written as DIR/pcm.npy, float32 [streams, sample-frames, out_ch] holding the int16 values exactly, for a fixed
        seeded sample of the streams that keeps the file under `budget_bytes` (all of them when they fit), and
        DIR/pcm_streams.npy, float64, the stream indices of that sample."""
        n, ch = self.last_n, self.out_ch
        per_stream = n * ch * 4
        k = min(self.S, max(1, budget_bytes // per_stream))
        n_kept = min(n, budget_bytes // (ch * 4))   # only when one stream alone is over the budget: its first samples
        ids = np.arange(self.S) if k == self.S else np.sort(np.random.default_rng(0).choice(self.S, k, replace=False))
        rows = buf[torch.from_numpy(ids).to(buf.device), :n_kept * ch * 2].cpu().numpy()
        pcm = rows.view(np.int16).reshape(k, n_kept, ch).astype(np.float32)
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "pcm.npy"), pcm)
        np.save(os.path.join(out_dir, "pcm_streams.npy"), ids.astype(np.float64))
        return {"dir": out_dir, "pcm": list(pcm.shape), "streams_of": self.S, "sample_frames_of": n}

    def verify(self, k=4):
        """After the timed regions: reset the stream state, render ONE more launch of exactly the timed geometry
        (same buffers, padded strides, F frames, all S streams) and compare k streams' PCM with the oracle on
        the host (tests/bench_verify.py; the oracle is the checker here, never the thing measured).  Bit-exact
        where the product's contract is bit-exact, +-1 LSB for the MFMA projection, and for the HRTF stage (parity
        unpinned) the stage's own f32 output against this repo's float64 specification (2^-17) plus the oracle's
        limiter + pack on that output against the PCM, bit for bit.  Returns the `verified` entry; ok=False
        fails the run."""
        import bench_verify as V
        A, kind, S, F, fs = self.A, self.kind, self.S, self.F, self.fs
        if kind in ("h2m_in2", "m2m_in2"):
            return None   # the two-element workloads are not in the default line; tests/test_gpu_extras.py checks them
        self.batch.reset()
        buf = self.pcm[0]
        buf.zero_()
        n = self.render_into(buf)
        torch.cuda.synchronize()
        if n != F * fs - 240:
            return {"ok": False, "why": "first launch after a reset emitted %d sample-frames, not %d" % (n, F * fs - 240)}
        picks = sorted({int(round(i * (S - 1) / max(1, k - 1))) for i in range(k)}) if k > 1 else [0]   # spread over the shard
        nfl = F * self.in_ch * fs
        xs = {s_: self.x[s_, :nfl].cpu().numpy().reshape(F, self.in_ch, fs) for s_ in picks}
        got = {s_: buf[s_, :n * self.out_ch * 2].cpu().numpy().view(np.int16).reshape(n, self.out_ch) for s_ in picks}
        tol = V.tolerance_lsb(kind, self.out_ch)
        res = {"streams": len(picks), "stream_ids": picks, "sample_frames_each": n, "tolerance_lsb": tol,
               "against": "oracle/ (CPU restatement pinned to the reference)", "geometry": "the timed launch: %d streams x %d "
               "frames, stream stride %d floats, pcm stride %d bytes" % (S, F, self.stream_stride, self.stride_bytes)}
        worst, frac, ok = 0, 0.0, True
        if kind == "fir":
            # the FIR stage's own output for the same streams: a k-stream batch with a threshold nothing reaches
            # (+60 dB: gain exactly 1) and float output; render + flush = all F*fs stage samples
            vb = A.Batch(len(picks), self.mx, 2, frame_size=fs, out_format=A.FMT_F32, limiter=True,
                         threshold_db=60.0, fir_taps=FIR_TAPS)
            xin = torch.stack([self.x[s_, :nfl] for s_ in picks]).contiguous()
            o1 = torch.zeros((len(picks), F * fs * 2), dtype=torch.float32, device=xin.device)
            o2 = torch.zeros((len(picks), 240 * 2), dtype=torch.float32, device=xin.device)
            n1 = vb.render(xin.data_ptr(), nfl, self.in_ch * fs, F, o1.data_ptr(), F * fs * 8, self.stream)
            n2 = vb.flush(o2.data_ptr(), 240 * 8, self.stream)
            torch.cuda.synchronize()
            vb.close()
            err = 0.0
            for i, s_ in enumerate(picks):
                y_stage = np.concatenate([o1[i, :n1 * 2].cpu().numpy().reshape(n1, 2), o2[i, :n2 * 2].cpu().numpy().reshape(n2, 2)])
                y64 = V.fir64(self.hrir, V.planar(xs[s_]))
                e = float(np.abs(y_stage.T - y64).max() / max(1.0, float(np.abs(y64).max())))
                err = max(err, e)
                o, w, fr = V.compare(got[s_], V.fir_pcm_from_stage(y_stage, fs, F), 0)
                ok = ok and o and e <= 2.0 ** -17
                worst, frac = max(worst, w if w is not None else 1 << 30), max(frac, fr or 0.0)
            res.update({"against": "this repo's float64 HRTF specification (parity unpinned) for the FIR stage; oracle/ limiter + "
                        "pack on the stage's own output for the PCM", "fir_stage_max_rel_err": err, "fir_stage_tolerance": 2.0 ** -17})
        else:
            for s_ in picks:
                want = V.oracle_pcm(kind, self.in_id, self.out_id, self.out_ch, xs[s_], fs, s_, proj=self.proj)
                o, w, fr = V.compare(got[s_], want, tol)
                ok = ok and o
                worst, frac = max(worst, w if w is not None else 1 << 30), max(frac, fr or 0.0)
        res.update({"ok": bool(ok), "max_lsb": worst, "max_fraction_differing": round(frac, 6)})
        return res

    def same_traffic_no_compute(self, reps=8):
        """What the memory system delivers for THIS workload's traffic shape on THESE buffers with no compute:
        the library's diagnostic kernel (iamf_probe.hip: one workgroup per stream, in_ch x 16 B read and
        out_ch / 2 x 16 B written per lane and chunk), timed like the render kernel.  Runs after the timed
        regions (it overwrites the PCM buffer).  None where the shape has no probe (odd channel counts)."""
        A = self.A
        if self.fs != 1024 or self.out_ch % 2 and self.out_ch != 1 or self.kind == "h2m_lpcm":   # (the probe reads 16-byte pieces)
            return None
        rows, pieces = self.in_ch, max(1, self.out_ch // 2)
        in_stride_b = self.stream_stride * 4
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            r = A.lib().iamf_hip_probe_traffic(self.S, self.F, rows, pieces, self.x.data_ptr(), in_stride_b,
                                               self.pcm[1].data_ptr(), self.stride_bytes, self.stream)
            b.record()
            if r != 0:
                return None
        torch.cuda.synchronize()
        ms = float(np.median([a.elapsed_time(b) for a, b in ev[2:]]))
        bytes_ = self.S * self.F * (rows + pieces) * 4096
        return {"msamples_s": round(self.sf_per_step / (ms * 1e-3) / 1e6, 1), "gbs": round(bytes_ / (ms * 1e-3) / 1e9, 1),
                "kernel_ms": round(ms, 4), "note": "same loads and stores per lane and chunk, same buffers, no compute"}

    def close(self):
        self.batch.close()
        self.x = self.x2 = self.extra = self.pcm = self.x_first = self.pcm_first = None
        torch.cuda.empty_cache()

    def roofline(self, kernel_ms):
        """the dominant kernel's roofline entry from its mean launch duration (HIP events)"""
        achieved = self.bytes_per_sf * self.sf_per_step / (kernel_ms * 1e-3) / 1e9
        traffic = measured_traffic(self.ktag, self.sf_per_step, self.name)
        mfma = measured_mfma(self.name, self.ktag)
        r = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": round(achieved / HBM_PEAK_GBS, 4),
             "traffic": round(traffic[0]) if traffic else None,
             "traffic_unit": "HBM bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)",
             "traffic_source": traffic[1] if traffic else None,
             "algorithmic_bytes_per_launch": self.bytes_per_sf * self.sf_per_step,
             "kernel": self.ktag if isinstance(self.ktag, str) else self.ktag[0], "kernel_ms": round(kernel_ms, 4),
             "algorithmic_bytes_per_sample_frame": self.bytes_per_sf,
             "frac_of_measured_copy_6290": round(achieved / 6290.0, 4)}
        if mfma:   # north_star: "MFMA utilisation on the HOA path" — the projection runs on the f32 matrix cores (cfg3)
            r["mfma"] = mfma
        dtype = "f32"
        if not isinstance(self.ktag, str):
            r["kernels"] = list(self.ktag)
            r["kernel_ms_spans"] = ("the %d kernels of one call, back to back on the stream (HIP events around the call); their "
                                    "separate durations: profiles/*_%s_pmc.json" % (len(self.ktag), self.name))
        if self.kind == "fir":
            # Three stages, one specification (render_fir.hpp).  Default: overlap-save FFT on the VALU (render_fir_fft.hpp):
            # ~770 flop per sample-frame -> the stage is no longer the bound by count; the kernel's bound is HBM (68 B per
            # sample-frame, as for the matrix form).  Reported against BOTH: 8 TB/s (`frac`) and the f32 vector peak for the
            # flops the algorithm issues (`valu`).  IAMF_HIP_FIR_F16 / _F32 select the direct-form MFMA stages (r2).
            flop_direct = 2 * self.in_ch * 2 * FIR_TAPS
            f32_stage, f16_stage = bool(os.environ.get("IAMF_HIP_FIR_F32")), bool(os.environ.get("IAMF_HIP_FIR_F16"))
            rate = self.sf_per_step / (kernel_ms * 1e-3)
            if not (f32_stage or f16_stage):
                pairs = (self.in_ch + 1) // 2
                n, hop = 1024, 768
                flop_fft = (pairs + 1) * 5 * n * 10 + pairs * 2 * 8 * n      # (pairs + 1) transforms + 2 complex MACs per bin and pair
                flop_sf = flop_fft / hop
                tf = flop_sf * rate / 1e12
                dtype = "f32 (overlap-save FFT on the VALU, f32 accumulate)"
                r.update({"valu": {"achieved_tflops": round(tf, 2), "peak_tflops": F32_VALU_PEAK_TFLOPS,
                                   "frac": round(tf / F32_VALU_PEAK_TFLOPS, 4), "flop_per_sample_frame": round(flop_sf, 1),
                                   "note": "1024-point transforms, 768-sample hops, two channels per complex transform"},
                          "direct_form_equivalent_tflops": round(flop_direct * rate / 1e12, 1),
                          "direct_form_flop_per_sample_frame": flop_direct,
                          "note": "bound = HBM by count (68 B per sample-frame + 16 for y between the two kernels): the FFT stage "
                                  "issues %.0f flop per sample-frame where the direct form needs %d; what limits it as measured: "
                                  "the stage kernel's VALU issue at 2 waves per SIMD (~240 VGPRs) and the limiter kernel's chain "
                                  "(NOTEBOOK.md 4.2c)" % (flop_sf, flop_direct)})
            else:
                tf = flop_direct * rate / 1e12
                peak = F32_MFMA_PEAK_TFLOPS if f32_stage else F16_MFMA_PEAK_TFLOPS
                r.update({"bound": "mfma", "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s",
                          "frac": round(tf / peak, 4), "algorithmic_flop_per_sample_frame": flop_direct,
                          "hbm_gbs": round(achieved, 1)})
                if f32_stage:
                    dtype = "f32 (f32 MFMA)"
                else:   # render_fir16.hpp: three f16 MFMAs per block of products, 288 of 256 taps multiplied
                    issued = tf * 3 * 288 / 256
                    dtype = "f32 via split f16 (hi/lo halves, three f16 MFMAs, f32 accumulate)"
                    r.update({"issued_tflops": round(issued, 1), "frac_issued": round(issued / peak, 4)})
        return r, dtype


def timed_region(wl, pipe, steps, world, dist):
    """EXACTLY `steps` launches between barrier + synchronize on both sides.
    Returns (wall seconds on this rank, mean kernel ms from the HIP events, sample-frames emitted per stream)."""
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    emitted = 0
    t0 = time.perf_counter()
    for i in range(steps):
        emitted += pipe.step(lambda buf, i=i: wl.render_into(buf, ev[i]))
    pipe.drain()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    return elapsed, kernel_ms, emitted


def device_info():
    """What rocm-smi says about this rank's card (memory vendor and clocks): the render kernels' rate differs by
    ~13 % between MI355X devices (NOTEBOOK.md 5), and this is what can be read in-band about the one measured."""
    import subprocess
    if "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or any("ROCPROF" in k.upper() for k in os.environ):
        # the profiler's preloaded library has initialised the GPU before this process started: no fork + exec here
        return {"skipped": "under rocprofv3 (see the unprofiled run's read-out)"}
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showmemvendor", "--showtemp", "--showpower",
                              "--showcomputepartition", "--showmemorypartition", "--json"],
                             capture_output=True, text=True, timeout=20).stdout
        d = json.loads(out[out.index("{"):])
        card = d.get("card%d" % int(os.environ.get("LOCAL_RANK", "0")), next(iter(d.values())))
        info = {"memory_vendor": card.get("GPU memory vendor"), "mclk": card.get("mclk clock speed:"),
                "fclk": card.get("fclk clock speed:"), "sclk_now": card.get("sclk clock speed:")}
        for k, v in card.items():
            if "emperature" in k or "ower" in k or "artition" in k:
                info[k.strip(" :")] = v
        return info
    except Exception as e:   # noqa: BLE001 — a diagnostic, never a reason to fail the bench
        return {"error": str(e)[:80]}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="launches in each timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5,
                    help="timed regions of --steps launches each; value is the MEDIAN region, all are listed")
    ap.add_argument("--streams", type=int, default=512, help="streams per GPU")
    ap.add_argument("--frames", type=int, default=64, help="frames per stream per step")
    ap.add_argument("--frame-size", type=int, default=1024)
    ap.add_argument("--workload", default="toa_binaural_limiter_s16", choices=sorted(WORKLOADS))
    ap.add_argument("--signal", default="hot", choices=sorted(SIGNALS),
                    help="hot: the limiter re-triggers in almost every 64-sample block; quiet: never; sparse: a "
                         "quiet programme with a short peak every ~1500 samples (one or two isolated trigger runs per chunk)")
    ap.add_argument("--gather", default="final", choices=["final", "step", "none"],
                    help="N>1: gather packed PCM to rank 0 over RCCL once after the last step (default, the "
                         "job's one exchange), after every step (overlapped with the next render), or never")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-facade", action="store_true", help="skip the IAMF_decoder.h facade rates (single handle / group of 64)")
    ap.add_argument("--no-verify", action="store_true",
                    help="skip the oracle check of one more launch of the timed geometry (the `verified` entry)")
    ap.add_argument("--rehearse-one-gpu", action="store_true",
                    help="development only: run the N > 1 control flow (launcher, barriers, max over ranks, gather, the "
                         "JSON line) with every rank on GPU 0 and gloo instead of RCCL, which refuses two ranks on one "
                         "device.  The line is marked `rehearsal` and its value means nothing")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="N=1, default workload: do not also measure BASELINE configs 2, 3 and the HRTF form of 4")
    ap.add_argument("--placement-tries", type=int, default=8,
                    help="setup: allocate up to this many candidate buffers for the element PCM, measure a few "
                         "launches on each and keep the fastest (the rate is bimodal per allocation, ~13 %% apart; "
                         "1 = take the first allocation as it comes)")
    ap.add_argument("--pcm-spacer-gib", type=int, default=12,
                    help="setup: untouched bytes allocated between two PCM placement candidates, so that the candidates "
                         "walk across the card's kinds of memory region (runs of 8-16 GB)")
    ap.add_argument("--pcm-placement-tries", type=int, default=6,
                    help="setup: candidates for the two PCM output buffers, tried with the chosen input (see "
                         "--placement-tries; 2 = keep the first two allocations)")
    ap.add_argument("--hrir-scale", type=float, default=HRIR_SCALE_R2,
                    help="tap scale of the synthetic HRIR set of the HRTF workload (0.08: per-ear gain 1.49, the set of rounds "
                         "1-2; 0.0481: the gain of the reference's TOA -> binaural matrix)")
    ap.add_argument("--pcm-pad-kb", type=int, default=0,
                    help="the same stagger for the streams' PCM output regions (stream stride = the call's bytes + this)")
    ap.add_argument("--pad-kb", type=int, default=4,
                    help="stagger the streams' input regions: stream stride = frames * channels * frame size "
                         "+ this many KiB, so that the workgroups, which advance in step, are not all on the "
                         "same HBM channel at once (0 = the power-of-two stride: -12 %% on the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed regions, write what the headline workload's last timed launch computed (rank 0's "
                         "packed PCM, a fixed sample of streams as float32: DIR/pcm.npy, DIR/pcm_streams.npy) so that two "
                         "builds can be compared output for output")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    from iac_amd import launch
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.gpus > 1 and not launch.under_launcher():
        # `python bench.py --gpus N` with no launcher around it: THIS process becomes the launcher.
        # It has made no GPU call (torch is imported, nothing under torch.cuda was called, the HIP
        # library is not loaded) and makes none: it starts N fresh rank processes, relays rank 0's
        # line and exits non-zero if any rank failed.
        child = os.environ.get("IAMF_BENCH_CHILD")   # test hook: a stub rank program
        argv = ([sys.executable, child] if child else [sys.executable, os.path.abspath(__file__)]) + sys.argv[1:]
        raise SystemExit(launch.launch_ranks(args.gpus, argv))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: refusing to measure a different job than the one asked for"
                         % (args.gpus, world))
    # rocm-smi is a program of its own: start it BEFORE this process touches the GPU (a process that has initialised the
    # GPU must not fork + exec on this pool; under rocprofv3 the box refuses it)
    dev_info = device_info() if rank == 0 else None
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the renderer has no CPU path")
    rehearse = bool(args.rehearse_one_gpu)
    dev_index = 0 if rehearse else local_rank
    if torch.cuda.device_count() <= dev_index:
        raise SystemExit("rank %d: LOCAL_RANK %d but only %d GPU(s) visible" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    ranks_seen, rccl = 1, None
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        ranks_seen = dist.get_world_size()
        try:
            rccl = None if rehearse else ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl = "unknown"
        # every rank must sit on its own device: gather (device index, PCI bus id) and compare
        mine = torch.tensor([dev_index], dtype=torch.int64, device="cpu" if rehearse else dev)
        seen = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(seen, mine)
        devices_seen = sorted(int(t.item()) for t in seen)
        if len(set(devices_seen)) != world and not rehearse:
            raise SystemExit("ranks share a device: %s" % devices_seen)

    def gather_to_rank0(t, recv):   # gloo (the rehearsal) moves CPU tensors only
        if rehearse:
            dist.gather(t.cpu(), recv if rank == 0 else None, dst=0)
        else:
            dist.gather(t, recv if rank == 0 else None, dst=0)

    import iac_amd as A
    from iac_amd.sharding import GatherPipeline
    wl = Workload(A, args.workload, args, rank, dev)
    S, F, fs = wl.S, wl.F, wl.fs
    pipe = GatherPipeline(wl.pcm, world, rank, enabled=world > 1 and args.gather == "step" and not rehearse)
    final_recv = None
    if world > 1 and args.gather == "final" and rank == 0:
        final_recv = [torch.empty_like(wl.pcm[0], device="cpu" if rehearse else dev) for _ in range(world)]

    for i in range(args.warmup):
        pipe.step(wl.render_into)
    pipe.drain()
    if world > 1 and args.gather == "final":   # untimed: sets up RCCL's point-to-point connections
        gather_to_rank0(wl.pcm[0], final_recv)

    regions = []
    # one region more than reported: the first one runs on clocks that have just come up from idle (sclk reads 158 MHz
    # between regions) and is dropped — listed as repeats.discarded_first_ms_per_step, never the reported value
    discarded = None
    for r in range(max(1, args.repeats) + 1):
        elapsed, kernel_ms, emitted = timed_region(wl, pipe, args.steps, world, dist)
        if r == 0:
            discarded = elapsed
            continue
        assert emitted >= args.steps * F * fs - 240, "every step must emit its F*fs sample-frames per stream"
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearse else dev)
        if world > 1:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)   # the slowest rank's time
        regions.append((float(tmax.item()), kernel_ms))
    gather_ms = None
    if world > 1 and args.gather == "final":
        # the job's one exchange: every rank's packed PCM of the last step -> rank 0 (RCCL over xGMI).
        # It happens once per job whatever the number of steps, so it is timed on its own and
        # reported beside the K-step rate instead of being folded into it.
        tg = time.perf_counter()
        gather_to_rank0(wl.pcm[(args.steps * (len(regions) + 1) - 1) % 2], final_recv)
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - tg) * 1e3
        if rank == 0:   # what arrived from rank r is rank r's PCM, not a copy of ours: ranks render different seeds
            same = sum(int(torch.equal(final_recv[r], final_recv[0])) for r in range(1, world))
            assert same == 0, "gather delivered identical PCM from %d other rank(s)" % same

    dumped = None
    if args.dump_outputs and rank == 0:   # before anything else renders into the PCM buffers
        dumped = wl.dump_outputs(pipe.buffers[(pipe.i - 1) % 2], args.dump_outputs)

    first_alloc = None
    if world == 1 and (wl.x_first is not None or wl.pcm_first is not None):
        # what a deployment that takes its buffers as hipMalloc hands them out gets: one more region on the FIRST
        # input allocation and the FIRST two PCM buffers (same programme copied over), beside the searched placement
        keep_x, keep_pcm = wl.x, wl.pcm
        if wl.x_first is not None:
            wl.x_first.copy_(wl.x)
            wl.x = wl.x_first
        if wl.pcm_first is not None:
            wl.pcm = wl.pcm_first
        p1 = GatherPipeline(wl.pcm, 1, 0, enabled=False)
        for i in range(max(1, args.warmup)):
            p1.step(wl.render_into)
        p1.drain()
        el1, k1, _ = timed_region(wl, p1, args.steps, 1, dist)
        first_alloc = {"value": round(wl.sf_per_step * args.steps / el1 / 1e6, 2), "kernel_ms": round(k1, 4),
                       "note": "same job on the first input allocation and the first two PCM buffers as they came (no search)"}
        wl.x, wl.pcm = keep_x, keep_pcm
    verified = None
    if not args.no_verify:
        verified = wl.verify()
        if verified is not None and not verified.get("ok"):
            raise SystemExit("rank %d: the timed geometry's PCM differs from the oracle: %s" % (rank, json.dumps(verified)))

    if rank == 0:
        order = sorted(range(len(regions)), key=lambda i: regions[i][0])
        med = order[len(order) // 2]     # the median region is the one reported (upper median for even counts)
        elapsed, kernel_ms = regions[med]
        total_sf = wl.sf_per_step * args.steps * world
        value = total_sf / elapsed / 1e6
        roof, dtype = wl.roofline(kernel_ms)
        if wl.kind in ("h2m", "m2m", "h2m_proj"):
            probe = wl.same_traffic_no_compute()
            if probe:
                roof["same_traffic_no_compute"] = probe
                # kernel time against kernel time (this GPU's launch): how much of what the memory system
                # gives this traffic shape the render kernel gets
                roof["frac_of_same_traffic"] = round(wl.sf_per_step / (kernel_ms * 1e-3) / 1e6 / probe["msamples_s"], 4)
        out = {
            "metric": "Msamples/s rendered (3rd-order HOA->binaural, 48 kHz)",
            "metric_note": "value: buffers picked at setup among <= %d input / %d PCM allocations (config.input_placement); "
                           "value_first_allocation: the buffers as they came" % (args.placement_tries, args.pcm_placement_tries),
            "value": round(value, 2), "unit": "Msamples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype,
            "data": "synthetic",
            "x_realtime": round(value / 0.048, 1),
            "ranks_seen": ranks_seen, "rccl_version": rccl,
            "launched_by": os.environ.get("IAMF_LAUNCHED_BY", "torchrun" if "TORCHELASTIC_RUN_ID" in os.environ else "direct"),
            "device": dev_info,
            "value_min": round(total_sf / max(e for e, _ in regions) / 1e6, 2),
            "value_max": round(total_sf / min(e for e, _ in regions) / 1e6, 2),
            "repeats": {"n": len(regions), "steps_each": args.steps, "reported": "median",
                        "discarded_first_ms_per_step": None if discarded is None else round(discarded / args.steps * 1e3, 4),
                        "ms_per_step": [round(e / args.steps * 1e3, 4) for e, _ in regions],
                        "value_min": round(total_sf / max(e for e, _ in regions) / 1e6, 2),
                        "value_median": round(value, 2),
                        "value_max": round(total_sf / min(e for e, _ in regions) / 1e6, 2),
                        "kernel_ms": [round(k, 4) for _, k in regions]},
            "config": {"workload": args.workload, "streams_per_gpu": S, "frames_per_step": F,
                       "frame_size": fs, "sample_rate": 48000, "in_channels": wl.in_ch,
                       "out_channels": wl.out_ch, "pcm": "s16", "limiter": "-1 dBFS, 240 look-ahead",
                       "signal": SIGNALS[args.signal], "parallelism": "streams sharded, dp%d" % world,
                       "input_stagger_kib": args.pad_kb, "input_placement": wl.placement,
                       "pcm_placement": wl.pcm_placement,
                       "gather": args.gather if world > 1 else "n/a (1 GPU)"},
            "gather_ms": None if gather_ms is None else round(gather_ms, 3),
            "gather_bytes_per_rank": wl.stride_bytes * S if world > 1 and args.gather == "final" else None,
            "roofline": roof,
            "verified": verified,
            "value_first_allocation": first_alloc["value"] if first_alloc else round(value, 2),
            "dumped_outputs": dumped,
            "first_allocation": first_alloc or {"note": "the search kept the first allocations: value is the unsearched rate"},
        }
        try:   # the C-side multi-device entry (include/iamf_hip.h iamf_hip_shard_*) finds its RCCL by dlopen
            out["c_abi_shard"] = {"rccl_version": A.lib().iamf_hip_shard_rccl_version().decode() or None,
                                  "note": "iamf_hip_shard_create / _render / _gather: one process, one batch + host thread + two "
                                          "streams per device; exercised on one device by tests/test_gpu_shard.py"}
        except Exception as e:   # noqa: BLE001
            out["c_abi_shard"] = {"error": str(e)[:120]}
        if wl.kind == "fir":
            out["config"]["parity"] = "unpinned (HRTF arithmetic is not in the reference tree)"
        if rehearse:
            out["rehearsal"] = "all %d ranks on GPU 0 over gloo: the control flow of the N > 1 path only, the value means nothing" % world
            out["data"] = "REHEARSAL - not a measurement"
        if out["n_gpus"] != args.gpus:   # cannot happen past the check above; never print a line for another job
            raise SystemExit("n_gpus %d != --gpus %d" % (out["n_gpus"], args.gpus))
    headline_kind = wl.kind
    wl.close()

    if rank == 0 and world == 1 and args.workload == "toa_binaural_limiter_s16" and not args.no_extra_configs:
        # BASELINE configs 2, 3 and the HRTF form of 4 in the same process, same harness, one region each
        out["configs"] = {}
        import copy
        for name, streams2, tries2 in EXTRA_CONFIGS:
            a2 = copy.copy(args)
            a2.streams, a2.placement_tries = streams2, tries2
            w2 = Workload(A, name, a2, rank, dev)
            p2 = GatherPipeline(w2.pcm, 1, 0, enabled=False)
            for i in range(args.warmup):
                p2.step(w2.render_into)
            el, kms, em = timed_region(w2, p2, args.steps, 1, dist)
            assert em >= args.steps * w2.F * w2.fs - 240
            v2 = w2.sf_per_step * args.steps / el / 1e6
            r2, dt2 = w2.roofline(kms)
            if w2.kind in ("h2m", "m2m"):
                pr2 = w2.same_traffic_no_compute()
                if pr2:
                    r2["same_traffic_no_compute"] = pr2
                    r2["frac_of_same_traffic"] = round(w2.sf_per_step / (kms * 1e-3) / 1e6 / pr2["msamples_s"], 4)
            out["configs"][name] = {"value": round(v2, 2), "unit": "Msamples/s", "steps": args.steps,
                                    "streams_per_gpu": streams2, "frames_per_step": w2.F,
                                    "ms_per_step": round(el / args.steps * 1e3, 4), "dtype": dt2,
                                    "in_channels": w2.in_ch, "out_channels": w2.out_ch,
                                    "input_placement": w2.placement, "pcm_placement": w2.pcm_placement, "roofline": r2}
            if w2.kind == "fir":
                out["configs"][name]["parity"] = "unpinned (HRTF arithmetic is not in the reference tree)"
                out["configs"][name]["hrir_scale"] = args.hrir_scale
            if not args.no_verify:
                v2_ = w2.verify()
                out["configs"][name]["verified"] = v2_
                if v2_ is not None and not v2_.get("ok"):
                    raise SystemExit("%s: the timed geometry's PCM differs from the oracle: %s" % (name, json.dumps(v2_)))
            w2.close()
            if w2.kind == "fir" and args.hrir_scale == HRIR_SCALE_R2:
                # The synthetic HRIR set of rounds 1-2 has a per-ear gain of 1.49 (the reference's TOA -> binaural matrix:
                # 0.895), so behind it the programme's noise floor crosses the limiter's threshold in nearly every 240-sample
                # window and the limiter holds the gain down the whole time; in the headline it does so in the bursts only.
                # The same job with the set scaled to the matrix's gain, beside it (a second data point, not the config's value).
                a3 = copy.copy(a2)
                a3.hrir_scale = HRIR_SCALE_R2 * 0.895 / 1.487
                w3 = Workload(A, name, a3, rank, dev)
                p3 = GatherPipeline(w3.pcm, 1, 0, enabled=False)
                for i in range(args.warmup):
                    p3.step(w3.render_into)
                el3, kms3, em3 = timed_region(w3, p3, args.steps, 1, dist)
                e3 = {"value": round(w3.sf_per_step * args.steps / el3 / 1e6, 2), "ms_per_step": round(el3 / args.steps * 1e3, 4),
                      "hrir_scale": round(a3.hrir_scale, 5),
                      "note": "HRIR set scaled to the per-ear gain of the reference's TOA -> binaural matrix (0.895): the limiter "
                              "works in the bursts, as in the headline"}
                if not args.no_verify:
                    e3["verified"] = w3.verify()
                    if e3["verified"] is not None and not e3["verified"].get("ok"):
                        raise SystemExit("%s at the headline's level: PCM differs: %s" % (name, json.dumps(e3["verified"])))
                out["configs"][name]["at_the_headline_level"] = e3
                w3.close()

    if rank == 0:
        kind = headline_kind
        if not args.no_cpu_baseline and world == 1:   # rank 0 at N = 1 only: the other ranks would wait for it
            wlname = {"fir": "toa_binaural_limiter_s16", "demix": "714_ssJ_limiter_s16"}.get(kind, args.workload)
            wlname = wlname.replace("toa_projection_", "toa_").replace("_lfe_", "_")
            if kind in ("dmx", "m2m_in2"):
                wlname = "714_ssJ_limiter_s16"
            if kind == "h2m_in2":
                wlname = "toa_binaural_limiter_s16"
            refb = reference_baseline(wlname, fs)
            port = cpu_baseline(wlname, fs, seconds_target=6.0 if refb else 12.0)
            if refb:   # the reference itself is the baseline; the oracle port is reported beside it
                refb["oracle_port"] = {k: port[k] for k in ("value", "unit", "cores", "single_core_value")}
            out["cpu_baseline"] = refb or port
            notes = {"fir": " [the matrix binaural path: the reference has no buildable HRTF]",
                     "demix": " [the single-layer 7.1.4 stream: without the demixer stage]",
                     "dmx": " [the 7.1.4 -> J matrix stream: the reference's down-mixer needs a demixing-parameter stream]",
                     "h2m_in2": " [the one-element stream: without the stereo element]",
                     "m2m_in2": " [the one-element stream: without the stereo element]",
                     "h2m_proj": " [the mono-mode stream: without the de-mapping stage]",
                     "h2m_lfe": " [the default reference build: LFE generator compiled out]"}
            out["cpu_baseline"]["sample"] += notes.get(kind, "")
            if args.workload == "toa_binaural_limiter_s16" and not args.no_facade:
                try:
                    fr = facade_rates(fs)
                    fr["reference_single_core_msamples_s"] = out["cpu_baseline"].get("single_core_value")
                    out["facade"] = fr
                except Exception as e:   # noqa: BLE001 - a side measurement never fails the bench
                    out["facade"] = {"error": str(e)[:200]}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
