#!/usr/bin/env python3
"""Decoder-group rates through the reference's API, synchronous against pipelined (include/iamf_hip.h:
iamf_hip_decoder_group_decode against _submit / _complete with two rounds in flight).

The stream is the one bench.py's facade line decodes (TOA -> binaural, 16-bit LPCM .iamf, one mono-coded ambisonics
element).  Every handle decodes it from the start; a round hands each handle the rest of its stream.  The pipelined loop
submits round k + 1 (its data pointers from the rsizes round k's _submit returned) before it completes round k, and
rotates two sets of pcm buffers.  Host OBU parsing, the packet uploads, the renders and the PCM back over PCIe are all
inside the time.  Prints ONE JSON line: Msamples/s and the per-round phases (iamf_hip_decoder_group_times) per group
size and mode; each figure is the best of --repeat runs.

usage: python tools/group_rate.py [--fs 1024] [--frames 192] [--sizes 64,256] [--repeat 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ("host_parse_stage_us", "enqueue_us", "device_wait_us", "copy_out_us")


def make_stream(fs, frames):
    import iamf_writer as W
    import synth
    in_ch = 16
    x = W.quantize(np.clip(synth.hot(4242, in_ch, frames * fs), -1, 1 - 2 ** -15).astype(np.float32), 16)
    pd = lambda pid: W.param_definition(pid, 48000, mode=1)
    s = W.sequence_header(1) + W.codec_config_lpcm(0, fs, 16, 48000)
    s += W.audio_element_ambisonics_mono(1, 0, in_ch, list(range(in_ch)))
    s += W.mix_presentation(1, [dict(eid=1, pdef=pd(100), default_q78=0)], dict(pdef=pd(101), default_q78=0), [("binaural",)])
    for f in range(frames):
        s += W.temporal_delimiter()
        s += W.audio_frames([(i, W.lpcm_bytes(x[i:i + 1, f * fs:(f + 1) * fs], 16)) for i in range(in_ch)])
    return s


def lib():
    import iac_amd
    L = C.CDLL(iac_amd.lib_path())
    L.IAMF_decoder_open.restype = C.c_void_p
    L.IAMF_decoder_close.argtypes = [C.c_void_p]
    L.IAMF_decoder_configure.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.IAMF_decoder_output_layout_set_binaural.argtypes = [C.c_void_p]
    L.IAMF_decoder_set_bit_depth.argtypes = [C.c_void_p, C.c_uint32]
    L.iamf_hip_decoder_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.iamf_hip_decoder_group_decode.argtypes = [C.c_void_p] * 6
    L.iamf_hip_decoder_group_submit.argtypes = [C.c_void_p] * 6 + [C.POINTER(C.c_uint64)]
    L.iamf_hip_decoder_group_complete.argtypes = [C.c_void_p, C.c_uint64]
    L.iamf_hip_decoder_group_destroy.argtypes = [C.c_void_p]
    L.iamf_hip_decoder_group_destroy.restype = None
    L.iamf_hip_decoder_group_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def run(L, stream, n, pipelined):
    buf = C.create_string_buffer(stream, len(stream))
    base = C.addressof(buf)
    hs, used0 = [], 0
    for _ in range(n):
        d = L.IAMF_decoder_open()
        L.IAMF_decoder_set_bit_depth(d, 16)
        L.IAMF_decoder_output_layout_set_binaural(d)
        rs = C.c_uint32(0)
        assert L.IAMF_decoder_configure(d, base, len(stream), C.byref(rs)) == 0
        hs.append(d)
        used0 = rs.value
    harr = (C.c_void_p * n)(*hs)
    g = C.c_void_p()
    assert L.iamf_hip_decoder_group_create(harr, n, 0, C.byref(g)) == 0
    pcms = [[C.create_string_buffer(2 * 6144 * 2) for _ in range(n)] for _ in range(2)]
    parr = [(C.c_void_p * n)(*[C.addressof(p) for p in pcms[k]]) for k in range(2)]
    data, sizes, rsz = (C.c_uint64 * n)(), (C.c_int32 * n)(), (C.c_uint32 * n)()
    res = [(C.c_int32 * n)() for _ in range(2)]
    vd, vs, vr = np.frombuffer(data, dtype=np.uint64), np.frombuffer(sizes, dtype=np.int32), np.frombuffer(rsz, dtype=np.uint32)
    vres = [np.frombuffer(r, dtype=np.int32) for r in res]
    used = np.full(n, used0, dtype=np.int64)
    total, rounds, k, out = 0, 0, 0, []
    t = C.c_uint64(0)
    t0 = time.perf_counter()
    last = False
    while True:
        if last:
            vd[:] = 0
            vs[:] = 0
        else:
            vd[:] = (base + used).astype(np.uint64)
            vs[:] = (len(stream) - used).astype(np.int32)
        if pipelined:
            assert L.iamf_hip_decoder_group_submit(g, data, sizes, rsz, parr[k], res[k], C.byref(t)) == 0
            out.append(t.value)
            if len(out) == 2:
                assert L.iamf_hip_decoder_group_complete(g, out.pop(0)) == 0
        else:
            assert L.iamf_hip_decoder_group_decode(g, data, sizes, rsz, parr[k], res[k]) == 0
        assert int(vres[k].min()) >= 0
        total += int(vres[k].sum())
        rounds += 1
        k ^= 1
        if last:
            break
        used += vr.astype(np.int64)
        last = int(vr.min()) == 0 or int(used.min()) >= len(stream)
    while out:
        assert L.iamf_hip_decoder_group_complete(g, out.pop(0)) == 0
    dt = time.perf_counter() - t0
    ph, nr = (C.c_double * 4)(), C.c_int64(0)
    L.iamf_hip_decoder_group_times(g, ph, C.byref(nr))
    assert nr.value == rounds
    L.iamf_hip_decoder_group_destroy(g)
    for d in hs:
        L.IAMF_decoder_close(d)
    return dict(msamples_s=round(total / dt / 1e6, 1), us_per_round=round(dt / rounds * 1e6, 1), rounds=rounds,
                phases_us_per_round={name: round(ph[i] / rounds * 1e6, 1) for i, name in enumerate(PHASES)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    L = lib()
    stream = make_stream(a.fs, a.frames)
    run(L, stream, 8, False)   # code objects loaded, LDS opted into, outside the timing
    run(L, stream, 8, True)
    res = {}
    for n in (int(v) for v in a.sizes.split(",")):
        for mode in ("sync", "pipelined"):
            best = max((run(L, stream, n, mode == "pipelined") for _ in range(a.repeat)), key=lambda r: r["msamples_s"])
            res["%d_%s" % (n, mode)] = best
        res["%d_speedup" % n] = round(res["%d_pipelined" % n]["msamples_s"] / res["%d_sync" % n]["msamples_s"], 3)
    print(json.dumps({"tool": "group_rate", "workload": "TOA -> binaural, 16-bit LPCM .iamf, %d frames of %d samples per handle, "
                      "through the reference's API (PCIe and host parsing included)" % (a.frames, a.fs),
                      "gpu": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
