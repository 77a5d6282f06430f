"""iamf_hip_batch_render_fanout_packets on a host without a GPU: the entry is declared, exported and bound — the prototype of
iamf_hip_batch_render_fanout_lpcm with the call block of iamf_hip_batch_render_packets in the place of the packets, the frame
counts and the stream; the count, NULL, call-block and n_streams <= 0 checks answer before anything needs a device and leave
n_emitted and the report alone; the family FANOUT_PACKETS (51) lists exactly the rows of the three instance
lists; and the device code of every kernel the parent commit held is found again, instruction for instruction, beside one new
kernel per new instance (tools/kernel_hashes.py --anon against tests/golden/kernel_hashes_before_fanout_packets.txt, which is
that tool's output for the parent commit)."""
import collections
import concurrent.futures
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import fanout_packets_util as PU
import iac_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
NAME = "iamf_hip_batch_render_fanout_packets"


def _header():
    with open(os.path.join(ROOT, "include", "iamf_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _prototype(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_entry_is_declared_exported_and_mirrored():
    src = _header()
    # parameter for parameter the old entry's, with {in, n_frames, n_samples, stream} gathered in the packet entries' call block
    old = _prototype(src, "iamf_hip_batch_render_fanout_lpcm")
    assert old[2:5] == ["const iamf_hip_lpcm_input *in", "int32_t n_frames", "int32_t n_samples"] and old[7] == "void *stream"
    assert _prototype(src, NAME) == old[:2] + ["const iamf_hip_packet_call *call"] + old[5:7] + old[8:]
    out = subprocess.run(["nm", "-D", "--defined-only", A.lib_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAME in names and hasattr(A.lib(), NAME)
    for hidden in ("iamf_hip_fanout_pk24_launch", "iamf_hip_fanout_pk16c_launch", "iamf_hip_fanout_pk24c_launch"):
        assert hidden not in names       # the launch entries stay hidden
    old_types = A.lib().iamf_hip_batch_render_fanout_lpcm.argtypes
    assert A.lib().iamf_hip_batch_render_fanout_packets.argtypes == old_types[:2] + [C.POINTER(A.PacketCall)] + old_types[5:7] + old_types[8:]
    assert re.search(r"IAMF_HIP_ROUTE_FANOUT_PACKETS\s*=\s*%d\b" % PU.FAMILY, src)
    assert A.ROUTE_FAMILY_FANOUT == {PU.FAM: PU.FAMILY} and A.hipabi._family_id(PU.FAM) == PU.FAMILY and A.hipabi._family_name(PU.FAMILY) == PU.FAM
    for pinned in (A.ROUTE, A.ROUTE_BY_FAMILY_ONLY, A.ROUTE_FAMILY_MORE, A.ROUTE_FAMILY_LATER, A.ROUTE_FAMILY_NEWER, A.ROUTE_FAMILY_OPEN):
        assert PU.FAM not in pinned
    assert callable(A.render_fanout_packets)


def _call(batches, n, inp="ok", d_raw=0x1000, d_pcm="ok", strides="ok", n_emitted="ok", stream0=0, n_streams=4, n_frames=1, hs=None,
          pcms=None, spoil=None):
    """every pointer that is not under test is non-NULL; the fake handles are never dereferenced: each call here is refused by
    a check that comes before the members are looked at"""
    cnt = max(n, 1)
    if hs is None:
        hs = [0x2000 + 0x100 * i for i in range(cnt)]
    if pcms is None:
        pcms = [0x3000 + 0x100 * i for i in range(cnt)]
    h = (C.c_void_p * cnt)(*hs) if batches == "ok" else None
    p = (C.c_void_p * cnt)(*pcms) if d_pcm == "ok" else None
    st = (C.c_int64 * cnt)(*([1 << 20] * cnt)) if strides == "ok" else None
    em = (C.c_int32 * cnt)(*([-9] * cnt)) if n_emitted == "ok" else None
    call = A.PacketCall()
    call.in_.d_raw = d_raw
    call.args.n_frames = n_frames
    if spoil:
        spoil(call)
    rep = A.FanoutReport(-7, -7, -7, -7)
    r = A.lib().iamf_hip_batch_render_fanout_packets(h, n, C.byref(call) if inp == "ok" else None, p, st, stream0, n_streams, em,
                                                     C.byref(rep))
    assert (rep.n_fused, rep.input_fused, rep.n_unpacks, rep.reserved) == (-7, -7, -7, -7)   # a refused call writes nothing
    assert em is None or list(em) == [-9] * cnt
    return r


def test_count_null_and_range_refusals_need_no_device():
    assert _call("ok", 0) == BAD_ARG
    assert _call("ok", -1) == BAD_ARG
    assert _call("ok", A.FANOUT_MAX + 1) == BAD_ARG
    assert _call(None, 2) == BAD_ARG
    assert _call("ok", 2, d_pcm=None) == BAD_ARG
    assert _call("ok", 2, strides=None) == BAD_ARG
    assert _call("ok", 2, n_emitted=None) == BAD_ARG
    assert _call("ok", 2, inp=None) == BAD_ARG
    assert _call("ok", 2, d_raw=None) == BAD_ARG
    assert _call("ok", 2, n_frames=-1) == BAD_ARG
    assert _call("ok", 2, n_streams=0) == BAD_ARG
    assert _call("ok", 2, n_streams=-3) == BAD_ARG
    assert _call("ok", 2, stream0=-1) == BAD_ARG


def test_the_call_block_is_checked_without_a_device():
    """a reserved word, or a field of the args other than n_frames, n_samples and stream"""
    def reserved(call):
        call.reserved[3] = 1

    def field(name, value):
        return lambda call: setattr(call.args, name, value)

    assert _call("ok", 2, spoil=reserved) == BAD_ARG
    for name, value in (("d_in", 0x4000), ("d_in2", 0x4000), ("d_pcm", 0x4000), ("pcm_stream_stride_bytes", 64), ("d_element_ramp", 0x4000),
                        ("d_output_ramp", 0x4000), ("d_dmx_frames", 0x4000), ("d_demix_frames", 0x4000), ("lfe_pre_samples", 4),
                        ("in_stream_stride", 8), ("reserved0", 1)):
        assert _call("ok", 2, spoil=field(name, value)) == BAD_ARG, name
    assert _call("ok", 0, spoil=reserved) == BAD_ARG       # (the member count answers first; the code is the same)


def test_the_member_list_is_checked_without_a_device():
    for n_frames in (1, 0):
        assert _call("ok", 1, hs=[None], n_frames=n_frames) == BAD_ARG
        assert _call("ok", 2, hs=[0x2000, None], n_frames=n_frames) == BAD_ARG
        assert _call("ok", 1, pcms=[None], n_frames=n_frames) == BAD_ARG
        assert _call("ok", 2, hs=[0x2000, 0x2000], n_frames=n_frames) == BAD_ARG
        assert _call("ok", 4, hs=[0x2000, 0x2100, 0x2200, 0x2100], n_frames=n_frames) == BAD_ARG


def test_the_python_binding_raises_like_its_neighbours():
    import pytest
    with pytest.raises(A.IamfHipError) as e:
        A.render_fanout_packets([], A.LpcmInput(), 1, [], [])
    assert e.value.code == BAD_ARG
    with pytest.raises(ValueError):
        A.render_fanout_packets([], A.LpcmInput(), 1, [0x3000], [])


def test_the_family_lists_exactly_the_three_lists():
    rows = A.route_family_instances(PU.FAM)
    assert rows == PU.instance_rows() and len(rows) == 33 and len(set(rows)) == 33
    assert A.route_family_tally(PU.FAM) == {}
    # no row of it in a numbered table, no row of another family under its number
    for t in range(A.lib().iamf_hip_route_tables()):
        assert all(r[0] != PU.FAM for r in A.route_table_instances(t))
    for fam in PU.all_family_names():
        if fam != PU.FAM:
            assert all(r[0] == fam for r in A.route_family_instances(fam)), fam


def _hipflags():
    text = open(os.path.join(ROOT, "iac_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", text, flags=re.M)
    assert m
    return m.group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()


def test_every_kernel_of_the_parent_commit_is_found_again(tmp_path):
    """tools/kernel_hashes.py --anon of this tree: every hash line of the parent commit again, plus one new kernel per new
    instance — all of them render_fanout_kernel<M, K, true, LPB, LPC> of a new form"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _hipflags()
    srcs = sorted(glob.glob(os.path.join(ROOT, "iac_amd", "csrc", "*.hip")))

    def asm(src):
        out = os.path.join(str(tmp_path), os.path.basename(src) + ".s")
        p = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        return out

    jobs = max(1, min(8, len(os.sched_getaffinity(0))))
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        outs = list(ex.map(asm, srcs))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_hashes.py"), "--anon"] + outs, capture_output=True, text=True,
                       check=True)
    now = [line.split() for line in p.stdout.splitlines() if line.strip()]
    with open(os.path.join(ROOT, "tests", "golden", "kernel_hashes_before_fanout_packets.txt")) as f:
        before = [line.split() for line in f if line.strip()]
    assert len(before) == 760
    left = collections.Counter(h for h, _ in now)
    moved = []
    for h, sym in before:
        if left[h] > 0:
            left[h] -= 1
        else:
            moved.append(sym)
    assert not moved, "kernels of the parent commit whose code is not found again: %s" % moved[:5]
    assert len(now) == len(before) + 33
    # what is left over is the new instances: the other symbols are the parent's (the two fan-out templates gained arguments)
    old_syms = {sym for _, sym in before}
    new_syms = [sym for _, sym in now if sym not in old_syms and re.search(r"render_fanout_kernelILi\d+ELi\dELb1ELi[23]ELb[01]E", sym)
                and "ELb1ELi2ELb0E" not in sym]
    want = {"Li%dELi%dELb1ELi%dELb%dE" % (m, k, PU.FORMS[f][0], int(PU.FORMS[f][1])) for f in PU.FORMS for m in PU.FORM_M[f] for k in PU.FAN_K}
    got = {re.search(r"render_fanout_kernelI(Li\d+ELi\dELb1ELi[23]ELb[01]E)", s).group(1) for s in new_syms}
    assert got == want and len(new_syms) == 33
