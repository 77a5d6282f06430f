"""The pipelined decoder group's host choreography without a GPU: iamf_decoder_facade.c linked against stand-ins whose
device work is DEFERRED (tests/group_async_stub/async_stub.c: copies, uploads, unpack, renders and signals run later, in
stream order, and the rendered PCM is a hash of everything a launch read).  Several streams, handles out of step,
flushes and block feeding go through the synchronous group (iamf_hip_decoder_group_decode) and through the pipelined one
(two rounds in flight, data overwritten after _submit, sentinels in the pcm buffers of an outstanding round): every
handle's digest must be equal, under ASan + UBSan and under TSan, and no wait for one round may run the next round's
work (what a wait with stream semantics would do)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "group_async_stub")
SRCS = [os.path.join(ROOT, "iac_amd", "csrc", "iamf_decoder_facade.c"), os.path.join(STUB, "async_stub.c"),
        os.path.join(STUB, "group_async_driver.c")]
DEPS = SRCS + [os.path.join(ROOT, "iac_amd", "csrc", "iamf_decoder_group.inc"), os.path.join(ROOT, "iac_amd", "csrc", "facade_tu.h"),
               os.path.join(ROOT, "include", "iamf_hip.h"),
               os.path.join(ROOT, "tests", "facade_stub", "device_stub.c")]
STREAMS = ["toa_binaural_s16", "l714_J_ramps", "stereo_plus_scalable_C_ramps", "l714dmx_plus_l714dmx_C_trim", "stereo_441_to_48k"]


def _build(kind):
    b = os.path.join(STUB, "build_" + kind)
    os.makedirs(b, exist_ok=True)
    exe = os.path.join(b, "group_async_driver")
    if os.path.exists(exe) and all(os.path.getmtime(x) <= os.path.getmtime(exe) for x in DEPS):
        return exe
    inc = ["-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    if kind == "asan":
        subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all"] + inc + SRCS + ["-lm", "-lpthread", "-o", exe])
    else:
        # the facade's target_clones dispatch is an IFUNC whose resolver runs before the TSan runtime is up: the facade is
        # built without function entry / exit hooks (its memory accesses are instrumented all the same)
        objs = []
        for src, extra in ((SRCS[0], ["--param=tsan-instrument-func-entry-exit=0"]), (SRCS[1], []), (SRCS[2], [])):
            o = os.path.join(b, os.path.basename(src) + ".o")
            subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-fno-omit-frame-pointer", "-fsanitize=thread", "-c"] + extra +
                                  inc + [src, "-o", o])
            objs.append(o)
        subprocess.check_call(["gcc", "-fsanitize=thread"] + objs + ["-lm", "-lpthread", "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["asan", "tsan"])
def driver(request):
    return request.param, _build(request.param)


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    import e2e_cases
    d = tmp_path_factory.mktemp("group_async")
    out = {}
    for name in STREAMS:
        s, _ = e2e_cases.build(name)
        p = d / (name + ".iamf")
        p.write_bytes(s)
        c = e2e_cases.CASES[name]
        lay = "b" if c["layout"][0] == "binaural" else str(c["layout"][1])
        out[name] = (str(p), lay, str(c.get("bit_depth", 16)))
    return out


def _run(kind, exe, args):
    cmd = [exe] + [str(a) for a in args]
    if kind == "tsan":
        # gcc's TSan runtime assumes less mmap randomisation than newer kernels allow: the driver runs with address
        # randomisation off (a personality flag of this one child process)
        cmd = ["setarch", os.uname().machine, "-R"] + cmd
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("block", [0, 777])
@pytest.mark.parametrize("name", STREAMS)
def test_pipelined_group_equals_the_synchronous_group(driver, stream_files, name, block):
    kind, exe = driver
    path, lay, bits = stream_files[name]
    outs = {}
    for mode in ("sync", "pipe"):
        out = _run(kind, exe, [path, lay, bits, 7, 3, mode, block])
        head = out.splitlines()[0].split()
        stats = dict(zip(head[0::2], head[1::2]))
        assert stats["errors"] == "0", out
        assert stats["sentinel_violations"] == "0", out          # an outstanding round's pcm buffers stay untouched
        assert stats["late_drained"] == "0", out                 # no wait for round k ran round k + 1's work
        assert "times_rounds %s" % stats["rounds"] in out, out   # _times counts the submits
        outs[mode] = [l for l in out.splitlines() if l.startswith("h")]
    assert len(outs["sync"]) == 7
    assert any(" total 0 " not in l for l in outs["sync"])
    assert outs["pipe"] == outs["sync"]
