"""The routing of the limiter-less renderer's two-element packet form without a GPU:
tests/route_host/route_host_nolim_packets_mix_check.cpp compiles render_route.hpp and lpcm_form.hpp with the host compiler and pins
one row per rule of nolim_packets_mix_shape_ok behind lpcm_form_packets on each element, each flipped alone — limiter on, total 6,
frame size 6, first + n > fs, element 1 off its grid (16 and 24 bit), the pair's partner misplaced, m2 = 2 as mono runs, m2 = 3,
sample sizes that differ, a ramp off 16 bytes, a ramp stride of 4k + 1, out_ch * bytes of 2 and 64, d_pcm off 16, each
off-switch, each stage that keeps the form away; every (sample size, M, LP2) takes Family::NolimPacketsMix, a row of set 12 and of
no other set; every set keeps its pinned row count, no row for a number outside the listing; a block without the mark, or with mark 4, routes as in the parent."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_nolim_packets_mix_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_nolim_packets_mix_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_nolim_packets_mix_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 250 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
