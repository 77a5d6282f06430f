"""The packet-fed limiter-less renderer's routing without a GPU: tests/route_host/route_host_nolim_packets_check.cpp compiles
render_route.hpp and lpcm_form.hpp with the host compiler and pins one row per rule of nolim_packets_shape_ok behind
lpcm_form_packets, each flipped alone — limiter on, total = 6, frame size = 6, d_pcm off 16, out_ch * bytes = 2 and 64,
first + n > fs, a 16-bit run off the 8-byte grid, big-endian, 32 bit, mono-coded 5.1, each off-switch, every stage that keeps
the f32 form away; every (sample size, M) takes Family::NolimPackets, a row of set 11 and of no other set; every set
keeps its pinned row count, no row for a number outside the listing; a block without the mark, or a limiter-on one with it, routes as in the parent."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_nolim_packets_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_nolim_packets_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_nolim_packets_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 145 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
