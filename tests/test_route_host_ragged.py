"""The planar ragged form without a GPU: tests/route_host/route_host_ragged_check.cpp compiles render_route.hpp with the host
compiler and pins pick_route() for Family::FastRagged — every one of the 18 instances, then one row per rule of
ragged_shape_ok with one field changed: the form's kernel on the near side, on the far side exactly the family the same
RenderParams get with ragged == 0 (what iamf_hip_batch_render_range runs, and ran before the form existed).  Lengths 1 ..
5000 in one frame and in several, whole blocks with the flag set (Family::Fast), positions 0 .. 2^31 + 1, misaligned input
and PCM, the 32-bit bound, both switches; the parameter block keeps its size and every field its offset; and every key of
set 6 is in that set only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_ragged_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_ragged_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_ragged_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
