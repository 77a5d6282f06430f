"""The interleaved f32 form without a GPU: tests/route_host/route_host_interleaved_check.cpp compiles render_route.hpp with
the host compiler and pins pick_route() for Family::FastInterleaved — every one of the 4 instances, then one row per rule:
the form's kernel on the near side, on the far side exactly the family the same RenderParams get with interleaved == 0 (what
iamf_hip_batch_render_range runs).  Lengths 1 .. 1115, positions 0 .. 2^31 + 1, strided and misaligned input, the 32-bit
bound of a call's bytes, both switches; and the parameter block keeps its size and every field its offset."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_interleaved_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_interleaved_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_interleaved_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 59 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
