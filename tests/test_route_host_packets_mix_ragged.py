"""The ragged two-element packet form without a GPU: tests/route_host/route_host_packets_mix_ragged_check.cpp compiles
render_route.hpp with the host compiler and pins one row per term of packets_mix_ragged_shape_ok — the length, the position,
lpcm_mix against lpcm_bytes and m2, the bed's lists, both elements' grids and 32-bit bounds, the ramp rows' alignment and
stride, the trimmed frame's inequality, every stage and flag that keeps a call away, the three switches — each with that term
changed alone; every (sample size, M, OC, LP2) takes Family::PacketsMixRagged, a row of set 10 and of no other set; every set
keeps its pinned row count, no row for a number outside the listing; a call without the mark routes as in the parent, as do the marks 1 and 2; sizeof and offsetof of
the parameter blocks are as pinned."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_packets_mix_ragged_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_packets_mix_ragged_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_packets_mix_ragged_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 340 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
