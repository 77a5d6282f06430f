"""The 24-bit LPCM form without a GPU: tests/route_host/route_host_lpcm24_check.cpp compiles render_route.hpp and
lpcm_form.hpp with the host compiler and pins one row per rule — every (m, oc) takes Family::Lpcm24, the variant by the
launch's size, each refusal, each alignment rule of the 12-byte loads, the 16-bit rows as they stood, and the route of every packet layout of
tests/gpu_util.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_lpcm24_form_and_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_lpcm24_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_lpcm24_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 80 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
