"""The two-element packet form without a GPU: tests/route_host/route_host_lpcm_mix_check.cpp compiles render_route.hpp and
lpcm_form.hpp with the host compiler and pins pick_route() for Family::LpcmMix — every one of the 36 instances, then one
row per rule, each an aligned call with one field changed: the refusals of the single-element packet forms, the second
element's channel count per form, its packets' alignment and 32-bit offset bound, the ramps' alignment — and the form
lpcm_form() gives each layout a second element can have."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_lpcm_mix_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_lpcm_mix_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_lpcm_mix_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 94 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
