"""The coupled 16-bit LPCM form without a GPU: tests/route_host/route_host_lpcm_coupled_check.cpp compiles render_route.hpp
and lpcm_form.hpp with the host compiler and pins one row per rule of LpcmForm::S16C — every channel count, the pairs'
8-byte grid with an odd and an even first sample, the partner's place, a pair on the wrong channels, C and LFE, the mono-coded
and 24-bit elements that stay unfused, byte order, a missing channel, the strides — and one per rule of pick_route():
every (m, oc) takes Family::LpcmCoupled, the variant by the launch's size and the switches, each refusal."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_lpcm_coupled_form_and_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_lpcm_coupled_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_lpcm_coupled_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 90 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
