"""The coupled 24-bit LPCM form without a GPU: tests/route_host/route_host_lpcm24_coupled_check.cpp compiles render_route.hpp
and lpcm_form.hpp with the host compiler and pins one row per rule of LpcmForm::S24C as lpcm_form_packets() answers it — every
channel count, the pairs' dword grid with odd and even first samples, the step, the partner's place, a pair on the wrong
channels, C and LFE, byte order, a missing channel, the strides, d_raw, 32-bit samples, and lpcm_form() still answering None for
every canonical layout — the 16-bit and mono-coded 24-bit rows through the wrapper, and one per rule of pick_route(): every
(m, oc) takes Family::Lpcm24Coupled, lpcm_coupled == 2 with another sample size and == 1 with 24-bit samples are refused, the
variant by the launch's size and the switches, each refusal of Family::Lpcm24, the listing's 20 rows of family 31 in a set
behind the pinned seven."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_lpcm24_coupled_form_and_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_lpcm24_coupled_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_lpcm24_coupled_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 120 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
