"""The two-element 24-bit packet form without a GPU: tests/route_host/route_host_lpcm24_mix_check.cpp compiles render_route.hpp
and lpcm_form.hpp with the host compiler and pins one row per rule — the second element's forms as lpcm_form_packets()
answers them (mono runs, one pair, the dword grid with trimmed starts, two mono runs for stereo, 16- and 32-bit samples, byte
order, d_raw, the strides), and pick_route(): every (M, OC, LP2) takes Family::Lpcm24Mix; lpcm_mix 1 / 2 with 24-bit samples and
lpcm_mix 3 are refused as before; 4 | LP2 with another sample size or coupling names no form; each refusal of Family::LpcmMix
with one pointer, stride, bound or flag changed; the route_key's set is 8 and no other set holds its row; every
set keeps its pinned row count, no row for a number outside the listing; sizeof and offsetof of the parameter blocks are as pinned."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_lpcm24_mix_form_and_routing_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_lpcm24_mix_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_lpcm24_mix_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 110 and int(m.group(2)) == 0, out
    assert "WRONG" not in out and out.strip().endswith("OK"), out
