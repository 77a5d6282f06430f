"""Which kernel a render call takes is decided by pick_route() in iac_amd/csrc/render_route.hpp, a plain C++ header:
tests/route_host/route_host_check.cpp compiles it with the host compiler and checks a table of parameter blocks against
the expected kernel family, variant and return code (and the instance-list helper the launchers walk).  Every render
kernel is exact, so a wrong routing decision is invisible to the parity tests and shows only as a slower rate; this
is the test that sees it.  (That the routes are what gets launched: launch() in iamf_render.hip is a switch over them,
and the GPU suites cover each family's results.)  The table's last block holds the rules that read the stream position
(fast_shape_ok, pos16, pos_any) at pos0 = 2^31, 2^31 + 16, 2^32 + 8 and 2^40 + 237: every such call must take the route
the same call takes at 4096, 4112, 4104 and 4333."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_routing_table_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    m = re.search(r"(\d+) cases, (\d+) wrong", out)
    assert m and int(m.group(1)) >= 262 and int(m.group(2)) == 0, out
    # both sides of the staged limiter-table windows (kFWin, kWWin), every family that stages one
    for block in ("stereo (and a fan-out's member)", "stereo + second element", "down-mixer 6 -> 2", "LPCM", "12 channels",
                  "12 channels + second element", "down-mixer 12 -> 6", "demixer 12 -> 12", "LFE, 12 channels"):
        for side in ("kFWin", "kFWin - 1"):
            assert re.search(r"^%s: n_end = %s\s" % (re.escape(block), re.escape(side)), out, re.M), (block, side)
    assert "12 -> 11: n_end = kWWin - 1" in out and re.search(r"^12 -> 11: n_end = kWWin\s", out, re.M)
    assert "WRONG" not in out and out.strip().endswith("OK"), out
    for pos, small in ((2 ** 31, 4096), (2 ** 31 + 16, 4112), (2 ** 32 + 8, 4104), (2 ** 40 + 237, 4333)):
        for block in ("stereo", "12 channels", "12 channels, s24", "LFE, 12 channels", "LPCM", "limiter off"):
            assert "%s: pos0 = %d as at %d" % (block, pos, small) in out, (block, pos)
