"""The routes did not move: tests/route_host/route_host_sweep_check.cpp compiles render_route.hpp with the host compiler and routes
a deterministic family of parameter blocks through both pick_route overloads — for every row of every set the smallest block
that routes to it, every single mutation of a fixed list from each (zero, a step off the grid, a step past each bound, each mark,
each off-switch alone) and a seeded selection of pairs — printing one digest line per 1024 cases.  tests/golden/route_sweep.txt
holds the lines the same program printed against the tree in front of the change that gathered the packet rules into shared
predicates; the output must be those lines, one by one.  The program checks its own coverage: every Family is reached by at
least 100 cases, each marked rule answers true and false on at least 5 % of the cases that carry its mark."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_route_sweep_matches_the_golden_lines(tmp_path):
    exe = os.path.join(str(tmp_path), "route_host_sweep_check")
    src = os.path.join(ROOT, "tests", "route_host", "route_host_sweep_check.cpp")
    cc = CLANG if os.path.exists(CLANG) else "clang++"
    subprocess.check_call([cc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, src])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAMF_HIP_")}
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr
    got = p.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "route_sweep.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 400 and want[-1] == "OK"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d: got %r, golden %r (route_host_sweep_check --dump prints the cases)" % (i + 1, g, w)
    assert len(got) == len(want)
    assert "WRONG" not in p.stdout
