"""What a temporal unit needs that is plain arithmetic — the trim window, the walk over an element's sub-streams and the
channel order behind it, the render arguments of an element's stage, the last stage behind the resampler — lives in
iac_amd/csrc/facade_tu.h, a plain C header that the decoder facade's single handle and its decoder group both use.
tests/facade_host/facade_host_check.c includes nothing else of the project, is compiled with the host compiler under
ASan / UBSan and checks the pieces against values written out by hand.  (That the facade uses them as before: the
bit-for-bit comparisons with the reference decoder in tests/test_gpu_facade.py and tests/test_gpu_group.py.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iac_amd", "csrc")


def test_the_header_compiles_alone():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", "-x", "c",
                           os.path.join(CSRC, "facade_tu.h")])
    text = open(os.path.join(CSRC, "facade_tu.h")).read()
    assert re.findall(r"^#include\s+(\S+)", text, re.M) == ["<stdint.h>", "<string.h>", '"iamf_hip.h"']
    assert "IAMF_Decoder" not in text


def test_temporal_unit_pieces_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "facade_host_check")
    src = os.path.join(ROOT, "tests", "facade_host", "facade_host_check.c")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    m = re.search(r"(\d+) cases, (\d+) wrong", p.stdout)
    assert m and int(m.group(1)) >= 45 and int(m.group(2)) == 0, p.stdout
    assert "WRONG" not in p.stdout and p.stdout.strip().endswith("OK"), p.stdout
