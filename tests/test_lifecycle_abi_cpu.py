"""The per-stream lifecycle entries (restart, range gains, export, import; batch and resampler) on a host without a GPU:
every entry is declared, exported and bound, a NULL handle is refused before anything needs a device, and the two ctypes
structures have the size the C compiler gives them."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1

INT_ENTRIES = ["iamf_hip_batch_set_gains_range", "iamf_hip_batch_restart_range", "iamf_hip_batch_export_range",
               "iamf_hip_batch_import_range", "iamf_hip_resampler_restart_range", "iamf_hip_resampler_export_range",
               "iamf_hip_resampler_import_range"]
BYTES_ENTRIES = ["iamf_hip_batch_stream_state_bytes", "iamf_hip_resampler_stream_state_bytes"]


def _lib():
    import iac_amd
    iac_amd.build()
    return iac_amd.lib()


def test_entries_are_declared_exported_and_bound():
    import iac_amd
    L = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamf_hip.h")).read(), flags=re.S)
    raw = C.CDLL(iac_amd.lib_path())
    for name in INT_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in BYTES_ENTRIES:
        assert re.search(r"\bint64_t\s+%s\s*\(" % name, src), name
        assert hasattr(raw, name), name
        assert getattr(L, name).restype is C.c_int64, name
    for typ in ("iamf_hip_stream_gains", "iamf_hip_stream_state"):
        assert re.search(r"\}\s*%s\s*;" % typ, src), typ
    for cls, meths in ((iac_amd.Batch, ("restart_range", "set_gains_range", "export_range", "import_range", "stream_state_bytes")),
                       (iac_amd.Resampler, ("restart_range", "export_range", "import_range", "stream_state_bytes"))):
        for m in meths:
            assert callable(getattr(cls, m)), (cls, m)


def test_null_handle_is_refused_without_a_device():
    import iac_amd
    L = _lib()
    g = iac_amd.stream_gains(element=[1.0])
    t = (iac_amd.StreamState * 1)()
    assert L.iamf_hip_batch_set_gains_range(None, 0, 1, C.byref(g), None) == BAD_ARG
    assert L.iamf_hip_batch_restart_range(None, 0, 1, None, None) == BAD_ARG
    assert L.iamf_hip_batch_restart_range(None, 0, 1, C.byref(g), None) == BAD_ARG
    assert L.iamf_hip_batch_export_range(None, 0, 1, 0x1000, 1 << 20, t, None) == BAD_ARG
    assert L.iamf_hip_batch_import_range(None, 0, 1, 0x1000, 1 << 20, t, None) == BAD_ARG
    assert L.iamf_hip_resampler_restart_range(None, 0, 1, None) == BAD_ARG
    assert L.iamf_hip_resampler_export_range(None, 0, 1, 0x1000, 1 << 20, t, None) == BAD_ARG
    assert L.iamf_hip_resampler_import_range(None, 0, 1, 0x1000, 1 << 20, t, None) == BAD_ARG
    assert L.iamf_hip_batch_stream_state_bytes(None) < 0
    assert L.iamf_hip_resampler_stream_state_bytes(None) < 0
    assert bytes(t) == bytes(C.sizeof(t))   # a refused export wrote no ticket


def test_python_binding_raises_like_its_neighbours():
    import iac_amd
    _lib()
    b = iac_amd.Batch.__new__(iac_amd.Batch)   # a handle that was never created
    b.h = None
    r = iac_amd.Resampler.__new__(iac_amd.Resampler)
    r.h = None
    for call in (lambda: b.restart_range(0, 1), lambda: b.set_gains_range(0, 1, iac_amd.stream_gains(output=[2.0])),
                 lambda: b.export_range(0, 1, 0x1000, 1 << 20), lambda: b.import_range(0, 1, 0x1000, 1 << 20, [iac_amd.StreamState()]),
                 b.stream_state_bytes, lambda: r.restart_range(0, 1), lambda: r.export_range(0, 1, 0x1000, 1 << 20),
                 lambda: r.import_range(0, 1, 0x1000, 1 << 20, [iac_amd.StreamState()]), r.stream_state_bytes):
        with pytest.raises(iac_amd.IamfHipError) as e:
            call()
        assert e.value.code == BAD_ARG


def test_structure_sizes_match_the_c_compiler(tmp_path):
    import iac_amd
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "iamf_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(iamf_hip_stream_state), sizeof(iamf_hip_stream_gains)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    state, gains = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert C.sizeof(iac_amd.StreamState) == state
    assert C.sizeof(iac_amd.StreamGains) == gains
