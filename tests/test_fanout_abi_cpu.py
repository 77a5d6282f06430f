"""iamf_hip_batch_render_fanout on a host without a GPU: the entry is declared, exported and bound, and the count and
NULL checks answer before anything needs a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def _lib():
    import iac_amd
    iac_amd.build()
    return iac_amd.lib()


def test_entry_is_declared_exported_and_bound():
    import iac_amd
    _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+iamf_hip_batch_render_fanout\s*\(", src)
    m = re.search(r"#define\s+IAMF_HIP_FANOUT_MAX\s+(\d+)", src)
    assert m and int(m.group(1)) == iac_amd.FANOUT_MAX == 4
    assert hasattr(C.CDLL(iac_amd.lib_path()), "iamf_hip_batch_render_fanout")
    assert callable(iac_amd.render_fanout)


def _call(L, batches, n, d_in=0x1000, d_pcm="ok", strides="ok", n_emitted="ok"):
    """every pointer that is not under test is non-NULL; the fake handles are never dereferenced: each call here is refused
    by a check that comes before the members are looked at"""
    cnt = max(n, 1)
    hs = (C.c_void_p * cnt)(*([0x2000] * cnt)) if batches == "ok" else None
    pcms = (C.c_void_p * cnt)(*([0x3000] * cnt)) if d_pcm == "ok" else None
    st = (C.c_int64 * cnt)(*([1 << 20] * cnt)) if strides == "ok" else None
    em = (C.c_int32 * cnt)() if n_emitted == "ok" else None
    fused = C.c_int32(-7)
    r = L.iamf_hip_batch_render_fanout(hs, n, d_in, 0, 0, 1, pcms, st, None, em, C.byref(fused))
    assert fused.value == -7   # a refused call writes nothing
    return r


def test_member_count_is_checked_without_a_device():
    import iac_amd
    L = _lib()
    assert _call(L, "ok", 0) == BAD_ARG
    assert _call(L, "ok", -1) == BAD_ARG
    assert _call(L, "ok", iac_amd.FANOUT_MAX + 1) == BAD_ARG


def test_null_pointers_are_refused_without_a_device():
    L = _lib()
    assert _call(L, None, 2) == BAD_ARG
    assert _call(L, "ok", 2, d_pcm=None) == BAD_ARG
    assert _call(L, "ok", 2, strides=None) == BAD_ARG
    assert _call(L, "ok", 2, n_emitted=None) == BAD_ARG
    assert _call(L, "ok", 2, d_in=None) == BAD_ARG
    # a NULL member and a NULL member buffer
    hs = (C.c_void_p * 2)(0x2000, None)
    pcms = (C.c_void_p * 2)(0x3000, 0x3000)
    st = (C.c_int64 * 2)(1 << 20, 1 << 20)
    em = (C.c_int32 * 2)()
    assert L.iamf_hip_batch_render_fanout(hs, 2, 0x1000, 0, 0, 1, pcms, st, None, em, None) == BAD_ARG
    hs = (C.c_void_p * 1)(0x2000)
    pcms = (C.c_void_p * 1)(None)
    assert L.iamf_hip_batch_render_fanout(hs, 1, 0x1000, 0, 0, 1, pcms, st, None, em, None) == BAD_ARG


def test_a_member_given_twice_is_refused_without_a_device():
    """the members are compared as pointers, in member order, before any of them is looked at: with every other argument
    good the call is refused at the first repeat, whichever members repeat"""
    L = _lib()
    pcms = (C.c_void_p * 4)(0x3000, 0x3100, 0x3200, 0x3300)
    st = (C.c_int64 * 4)(*([1 << 20] * 4))
    for hs in ((0x2000, 0x2000), (0x2000, 0x2100, 0x2000), (0x2000, 0x2100, 0x2100), (0x2000, 0x2100, 0x2200, 0x2100)):
        em = (C.c_int32 * 4)(*([-9] * 4))
        fused = C.c_int32(-7)
        r = L.iamf_hip_batch_render_fanout((C.c_void_p * len(hs))(*hs), len(hs), 0x1000, 0, 0, 1, pcms, st, None, em, C.byref(fused))
        assert r == BAD_ARG and fused.value == -7 and list(em) == [-9] * 4, hs
    # ... and with n_frames == 0 too: the member list is checked before the early return
    em = (C.c_int32 * 4)(*([-9] * 4))
    assert L.iamf_hip_batch_render_fanout((C.c_void_p * 2)(0x2000, 0x2000), 2, 0x1000, 0, 0, 0, pcms, st, None, em, None) == BAD_ARG
    assert list(em) == [-9] * 4


def test_python_binding_raises_like_its_neighbours():
    import pytest

    import iac_amd
    _lib()
    with pytest.raises(iac_amd.IamfHipError) as e:
        iac_amd.render_fanout([], 0x1000, 0, 0, 1, [], [])
    assert e.value.code == BAD_ARG
