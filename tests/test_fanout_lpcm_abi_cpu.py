"""iamf_hip_batch_render_fanout_lpcm and iamf_hip_batch_render_fanout_range on a host without a GPU: both entries are
declared, exported and bound; the count, NULL and n_streams <= 0 checks answer before anything needs a device and leave
the report alone; the extension listing is there and its tally is empty."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def _lib():
    import iac_amd
    iac_amd.build()
    return iac_amd.lib()


def test_entries_are_declared_exported_and_bound():
    import iac_amd
    _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamf_hip.h")).read(), flags=re.S)
    so = C.CDLL(iac_amd.lib_path())
    for name in ("iamf_hip_batch_render_fanout_lpcm", "iamf_hip_batch_render_fanout_range", "iamf_hip_route_instances_ext",
                 "iamf_hip_route_tally_ext"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(so, name), name
    assert re.search(r"typedef\s+struct\s+iamf_hip_fanout_report\s*\{[^}]*n_fused;[^}]*input_fused;[^}]*n_unpacks;[^}]*reserved;[^}]*\}", src)
    assert re.search(r"IAMF_HIP_ROUTE_FANOUT_LPCM\s*=\s*15\b", src) and iac_amd.ROUTE["FANOUT_LPCM"] == 15
    assert C.sizeof(iac_amd.FanoutReport) == 16
    assert callable(iac_amd.render_fanout_lpcm) and callable(iac_amd.render_fanout_range)
    assert callable(iac_amd.route_instances_ext) and callable(iac_amd.route_tally_ext)


def _lpcm(L, batches, n, inp="ok", d_raw=0x1000, d_pcm="ok", strides="ok", n_emitted="ok", stream0=0, n_streams=4, n_frames=1):
    """every pointer that is not under test is non-NULL; the fake handles are never dereferenced: each call here is refused
    by a check that comes before the members are looked at"""
    import iac_amd
    cnt = max(n, 1)
    hs = (C.c_void_p * cnt)(*([0x2000] * cnt)) if batches == "ok" else None
    pcms = (C.c_void_p * cnt)(*([0x3000] * cnt)) if d_pcm == "ok" else None
    st = (C.c_int64 * cnt)(*([1 << 20] * cnt)) if strides == "ok" else None
    em = (C.c_int32 * cnt)(*([-9] * cnt)) if n_emitted == "ok" else None
    li = iac_amd.LpcmInput()
    li.d_raw = d_raw
    rep = iac_amd.FanoutReport(-7, -7, -7, -7)
    r = L.iamf_hip_batch_render_fanout_lpcm(hs, n, C.byref(li) if inp == "ok" else None, n_frames, 0, pcms, st, None, stream0,
                                            n_streams, em, C.byref(rep))
    assert (rep.n_fused, rep.input_fused, rep.n_unpacks, rep.reserved) == (-7, -7, -7, -7)   # a refused call writes nothing
    assert em is None or list(em) == [-9] * cnt
    return r


def _range(L, batches, n, d_in=0x1000, d_pcm="ok", strides="ok", n_emitted="ok", stream0=0, n_streams=4):
    cnt = max(n, 1)
    hs = (C.c_void_p * cnt)(*([0x2000] * cnt)) if batches == "ok" else None
    pcms = (C.c_void_p * cnt)(*([0x3000] * cnt)) if d_pcm == "ok" else None
    st = (C.c_int64 * cnt)(*([1 << 20] * cnt)) if strides == "ok" else None
    em = (C.c_int32 * cnt)(*([-9] * cnt)) if n_emitted == "ok" else None
    fused = C.c_int32(-7)
    r = L.iamf_hip_batch_render_fanout_range(hs, n, d_in, 0, 0, 1, pcms, st, None, em, C.byref(fused), stream0, n_streams)
    assert fused.value == -7
    assert em is None or list(em) == [-9] * cnt
    return r


def test_member_count_is_checked_without_a_device():
    import iac_amd
    L = _lib()
    for call in (_lpcm, _range):
        assert call(L, "ok", 0) == BAD_ARG
        assert call(L, "ok", -1) == BAD_ARG
        assert call(L, "ok", iac_amd.FANOUT_MAX + 1) == BAD_ARG


def test_null_pointers_are_refused_without_a_device():
    L = _lib()
    for call in (_lpcm, _range):
        assert call(L, None, 2) == BAD_ARG
        assert call(L, "ok", 2, d_pcm=None) == BAD_ARG
        assert call(L, "ok", 2, strides=None) == BAD_ARG
        assert call(L, "ok", 2, n_emitted=None) == BAD_ARG
    assert _range(L, "ok", 2, d_in=None) == BAD_ARG
    assert _lpcm(L, "ok", 2, inp=None) == BAD_ARG
    assert _lpcm(L, "ok", 2, d_raw=None) == BAD_ARG
    assert _lpcm(L, "ok", 2, n_frames=-1) == BAD_ARG


def test_an_empty_or_negative_range_is_refused_without_a_device():
    L = _lib()
    for call in (_lpcm, _range):
        assert call(L, "ok", 2, n_streams=0) == BAD_ARG
        assert call(L, "ok", 2, n_streams=-3) == BAD_ARG
        assert call(L, "ok", 2, stream0=-1) == BAD_ARG


def _members(L, entry, hs, pcms, n_frames=1):
    """every argument good but the member list: the handles are fakes that the member-list check compares and never reads"""
    import iac_amd
    n = len(hs)
    st = (C.c_int64 * n)(*([1 << 20] * n))
    em = (C.c_int32 * n)(*([-9] * n))
    if entry == "lpcm":
        li = iac_amd.LpcmInput()
        li.d_raw = 0x1000
        rep = iac_amd.FanoutReport(-7, -7, -7, -7)
        r = L.iamf_hip_batch_render_fanout_lpcm((C.c_void_p * n)(*hs), n, C.byref(li), n_frames, 0, (C.c_void_p * n)(*pcms), st, None,
                                                0, 4, em, C.byref(rep))
        assert (rep.n_fused, rep.input_fused, rep.n_unpacks, rep.reserved) == (-7, -7, -7, -7)
    else:
        fused = C.c_int32(-7)
        r = L.iamf_hip_batch_render_fanout_range((C.c_void_p * n)(*hs), n, 0x1000, 0, 0, n_frames, (C.c_void_p * n)(*pcms), st, None,
                                                 em, C.byref(fused), 0, 4)
        assert fused.value == -7
    assert list(em) == [-9] * n
    return r


def test_the_member_list_is_checked_without_a_device():
    """a NULL member, a NULL member buffer and a member given twice are refused in member order, by pointer comparison
    alone, before any member is looked at and before the n_frames == 0 early return"""
    L = _lib()
    ok = [0x3000, 0x3100, 0x3200, 0x3300]
    for entry in ("lpcm", "range"):
        for n_frames in (1, 0):
            assert _members(L, entry, [None], ok[:1], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000, None], ok[:2], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000], [None], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000, 0x2000], ok[:2], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000, 0x2100, 0x2000], ok[:3], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000, 0x2100, 0x2100], ok[:3], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000, 0x2100, 0x2200, 0x2100], ok, n_frames) == BAD_ARG
            # the buffer of member 1 is looked at before member 2 is compared with member 0, and the other way round
            assert _members(L, entry, [0x2000, 0x2100, 0x2000], [0x3000, None, 0x3200], n_frames) == BAD_ARG
            assert _members(L, entry, [0x2000, 0x2000, 0x2200], [0x3000, 0x3100, None], n_frames) == BAD_ARG


def test_python_bindings_raise_like_their_neighbours():
    import pytest

    import iac_amd
    _lib()
    with pytest.raises(iac_amd.IamfHipError) as e:
        iac_amd.render_fanout_lpcm([], iac_amd.LpcmInput(), 1, [], [])
    assert e.value.code == BAD_ARG
    with pytest.raises(iac_amd.IamfHipError) as e:
        iac_amd.render_fanout_range([], 0x1000, 0, 0, 1, [], [], 0, 1)
    assert e.value.code == BAD_ARG


def test_ext_listing_and_tally_without_a_device():
    import iac_amd
    _lib()
    rows = iac_amd.route_instances_ext()
    assert rows and all(r[0] == "FANOUT_LPCM" for r in rows)
    assert iac_amd.route_tally_ext(reset=False) == {}
    assert iac_amd.route_tally_ext(reset=True) == {}
