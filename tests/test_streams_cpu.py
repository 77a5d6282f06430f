"""No GPU: tests/stream_util.py wraps exactly the entries of include/iamf_hip.h that take a stream.

stalled() puts a stall in front of every entry of stream_util.ENTRIES.  An entry added to the header later with a
`void *stream`, an `iamf_hip_render_args *` or an `iamf_hip_lpcm_input *` and not added there would run unstalled in
tests/test_gpu_streams.py without anybody noticing; here it fails."""
import ctypes as C
import os

import stream_util as SU

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iamf_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_wrapper_lists_exactly_the_headers_stream_taking_prototypes():
    found = SU.header_stream_entries(_header())
    assert len(found) >= 28, sorted(found)         # the parser found the prototypes at all
    assert set(found) == set(SU.ENTRIES), (sorted(set(found) - set(SU.ENTRIES)), sorted(set(SU.ENTRIES) - set(found)))
    assert found == SU.ENTRIES, {k: (found[k], SU.ENTRIES[k]) for k in found if found[k] != SU.ENTRIES[k]}


def test_the_parser_sees_each_form():
    text = """
    /* int iamf_hip_in_a_comment(void *stream); */
    #define iamf_hip_in_a_macro(stream) 0
    typedef struct { void *stream; } iamf_hip_some_args;
    int iamf_hip_a(int x, void *stream);
    int iamf_hip_b(iamf_hip_batch *b,
                   const iamf_hip_render_args *args /* a comment, with a comma */, int n);
    int iamf_hip_c(const iamf_hip_lpcm_input *in, const iamf_hip_render_args *a);
    int iamf_hip_d(const iamf_hip_lpcm_input *in);
    void *iamf_hip_shard_render_stream(iamf_hip_shard *s, int index);
    int iamf_hip_e(void *streams, void *decoder_handle);
    int iamf_hip_f(iamf_hip_render_args *args);
    int iamf_hip_g(int n, struct iamf_hip_lpcm_input *const in);
    int iamf_hip_h(void *const stream);
    """
    assert SU.header_stream_entries(text) == {"iamf_hip_a": ("arg", 1), "iamf_hip_b": ("args", 1), "iamf_hip_c": ("args", 1),
                                              "iamf_hip_d": ("lpcm", 0), "iamf_hip_f": ("args", 0), "iamf_hip_g": ("lpcm", 1),
                                              "iamf_hip_h": ("arg", 0)}


def test_the_binding_knows_every_wrapped_entry():
    """stalled() patches the attributes of iac_amd.lib(): an entry of ENTRIES the binding never names (no argtypes, no
    caller) would be wrapped and never called through the wrapper"""
    import re
    src = open(os.path.join(os.path.dirname(HEADER), "..", "iac_amd", "hipabi.py")).read()
    unnamed = [name for name in SU.ENTRIES if not re.search(r"\b%s\b" % name, src)]
    assert unnamed == ["iamf_hip_upload_by_kernel"], unnamed     # the tests call it with ctypes values of their own


def test_stream_of_finds_the_stream():
    class Args(C.Structure):
        _fields_ = [("d_in", C.c_void_p), ("stream", C.c_void_p)]

    a = Args()
    a.stream = 0x1234
    assert SU.stream_of("iamf_hip_batch_render_ex", (None, C.byref(a))) == 0x1234
    assert SU.stream_of("iamf_hip_batch_render_lpcm", (None, None, C.pointer(a))) == 0x1234
    assert SU.stream_of("iamf_hip_batch_flush", (None, 0, 0, 0x77)) == 0x77
    assert SU.stream_of("iamf_hip_batch_flush", (None, 0, 0, C.c_void_p(0x78))) == 0x78
    assert SU.stream_of("iamf_hip_batch_flush", (None, 0, 0, None)) == 0
    assert SU.stream_of("iamf_hip_stream_signal", (0x55, 0, 1)) == 0x55
    a.stream = None
    assert SU.stream_of("iamf_hip_batch_render_range", (None, C.byref(a), 0, 1)) == 0


def test_the_stall_is_bounded():
    import pytest
    assert 0 < SU.STALL_MS <= SU.MAX_STALL_MS <= 50.0
    with pytest.raises(AssertionError):
        SU.stall(None, 50.1)
    with pytest.raises(AssertionError):
        SU.stalled("ELSEWHERE").__enter__()
