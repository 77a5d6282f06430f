"""Caller-owned non-blocking streams for the -m gpu tests (tests/test_gpu_streams.py): a side stream that is proven
non-blocking, a bounded spin to put in front of a library call, and a wrapper that puts one in front of EVERY entry of
include/iamf_hip.h that takes a stream.  Nothing here needs a GPU, torch or the library until it is used;
tests/test_streams_cpu.py holds ENTRIES against the header.

The stall is a test INPUT, never a pass threshold: it only has to be long against the host time of one library call (tens
of microseconds once the kernels are loaded) so that "the device had not started the call's work when the call
returned" is what the tests observe.  It is torch.cuda._sleep(cycles), calibrated once per process with events:

    STALL_MS = 10 ms asked for, MAX_STALL_MS = 50 ms never exceeded (stall() refuses more, and calibration fails if
    the spin it measured is not between 0.5 and 5 times what it asked for).
    Measured on an MI355X (printed by calibrate(), `-s` shows it): 2 392 187 spin cycles per ms (torch's spin counts
    the 2.4 GHz shader clock), and the 10 ms stall made from that measured 9.97 ms.  Stall lengths used by the tests: 10 ms
    everywhere.

A run where the spin does not spin fails: the wrapper asserts, before it enters the library, that the stream of the call
is a non-null stream whose flags (hipStreamGetFlags, read from the HIP runtime the process has loaded) say
hipStreamNonBlocking, and that the stall's event has not completed.
"""
import collections
import contextlib
import ctypes as C
import threading

STALL_MS = 10.0
MAX_STALL_MS = 50.0
NULL, SAME = "NULL", "SAME"
HIP_STREAM_NON_BLOCKING = 0x01

# Every prototype of include/iamf_hip.h that takes a `void *stream`, an `iamf_hip_render_args *` or an
# `iamf_hip_lpcm_input *`: where its stream is — ("arg", i): argument i is the stream; ("args", i): argument i is the
# iamf_hip_render_args whose field `stream` is.  (The entries that take an iamf_hip_lpcm_input also take one of the two.)
ENTRIES = {
    "iamf_hip_batch_render": ("arg", 7),
    "iamf_hip_batch_render_ex": ("args", 1),
    "iamf_hip_batch_render_range": ("args", 1),
    "iamf_hip_batch_flush": ("arg", 3),
    "iamf_hip_batch_flush_range": ("arg", 3),
    "iamf_hip_batch_lfe_advance": ("arg", 4),
    "iamf_hip_batch_render_fanout": ("arg", 8),
    "iamf_hip_batch_render_fanout_range": ("arg", 8),
    "iamf_hip_batch_render_lpcm": ("args", 2),
    "iamf_hip_batch_render_lpcm_range": ("args", 2),
    "iamf_hip_batch_render_fanout_lpcm": ("arg", 7),
    "iamf_hip_batch_set_gains_range": ("arg", 4),
    "iamf_hip_batch_restart_range": ("arg", 4),
    "iamf_hip_batch_export_range": ("arg", 6),
    "iamf_hip_batch_import_range": ("arg", 6),
    "iamf_hip_resampler_process": ("arg", 6),
    "iamf_hip_resampler_flush": ("arg", 3),
    "iamf_hip_resampler_process_range": ("arg", 6),
    "iamf_hip_resampler_flush_range": ("arg", 3),
    "iamf_hip_resampler_restart_range": ("arg", 3),
    "iamf_hip_resampler_export_range": ("arg", 6),
    "iamf_hip_resampler_import_range": ("arg", 6),
    "iamf_hip_lpcm_unpack": ("arg", 8),
    "iamf_hip_upload_by_kernel": ("arg", 3),
    "iamf_hip_stream_signal": ("arg", 0),
    "iamf_hip_deinterleave_f32": ("arg", 8),
    "iamf_hip_probe_traffic": ("arg", 8),
    "iamf_hip_pick_buffer_pair": ("arg", 10),
}


def header_stream_entries(text):
    """{prototype name: ("arg", i) | ("args", i)} of a header's text, by the rule above ENTRIES (a `void *stream`
    argument wins where a prototype has both)"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for name, params in re.findall(r"\b(iamf_hip_\w+)\s*\(([^()]*)\)\s*;", text):
        ps = [" ".join(p.split()) for p in params.split(",")]
        st = [i for i, p in enumerate(ps) if re.fullmatch(r"void \*\s?(const )?stream", p)]
        ra = [i for i, p in enumerate(ps) if re.fullmatch(r"(const )?(struct )?iamf_hip_render_args \*\s?(const )?\w+", p)]
        lp = [i for i, p in enumerate(ps) if re.fullmatch(r"(const )?(struct )?iamf_hip_lpcm_input \*\s?(const )?\w+", p)]
        if st:
            out[name] = ("arg", st[0])
        elif ra:
            out[name] = ("args", ra[0])
        elif lp:
            out[name] = ("lpcm", lp[0])     # a prototype with the packets and no stream: ENTRIES has no such form
    return out


# ------------------------------------------------------------------------------------------
# the HIP runtime the process has loaded (torch's and the library's: one instance)
# ------------------------------------------------------------------------------------------
_hip = None


def hip_runtime():
    global _hip
    if _hip is None:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "no HIP runtime is loaded: make a torch.cuda call first"
        _hip = C.CDLL(path)
        _hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    return _hip


def stream_flags(handle):
    """hipStreamGetFlags of a raw hipStream_t (int)"""
    flags = C.c_uint(0xFFFFFFFF)
    r = hip_runtime().hipStreamGetFlags(C.c_void_p(handle), C.byref(flags))
    assert r == 0, "hipStreamGetFlags: %d" % r
    return flags.value


def assert_non_blocking(handle):
    assert handle, "the null stream is no side stream"
    fl = stream_flags(handle)
    assert fl & HIP_STREAM_NON_BLOCKING, "stream %#x has flags %#x: it is a blocking stream" % (handle, fl)


@contextlib.contextmanager
def side_stream():
    """A fresh stream of the caller's, proven non-blocking with respect to the null stream, as torch's current stream of
    the calling thread (the builders of the GPU tests take torch.cuda.current_stream()).  Leaves with the stream drained
    and the thread's earlier stream current again."""
    import torch
    s = torch.cuda.Stream()
    assert_non_blocking(s.cuda_stream)
    before = torch.cuda.current_stream()
    torch.cuda.set_stream(s)
    try:
        yield s
    finally:
        torch.cuda.set_stream(before)
        s.synchronize()


# ------------------------------------------------------------------------------------------
# the stall
# ------------------------------------------------------------------------------------------
_cal = None
_cal_lock = threading.Lock()


def calibrate():
    """cycles of torch.cuda._sleep per millisecond, measured once per process with events (and printed)"""
    global _cal
    with _cal_lock:
        if _cal is None:
            import torch
            s = torch.cuda.Stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def spin_ms(cycles):
                with torch.cuda.stream(s):
                    e0.record()
                    torch.cuda._sleep(int(cycles))
                    e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            spin_ms(10000)                       # the spin kernel's first launch loads it
            cycles, ms = 50000, 0.0
            while True:                          # from well under a millisecond upwards: never a long spin by accident
                ms = spin_ms(cycles)
                if ms >= 1.0 or cycles >= 10 ** 9:
                    break
                cycles *= 4
            assert 1.0 <= ms <= MAX_STALL_MS, "torch.cuda._sleep(%d) took %.3f ms: the spin does not spin" % (cycles, ms)
            per_ms = cycles / ms
            check = spin_ms(per_ms * STALL_MS)
            assert 0.5 * STALL_MS <= check <= min(5 * STALL_MS, MAX_STALL_MS), (per_ms, check)
            print("stream_util: %.0f spin cycles per ms; a %.1f ms stall measured %.2f ms" % (per_ms, STALL_MS, check))
            _cal = per_ms
    return _cal


def stall(stream, ms=STALL_MS):
    """Queues a spin of about `ms` milliseconds on `stream` (a torch stream) and returns an event behind it:
    event.query() is False while the stall runs."""
    assert 0 < ms <= MAX_STALL_MS, ms
    import torch
    cycles = int(calibrate() * ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def torch_stream(handle):
    """the torch stream of a raw hipStream_t (None / 0: the legacy null stream)"""
    import torch
    return torch.cuda.ExternalStream(handle) if handle else torch.cuda.default_stream()


def _handle(v):
    if v is None:
        return 0
    if isinstance(v, C.c_void_p):
        return v.value or 0
    return int(v)


def stream_of(name, args):
    """the raw stream handle a call of entry `name` with these ctypes arguments runs on"""
    how, i = ENTRIES[name]
    if len(args) <= i:
        return 0
    a = args[i]
    if how == "arg":
        return _handle(a)
    a = getattr(a, "_obj", a)                   # byref(struct) -> the struct
    a = getattr(a, "contents", a)               # pointer(struct) -> the struct
    return _handle(a.stream)


Stalled = collections.namedtuple("Stalled", "entry where result running_after")


@contextlib.contextmanager
def stalled(where, ms=STALL_MS):
    """Inside, every stream-taking entry of iac_amd.lib() (ENTRIES) has a stall queued in front of it: on the legacy null
    stream (NULL: a caller-owned non-blocking stream must neither wait for it nor be overtaken by work the library leaves
    on the null stream) or on the call's own stream (SAME: the call's device work cannot start before the call returns).
    Before entering the library the wrapper asserts that the call's stream is a non-null, non-blocking one and that the
    stall has not finished; behind the call it records whether the stall was still running.  Yields the list of records
    (Stalled)."""
    assert where in (NULL, SAME) and 0 < ms <= MAX_STALL_MS
    import iac_amd as A
    L = A.lib()
    calibrate()
    log = []
    saved = {}

    def wrap(name, fn):
        def call(*args):
            h = stream_of(name, args)
            assert_non_blocking(h)
            ev = stall(torch_stream(0 if where == NULL else h), ms)
            assert not ev.query(), "%s: the stall in front of the call had finished before the call was made" % name
            r = fn(*args)
            log.append(Stalled(name, where, r, not ev.query()))
            return r
        return call

    for name in ENTRIES:
        saved[name] = getattr(L, name)
        setattr(L, name, wrap(name, saved[name]))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)
