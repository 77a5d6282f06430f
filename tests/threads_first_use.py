"""Child process of tests/test_gpu_streams.py: the first render launches of a process, made by four host threads at once.

Every thread has a side stream of its own (stream_util.side_stream) and a batch of its own, and waits at a barrier in
front of its first library call.  All four kernels take more than 64 KiB of LDS, so each thread's first launch goes through
the per-kernel, per-device opt-in of launch_big_lds (iac_amd/csrc/render_common.hpp), threads 0 and 1 through the SAME
instance's.  Prints one JSON line: {"hashes": {job: [sha1 of the PCM of stream 0, 1, 2]}, "tally": [[instance, launches]]};
the parent holds both against the oracle."""
import hashlib
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CALLS = [1, 3, 2]
# job -> (inputs, output channels, frame size, seed): two threads on render_fast_kernel<16, 2>, one on
# render_wide4_kernel<12, 12>, one on render_wide_kernel<12> (11 channels)
JOBS = {"fast_a": (16, 2, 1024, 900), "fast_b": (16, 2, 1024, 1700), "wide4": (12, 12, 1024, 900), "wide": (12, 11, 256, 900)}


def programme(job):
    """(product matrix, oracle matrix, x [S][m][total]) of a job, as route_cases.run_matrix makes them"""
    import oracle_lib as O
    import route_cases as R
    m, oc, fs, seed = JOBS[job]
    mx, omx = R.matrices(m, oc)
    x = R.drive_limiter(O, omx, oc, R.hot(m, sum(CALLS), fs, seed=seed))
    return mx, omx, x


def expected_tally():
    import route_cases as R
    return {("FAST", 0, 16, 2, 0): 2 * len(CALLS), ("WIDE4", 0, 12, 12, 0): len(CALLS), ("WIDE", 0, 12, 0, 0): len(CALLS),
            R.gen(16): 2, R.gen(12): 2}


def digest(pcm):
    import numpy as np
    return hashlib.sha1(np.ascontiguousarray(pcm, dtype=np.int16).tobytes()).hexdigest()


def main():
    import torch
    import gpu_util as G
    import iac_amd as A
    import route_cases as R
    import stream_util as SU
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")       # a context; no kernel of the library has run
    progs = {job: programme(job) for job in JOBS}
    A.route_reset()
    barrier = threading.Barrier(len(JOBS))
    out, errors = {}, []

    def work(job):
        try:
            m, oc, fs, _ = JOBS[job]
            mx, _, x = progs[job]
            with SU.side_stream():
                barrier.wait(timeout=60)
                got = G.hip_render(mx, oc, x, frame_size=fs, frames_per_call=CALLS, gains=dict(element=R.EG, output=R.OG),
                                   projection=A.PROJ_EXACT)
            out[job] = [digest(g) for g in got]
        except BaseException as e:     # reported by the parent
            barrier.abort()
            errors.append("%s: %r" % (job, e))

    threads = [threading.Thread(target=work, args=(job,)) for job in JOBS]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors and len(out) == len(JOBS), errors
    tally = sorted([list(k), v] for k, v in A.route_tally().items())
    print(json.dumps({"hashes": out, "tally": tally}))


if __name__ == "__main__":
    main()
