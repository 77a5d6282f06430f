"""One smallest case per kernel instance of the library's EXTENSION table (iamf_hip_route_instances_ext): the instances
added behind the table tests/route_cases.py pins.  tests/test_route_ext_coverage_cpu.py holds the cases against the
listing (no GPU); tests/test_gpu_route_ext_coverage.py runs each against the oracle and asserts the extension tally."""
import numpy as np

import route_cases as R
from route_cases import Case

# the lists of render_route.hpp, restated: tests/test_route_ext_coverage_cpu.py fails when they drift
FAN_LP_M = [4, 9, 16]
FAN_LP_K = [2, 3, 4]


def run_fanout_lpcm(c):
    """a mono-coded ambisonics element as 16-bit LPCM packets into K one- and two-channel batches in one launch
    (render_fanout_kernel<M, K, LP>); kw: m, k"""
    import torch
    import iac_amd as A
    import lpcm_util as LP
    import oracle_lib as O
    m, K = c.kw["m"], c.kw["k"]
    S, fs, calls = R.S, 1024, [1, 3, 2]
    F = sum(calls)
    ocs = [2, 1, 2, 1][:K]
    gains = [(R.EG, R.OG), (R.OG, R.EG), ([1.1, 0.9, 1.0], R.OG), (R.EG, [1.0, 1.0, 1.1])][:K]
    # seeded matrices whose weights add up to 1.4 per output: full-scale bursts on every channel at once pass the threshold
    mxs = [R.matrices(m, oc, table=False, salt=j) for j, oc in enumerate(ocs)]
    rng = np.random.default_rng(300 + 16 * m + K)
    ints = LP.ints(rng, S, F, m, fs, 2)
    ints[:, :, :, ::97] = (31000 * (-1) ** np.arange(ints[0, 0, 0, ::97].size))[None, None, None, :]
    perm = list(rng.permutation(m))
    x = (ints[:, :, perm, :].astype(np.float64) / 32768.0).astype(np.float32)
    planar = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(S, m, F * fs)
    for j in range(K):   # every member's limiter must work, in every stream
        for s in range(S):
            peak = float(np.abs(O.render(mxs[j][1], planar[s], ocs[j])).max()) * gains[j][0][s] * gains[j][1][s]
            assert peak > 0.95, ("the programme does not drive the limiter", j, s, peak)
    raw, L, row = LP.rows(ints, 2, True, [1] * m, perm, head=16, pad=0, frame_size=fs)
    d_raw = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    batches = []
    for j in range(K):
        b = A.Batch(S, mxs[j][0], ocs[j], frame_size=fs, projection=A.PROJ_EXACT)
        b.set_gains(element=gains[j][0], output=gains[j][1])
        batches.append(b)
    outs = [[[] for _ in range(S)] for _ in range(K)]

    def take(j, pcm, n):
        torch.cuda.synchronize()
        h = pcm.cpu().numpy()
        for s in range(S):
            outs[j][s].append(h[s][:n * ocs[j] * 2].view(np.int16).reshape(n, ocs[j]).copy())

    A.route_reset()
    A.route_tally_ext(reset=True)
    try:
        f0 = 0
        for nf in calls:
            caps = [(nf * fs * oc * 2 + 15) & ~15 for oc in ocs]
            pcms = [torch.zeros((S, cap), dtype=torch.uint8, device="cuda") for cap in caps]
            inp = A.LpcmInput()
            inp.d_raw, inp.raw_stream_stride, inp.raw_frame_stride, inp.layout = d_raw.data_ptr() + f0 * row, F * row, row, L
            n_emitted, report = A.render_fanout_lpcm(batches, inp, nf, [p.data_ptr() for p in pcms], caps, st)
            assert report == (K, 1, 0), report
            for j in range(K):
                take(j, pcms[j], n_emitted[j])
            f0 += nf
        for j, b in enumerate(batches):
            cap = (240 * ocs[j] * 2 + 15) & ~15
            pcm = torch.zeros((S, cap), dtype=torch.uint8, device="cuda")
            take(j, pcm, b.flush(pcm.data_ptr(), cap, st))
    finally:
        for b in batches:
            b.close()
    ext, base = A.route_tally_ext(), A.route_tally()
    for j in range(K):
        for s in range(S):
            want = O.stream_run(mxs[j][1], ocs[j], planar[s], fs, element_gain=gains[j][0][s], output_gain=gains[j][1][s])
            R.compare(np.concatenate(outs[j][s]), want, 0, (c.id, j, s))
    R.check_tally(ext, [(c.inst, len(calls))])
    R.check_tally(base, [(R.gen(m), K)])      # the members' flushes; the shared launch is no row of the base tally


CASES = [Case("fanout_lpcm_m%d_k%d" % (m, k), ("FANOUT_LPCM", 0, m, 0, k), run_fanout_lpcm, dict(m=m, k=k))
         for m in FAN_LP_M for k in FAN_LP_K]
