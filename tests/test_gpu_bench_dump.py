"""-m gpu: bench.py --dump-outputs writes what the last timed launch computed.  Two runs with the same arguments dump the
same arrays, and what is dumped is the oracle's PCM for the last of the run's launches over the same programme."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, F, FS, STEPS, WARMUP, REPEATS = 16, 4, 1024, 3, 1, 1


def run_bench(out_dir):
    env = dict(os.environ)
    for k in ("IAMF_BENCH_CHILD", "RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(S), "--frames", str(F),
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--repeats", str(REPEATS), "--placement-tries", "1",
                        "--no-cpu-baseline", "--no-extra-configs", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_dump_is_reproducible_and_is_the_last_launch(tmp_path):
    import torch

    import bench
    import bench_verify as V
    import oracle_lib as O
    d1 = run_bench(str(tmp_path / "a"))
    run_bench(str(tmp_path / "b"))
    assert d1["steps"] == STEPS and d1["repeats"]["steps_each"] == STEPS
    assert d1["dumped_outputs"]["pcm"] == [S, F * FS, 2]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["pcm.npy", "pcm_streams.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    a, b = np.load(tmp_path / "a" / "pcm.npy"), np.load(tmp_path / "b" / "pcm.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "pcm_streams.npy"), np.arange(S))
    # launches on the headline's stream state: warm-up, then one discarded region and REPEATS reported ones, same input each
    launches = WARMUP + (REPEATS + 1) * STEPS
    x = bench.synth_hot_device(S, 16, F, FS, 1000, torch.device("cuda", 0)).cpu().numpy()
    mx = O.get_h2m(3, O.SS["BINAURAL"])
    for s in (0, S - 1):
        xp = np.tile(V.planar(x[s]), (1, launches))
        want = O.stream_run(mx, 2, xp, FS, flush=False)[-F * FS:]
        assert np.array_equal(a[s], want.astype(np.float32)), s
