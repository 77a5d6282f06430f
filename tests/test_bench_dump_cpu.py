"""bench.py --dump-outputs on the host: Workload.dump_outputs turns the packed s16 PCM of a launch into float32 arrays that
hold the int16 values exactly, samples the same streams every time and keeps under its byte budget."""
import numpy as np
import torch

import bench


def fake_workload(S, n, ch):
    wl = bench.Workload.__new__(bench.Workload)
    wl.S, wl.out_ch, wl.last_n = S, ch, n
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32768, size=(S, n, ch)).astype(np.int16)
    stride = n * ch * 2 + 512   # padded rows, as the bench's PCM buffers may be
    buf = np.zeros((S, stride), dtype=np.uint8)
    buf[:, :n * ch * 2] = pcm.reshape(S, -1).view(np.uint8)
    return wl, torch.from_numpy(buf), pcm


def test_everything_fits_every_stream_is_written(tmp_path):
    wl, buf, pcm = fake_workload(8, 300, 2)
    info = wl.dump_outputs(buf, str(tmp_path))
    got, ids = np.load(tmp_path / "pcm.npy"), np.load(tmp_path / "pcm_streams.npy")
    assert got.dtype == np.float32 and ids.dtype == np.float64
    assert np.array_equal(ids, np.arange(8)) and info["pcm"] == [8, 300, 2]
    assert np.array_equal(got, pcm.astype(np.float32))


def test_over_budget_a_fixed_sample_of_streams(tmp_path):
    wl, buf, pcm = fake_workload(64, 256, 6)
    budget = 10 * 256 * 6 * 4 + 100
    wl.dump_outputs(buf, str(tmp_path / "a"), budget_bytes=budget)
    wl.dump_outputs(buf, str(tmp_path / "b"), budget_bytes=budget)
    a, ids = np.load(tmp_path / "a" / "pcm.npy"), np.load(tmp_path / "a" / "pcm_streams.npy")
    assert a.nbytes <= budget and a.shape == (10, 256, 6)
    assert np.array_equal(ids, np.load(tmp_path / "b" / "pcm_streams.npy"))
    assert np.array_equal(a, np.load(tmp_path / "b" / "pcm.npy"))
    assert len(set(ids.tolist())) == 10 and np.all(np.diff(ids) > 0)
    assert np.array_equal(a, pcm[ids.astype(np.int64)].astype(np.float32))


def test_one_stream_over_budget_keeps_its_first_samples(tmp_path):
    wl, buf, pcm = fake_workload(3, 1000, 2)
    wl.dump_outputs(buf, str(tmp_path), budget_bytes=800)
    got = np.load(tmp_path / "pcm.npy")
    assert got.nbytes <= 800 and got.shape == (1, 100, 2)
    ids = np.load(tmp_path / "pcm_streams.npy").astype(np.int64)
    assert np.array_equal(got[0], pcm[ids[0], :100].astype(np.float32))
