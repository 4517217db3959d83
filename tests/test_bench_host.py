"""Host side of bench.py, no GPU: the step payloads it makes are the package's LCG payloads, and --dump-outputs writes float
files of a bounded size, the same from run to run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_lcg_steps_are_the_package_payloads(pkg):
    n, frames = 5000, 3  # (not a whole number of blocks)
    for L, seed, threads in ((160, 0x9E3779B9, 1), (40, 0x1234567, 3)):
        want = pkg.lcg_payloads(n, frames, L, seed_base=seed)
        got = list(bench.lcg_steps(np.arange(n), frames, L, seed, threads=threads))
        assert len(got) == frames
        for f in range(frames):
            assert got[f].dtype == np.uint8 and np.array_equal(got[f], want[f])
        ids = np.array([0, 7, 2048, 4999])
        sub = np.stack(list(bench.lcg_steps(ids, frames, L, seed)))
        assert np.array_equal(sub, want[:, ids])


def test_dump_outputs_sizes_types_and_sample(tmp_path):
    n = 65536  # the headline workload's batch
    rng = np.random.default_rng(1)
    pcm = rng.integers(-32768, 32768, (n, 960, 2), dtype=np.int16)
    res = np.full(n, 960, dtype=np.int32)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), pcm, res)
    bench.dump_outputs(str(b), pcm, res)
    names = sorted(os.listdir(a))
    assert names == ["pcm.npy", "pcm_energy.npy", "pcm_streams.npy", "result.npy"]
    assert sum(os.path.getsize(a / f) for f in names) < 64 << 20
    for f in names:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y)
    ids = np.load(a / "pcm_streams.npy").astype(np.int64)
    assert len(ids) > 4096 and np.all(np.diff(ids) > 0)
    assert np.array_equal(np.load(a / "pcm.npy"), pcm[ids].astype(np.float32))
    energy = (pcm.reshape(n, -1).astype(np.int64) ** 2).sum(axis=1)
    assert np.array_equal(np.load(a / "pcm_energy.npy"), energy.astype(np.float64))
    assert np.array_equal(np.load(a / "result.npy"), res.astype(np.float64))
