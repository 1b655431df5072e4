"""bench.py --dump-outputs (dump_outputs): the files, their float dtypes, the 64 MB bound and the seeded sample, on results
made up on the host (the GPU runs of bench.py are in test_bench_rehearsal.py)."""
import os

import numpy as np
import torch

import bench
from conftest import load_package


def _batch(lengths, stride):
    fl = load_package()
    rng = np.random.default_rng(3)
    rows = torch.from_numpy(rng.integers(0, 256, (len(lengths), stride), dtype=np.uint8))
    dsts = [fl.flgpu_image(0, stride, 300, 200, 4, 1, b) for b in lengths]
    return dsts, rows


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("output_bytes", "output_meta", "sample_index", "outputs")}


def test_dump_holds_the_sampled_bytes_and_every_length(tmp_path):
    lengths = [1000 + 37 * i for i in range(300)]             # (up to 12,063 bytes)
    dsts, rows = _batch(lengths, 12288)
    k = bench.dump_outputs(str(tmp_path / "a"), dsts, lambda i: rows[i])
    got = _load(str(tmp_path / "a"))
    assert k == bench.DUMP_SAMPLE == len(got["sample_index"])
    assert got["output_bytes"].dtype == got["output_meta"].dtype == got["sample_index"].dtype == np.float64
    assert got["outputs"].dtype == np.float32
    assert np.array_equal(got["output_bytes"], lengths) and got["output_meta"].shape == (300, 4)
    assert np.array_equal(got["output_meta"][7], [300, 200, 4, 1])
    idx = got["sample_index"].astype(np.int64)
    assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < 300
    want = np.concatenate([rows[i][:lengths[i]].numpy() for i in idx]).astype(np.float32)
    assert np.array_equal(got["outputs"], want)
    # the same batch again: the same files
    bench.dump_outputs(str(tmp_path / "b"), dsts, lambda i: rows[i])
    again = _load(str(tmp_path / "b"))
    assert all(np.array_equal(got[n], again[n]) for n in got)


def test_dump_stays_within_64_mb(tmp_path):
    stride = 600_000                                           # 4 x 600 kB x 256 images would be ~600 MB of float32
    dsts, rows = _batch([stride] * 40, stride)
    k = bench.dump_outputs(str(tmp_path), dsts, lambda i: rows[i])
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert 0 < k < 40 and total <= 64 << 20
    assert len(np.load(os.path.join(tmp_path, "outputs.npy"))) == k * stride
