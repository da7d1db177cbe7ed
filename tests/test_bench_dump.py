"""CPU: bench.py --dump-outputs writes the decoded units as fp32 .npy, and a fixed seeded subset of whole units above the cap."""
import numpy as np
import torch

import bench


def test_dump_outputs_whole(tmp_path):
    x = torch.rand(3, 3, 8, 8, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), x)
    a = np.load(tmp_path / "decoded_units.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.float().numpy())
    assert not (tmp_path / "decoded_units_index.npy").exists()


def test_dump_outputs_sampled_under_cap(tmp_path, monkeypatch):
    x = torch.rand(10, 3, 8, 8)
    per = x[0].numel() * 4 + 8
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 4 * per)
    bench.dump_outputs(str(tmp_path), x)
    a = np.load(tmp_path / "decoded_units.npy")
    idx = np.load(tmp_path / "decoded_units_index.npy")
    assert a.shape[0] == 4 and idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a, x.numpy()[idx.astype(np.int64)])
    bench.dump_outputs(str(tmp_path), x)                        # the same subset every time
    assert np.array_equal(np.load(tmp_path / "decoded_units_index.npy"), idx)
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 30)
    bench.dump_outputs(str(tmp_path), x)                        # a whole dump removes a stale index file
    assert not (tmp_path / "decoded_units_index.npy").exists()
